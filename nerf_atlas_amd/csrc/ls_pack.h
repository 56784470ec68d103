// Weight-stream packing of the bf16 / bf16x3 / f16 schedules and the launch of render_ls_kernel (the NA_PREC_F16X streams are
// built from schedule tables: ls_xsched.h).
#pragma once
#include "ls_kernel.h"

namespace na {
namespace ls {

// ================================================================================================ pack
#if NA_PREC_INST == 0
// dir_to_elev_azim of every ray, once (src/utils.py:247-254): the View MLP's geometry chunk reads it per block
__global__ void ray_elaz_kernel(const float* __restrict__ rays, int64_t R, float* __restrict__ elaz) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    float el, az;
    elev_azim(rays[r * 6 + 3], rays[r * 6 + 4], rays[r * 6 + 5], el, az);
    elaz[r * 2] = el;
    elaz[r * 2 + 1] = az;
  }
}

__global__ void pack_ls_header_kernel(uint32_t magic, uint32_t precision, uint32_t* __restrict__ dst, uint32_t pairs) {
  if (threadIdx.x == 0) { dst[0] = magic; dst[1] = precision; dst[2] = pairs; dst[3] = kNPhase; }
}

// ---- what the five pack kernels share.  A stream = header | [row group][phase] bias blocks | [row group][fragment] weights; a pack
// kernel runs one thread per bf16 element of the hi plane of every fragment (4 row groups x 2 * pairs fragments x 512), then one per
// bias float (4 x kNPhase x 256), and differs from the others only in its schedule's map: which Linear, row and column an element holds.
struct PackElem { int e, l, rg, f, p, kappa; int64_t frag; };  // element e of lane l; fragment `frag` of row group rg = fragment f of phase p
template <int (*PHASE_PAIRS)(int)>
__device__ inline PackElem pack_elem(int64_t i, int64_t nfrag_rg) {
  PackElem x;
  x.e = (int)(i & 7); x.l = (int)((i >> 3) & 63);
  const int64_t fg = i >> 9;
  x.rg = (int)(fg / nfrag_rg);
  x.frag = fg % nfrag_rg;
  x.f = (int)x.frag; x.p = 0;
  while (x.f >= 2 * PHASE_PAIRS(x.p)) { x.f -= 2 * PHASE_PAIRS(x.p); ++x.p; }
  x.kappa = 8 * (x.l >> 5) + x.e;
  return x;
}

// the element's hi value (bf16, or f16 for NA_PREC_F16) and, in the two-plane format, the bf16 of what the hi value missed
__device__ inline void pack_store_elem(char* __restrict__ dst, const PackElem& x, int64_t nfrag_rg, int planes, int f16, float v) {
  char* o = dst + kHeaderBytes + kBiasBytes + ((int64_t)x.rg * nfrag_rg + x.frag) * (1024 * planes) + x.l * 16 + x.e * 2;
  const __bf16 h = f16 ? to_elem<NA_PREC_F16>(v) : (__bf16)v;
  *(uint16_t*)o = __builtin_bit_cast(uint16_t, h);
  if (planes == 2) {
    const __bf16 lo = (__bf16)(v - (float)h);
    *(uint16_t*)(o + 1024) = __builtin_bit_cast(uint16_t, lo);
  }
}

struct PackBias { int k, p, rg, slot, rin; };  // float k of the block of (row group rg, phase p): row rin of the 32-row tile in `slot`
__device__ inline PackBias pack_bias(int64_t q) {
  PackBias b;
  b.k = (int)(q & 255); b.p = (int)((q >> 8) % kNPhase); b.rg = (int)((q >> 8) / kNPhase);
  const int hi = (b.k >> 4) & 1, r = b.k & 15;
  b.slot = b.k >> 5;
  b.rin = (r & 3) + 8 * (r >> 2) + 4 * hi;
  return b;
}
__device__ inline void pack_store_bias(char* __restrict__ dst, const PackBias& b, float v) {
  *(float*)(dst + kHeaderBytes + ((int64_t)b.rg * kNPhase + b.p) * 1024 + b.k * 4) = v;
}

// where an element comes from: W[row * in_dim + col] of an nn.Linear [out_dim, in_dim], zero outside it (padding rows, slots and fragments)
struct PackSrc { int row = -1, col = -1, in_dim = 1, out_dim = 0; };
__device__ inline float pack_weight(const float* __restrict__ W, const PackSrc& m) {
  return m.row >= 0 && m.row < m.out_dim && m.col >= 0 && m.col < m.in_dim ? W[(int64_t)m.row * m.in_dim + m.col] : 0.f;
}

// column of chunk q of a skip layer.  Stream order [nlds init chunks (from LDS) | the 16 hidden chunks | (View) the geometry chunk];
// the reference's column order is [hidden | init]
__device__ inline int skip_col(const NaMlpDesc& d, int q, int kappa, int nlds) {
  if (q >= nlds && q < nlds + kHC) return 16 * (q - nlds) + pi_perm(kappa);
  const int col = init_slot_feature(d, q < nlds ? q : 4, kappa);
  return col >= 0 ? col + kHidden : col;
}

// A 256-row Linear: row group rg holds rows 64 rg .. + 63, fragment f = (chunk f >> 1, tile f & 1).  kind 0: the init Linear (ninit
// init chunks, anything behind them zero), 1: a skip layer (skip_col), 2: hidden -> hidden
__device__ inline PackSrc hidden_src(const NaMlpDesc& d, int kind, int ninit, int nlds, const PackElem& x) {
  const int q = x.f >> 1, t = x.f & 1, dim_p = d.in_size + d.enc_dims + d.latent_size;
  PackSrc m;
  m.row = 32 * (2 * x.rg + t) + (x.l & 31);
  m.out_dim = kHidden;
  if (kind == 0) { m.col = q < ninit ? init_slot_feature(d, q, x.kappa) : -1; m.in_dim = dim_p; }
  else if (kind == 1) { m.col = skip_col(d, q, x.kappa, nlds); m.in_dim = kHidden + dim_p; }
  else { m.col = 16 * q + pi_perm(x.kappa); m.in_dim = kHidden; }
  return m;
}
__device__ inline float hidden_bias(const float* __restrict__ B, const PackBias& b) { return b.slot < 2 ? B[32 * (2 * b.rg + b.slot) + b.rin] : 0.f; }

// An out Linear: fragment f = chunk f of ONE 32-row tile (fragments 16.. of a padded out phase are zero); its bias block holds
// `tiles` tiles from tile0 on in slots 0..
__device__ inline PackSrc out_src(const NaMlpDesc& d, int tile, const PackElem& x) {
  PackSrc m;
  if (x.f < 16) { m.row = out_row_map(d, 32 * tile + (x.l & 31)); m.col = 16 * x.f + pi_perm(x.kappa); m.in_dim = kHidden; m.out_dim = d.out_size; }
  return m;
}
__device__ inline float out_bias(const NaMlpDesc& d, const float* __restrict__ B, int tiles, int tile0, const PackBias& b) {
  const int row = b.slot < tiles ? out_row_map(d, 32 * (tile0 + b.slot) + b.rin) : -1;
  return row >= 0 && row < d.out_size ? B[row] : 0.f;
}
// a 65-row out Linear (density + latent; the SIREN's distance + latent) runs block-per-wave: row group rg holds tile min(rg, 2), all three biases
__device__ inline PackSrc out65_src(const NaMlpDesc& d, const PackElem& x) { return out_src(d, x.rg < 2 ? x.rg : 2, x); }
__device__ inline float out65_bias(const NaMlpDesc& d, const float* __restrict__ B, const PackBias& b) { return out_bias(d, B, 3, 0, b); }

// The View MLP (refl.View: [x, y, z, elev, azim | 64 latent] -> 4 x 256 sin -> 3) at its own phase lp: 0 init (4 latent chunks + the
// geometry chunk), 1 the skip layer, 2..4 hidden, 5 out.  PlainNeRF, the View half alone and SIREN-VolSDF end in it.
__device__ inline NaMlpDesc view_mlp_desc() { return {5, NA_ENC_NONE, 0, 64, 4, 256, 3, 3, NA_ACT_SIN, NA_LAYOUT_PLAIN_VIEW}; }
__device__ inline PackSrc view_mlp_src(int lp, const PackElem& x) {
  const NaMlpDesc d = view_mlp_desc();
  return lp == 5 ? out_src(d, 0, x) : hidden_src(d, lp < 2 ? lp : 2, 5, 4, x);
}
__device__ inline float view_mlp_bias(const float* __restrict__ B, int lp, const PackBias& b) {
  return lp == 5 ? out_bias(view_mlp_desc(), B, 1, 0, b) : hidden_bias(B, b);
}

constexpr int64_t kPackBiasFloats = 4 * kNPhase * 256;
#define NA_LS_PACK_LOOP(i, pairs) \
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < 4 * 2 * (int64_t)(pairs) * 512 + kPackBiasFloats; i += (int64_t)gridDim.x * blockDim.x)

// ---- PlainNeRF(view) (MODEL 0, 9): first (phases 0..5: init, the skip layer, 3 hidden, out) then the View MLP (6..11)
struct PackArgs {
  const float* w_first[6];  // init, layers.0..3, out   (nn.Linear layout [out,in])
  const float* b_first[6];
  const float* w_view[6];
  const float* b_view[6];
};
__global__ void pack_ls_kernel(PackArgs w, int planes, int f16, char* __restrict__ dst) {
  const NaMlpDesc d1 = {3, NA_ENC_HASH, 35, 0, 4, 256, 65, 3, NA_ACT_LEAKY_RELU, NA_LAYOUT_PLAIN_FIRST};
  const int64_t nfrag_rg = 2 * kPairsPerPass, nelem = 4 * nfrag_rg * 512;
  NA_LS_PACK_LOOP(i, kPairsPerPass) {
    if (i < nelem) {
      const PackElem x = pack_elem<phase_pairs>(i, nfrag_rg);
      const bool view = x.p >= 6;
      const int lp = view ? x.p - 6 : x.p;
      const PackSrc m = view ? view_mlp_src(lp, x) : lp == 5 ? out65_src(d1, x) : hidden_src(d1, lp < 2 ? lp : 2, 3, 3, x);
      pack_store_elem(dst, x, nfrag_rg, planes, f16, pack_weight(view ? w.w_view[lp] : w.w_first[lp], m));
    } else {
      const PackBias b = pack_bias(i - nelem);
      const bool view = b.p >= 6;
      const int lp = view ? b.p - 6 : b.p;
      const float* B = b.p >= 12 ? nullptr : view ? w.b_view[lp] : w.b_first[lp];  // (bias blocks 12..kNPhase-1: other schedules)
      pack_store_bias(dst, b, B == nullptr ? 0.f : view ? view_mlp_bias(B, lp, b) : lp == 5 ? out65_bias(d1, B, b) : hidden_bias(B, b));
    }
  }
}

// ---- TinyNeRF (MODEL 1): phases per tiny_phase_pairs -- init (the x, y, z chunk + one zero chunk), layers.0..5 (skip layers 1 and 4), out
struct TinyPackArgs {
  const float* w[8];  // init, layers.0..5, out   (nn.Linear layout [out,in])
  const float* b[8];
};
__global__ void pack_ls_tiny_kernel(TinyPackArgs w, int planes, int f16, char* __restrict__ dst) {
  const NaMlpDesc d = {3, NA_ENC_NONE, 0, 0, 6, 256, 4, 3, NA_ACT_LEAKY_RELU, NA_LAYOUT_GENERIC};
  const int64_t nfrag_rg = 2 * kTinyPairs, nelem = 4 * nfrag_rg * 512;
  NA_LS_PACK_LOOP(i, kTinyPairs) {
    if (i < nelem) {
      const PackElem x = pack_elem<tiny_phase_pairs>(i, nfrag_rg);
      const PackSrc m = x.p == 7 ? out_src(d, 0, x) : hidden_src(d, x.p == 0 ? 0 : (x.p == 1 || x.p == 4) ? 1 : 2, 1, 1, x);
      pack_store_elem(dst, x, nfrag_rg, planes, f16, pack_weight(w.w[x.p], m));
    } else {
      const PackBias b = pack_bias(i - nelem);
      const float* B = b.p < kTinyPhases ? w.b[b.p] : nullptr;
      pack_store_bias(dst, b, B == nullptr ? 0.f : b.p == 7 ? out_bias(d, B, 1, 0, b) : hidden_bias(B, b));
    }
  }
}

// ---- a hash-encoded SkipConnMLP (MODEL 4 outside f16x, round 6): phases per hashmlp_phase_pairs -- init (3 chunks [hash | x]), layers.0..4
// (skip layers 1 and 4), out: row group rg holds ONE 32-row tile (rows 32 (rg >> 1) ..) and three zero pairs
struct HashMlpPackArgs {
  const float* w[7];  // init, layers.0..4, out   (nn.Linear layout [out,in])
  const float* b[7];
  int n_out;
};
__global__ void pack_ls_hashmlp_kernel(HashMlpPackArgs w, int planes, int f16, char* __restrict__ dst) {
  const NaMlpDesc d = {3, NA_ENC_HASH, 35, 0, 5, 256, w.n_out, 3, NA_ACT_LEAKY_RELU, NA_LAYOUT_GENERIC};
  const int64_t nfrag_rg = 2 * kHashMlpPairs, nelem = 4 * nfrag_rg * 512;
  NA_LS_PACK_LOOP(i, kHashMlpPairs) {
    if (i < nelem) {
      const PackElem x = pack_elem<hashmlp_phase_pairs>(i, nfrag_rg);
      const PackSrc m = x.p == 6 ? out_src(d, x.rg >> 1, x) : hidden_src(d, x.p == 0 ? 0 : (x.p == 1 || x.p == 4) ? 1 : 2, 3, 3, x);
      pack_store_elem(dst, x, nfrag_rg, planes, f16, pack_weight(w.w[x.p], m));
    } else {
      const PackBias b = pack_bias(i - nelem);
      const float* B = b.p < kHashMlpPhases ? w.b[b.p] : nullptr;
      pack_store_bias(dst, b, B == nullptr ? 0.f : b.p == 6 ? out_bias(d, B, 1, b.rg >> 1, b) : hidden_bias(B, b));  // (slot 0 = this row group's tile)
    }
  }
}

// ---- the View head alone (MODEL 2): phases per view_phase_pairs; the last two pairs of the out phase are zero
struct ViewPackArgs {
  const float* w[6];  // init, layers.0..3, out
  const float* b[6];
};
__global__ void pack_ls_view_kernel(ViewPackArgs w, int planes, int f16, char* __restrict__ dst) {
  const int64_t nfrag_rg = 2 * kViewPairs, nelem = 4 * nfrag_rg * 512;
  NA_LS_PACK_LOOP(i, kViewPairs) {
    if (i < nelem) {
      const PackElem x = pack_elem<view_phase_pairs>(i, nfrag_rg);
      pack_store_elem(dst, x, nfrag_rg, planes, f16, pack_weight(w.w[x.p], view_mlp_src(x.p, x)));
    } else {
      const PackBias b = pack_bias(i - nelem);
      const float* B = b.p < kViewPhases ? w.b[b.p] : nullptr;
      pack_store_bias(dst, b, B == nullptr ? 0.f : view_mlp_bias(B, b.p, b));
    }
  }
}

// ---- SIREN-VolSDF (MODEL 3): the SIREN SDF network (phases 0..6: init, layers.0..4 with skip layers 1 and 4, out 65 rows) then the
// View MLP (7..12)
struct SirenPackArgs {
  const float* ws[7];  // sdf: init, layers.0..4, out
  const float* bs[7];
  const float* wv[6];  // view: init, layers.0..3, out
  const float* bv[6];
};
__global__ void pack_ls_siren_kernel(SirenPackArgs w, int planes, int f16, char* __restrict__ dst) {
  const NaMlpDesc d1 = {3, NA_ENC_NONE, 0, 0, 5, 256, 65, 3, NA_ACT_SIN, NA_LAYOUT_PLAIN_FIRST};
  const int64_t nfrag_rg = 2 * kSirenPairs, nelem = 4 * nfrag_rg * 512;
  NA_LS_PACK_LOOP(i, kSirenPairs) {
    if (i < nelem) {
      const PackElem x = pack_elem<siren_phase_pairs>(i, nfrag_rg);
      const bool view = x.p >= 7;
      const int lp = view ? x.p - 7 : x.p;
      const PackSrc m = view ? view_mlp_src(lp, x) : lp == 6 ? out65_src(d1, x) : hidden_src(d1, lp == 0 ? 0 : (lp == 1 || lp == 4) ? 1 : 2, 1, 1, x);
      pack_store_elem(dst, x, nfrag_rg, planes, f16, pack_weight(view ? w.wv[lp] : w.ws[lp], m));
    } else {
      const PackBias b = pack_bias(i - nelem);
      const bool view = b.p >= 7;
      const int lp = view ? b.p - 7 : b.p;
      const float* B = b.p >= kSirenPhases ? nullptr : view ? w.bv[lp] : w.bs[lp];
      pack_store_bias(dst, b, B == nullptr ? 0.f : view ? view_mlp_bias(B, lp, b) : lp == 6 ? out65_bias(d1, B, b) : hidden_bias(B, b));
    }
  }
}
#undef NA_LS_PACK_LOOP

#endif  // NA_PREC_INST == 0

static std::atomic<uint32_t> g_lsx_launch_id{0};  // ids of the NA_PREC_F16X launches (range guard), shared by every schedule
// per-device hipFuncSetAttribute bookkeeping (the attribute is per device, not per thread)
template <int PREC, int MODEL = 0>
static int launch(Args& a, hipStream_t stream, const char* what) {
  using C = Cfg<PREC>;
  auto kern = render_ls_kernel<PREC, MODEL>;
  static std::atomic<uint64_t> attr_done{0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) { set_error("hipGetDevice failed"); return NA_EHIP; }
  const uint64_t bit = 1ull << (dev & 63);
  if (!(attr_done.load(std::memory_order_acquire) & bit)) {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e)); return NA_EHIP; }
    attr_done.fetch_or(bit, std::memory_order_release);
  }
  const int64_t wgs = (a.R + 1) / 2;  // at least one ray per sample group
  const int grid = wgs < 256 ? (int)wgs : 256;
  a.nG = 2 * grid;
  const int64_t rays_per_group = (a.R + a.nG - 1) / a.nG;
  a.npg = (int)((rays_per_group * a.nb + C::NBLK - 1) / C::NBLK);
  a.nb_magic = (1ull << 32) / (uint64_t)a.nb + 1;
  if ((int64_t)(a.npg + 1) * C::NBLK * a.nb >= (1ll << 32)) { set_error("%s: batch too large", what); return NA_EINVAL; }
  if constexpr (PREC == NA_PREC_F16X) {
    // ONE counter for all schedules: the flag ring is shared, and a stale id left by a saturated launch of one schedule
    // must never equal the id of a later launch of another (a per-instantiation counter did exactly that: the frame after
    // tests/test_gpu_range.py's saturated PlainNeRF launch came out poisoned in whichever VolSDF kernel reached the same count)
    uint32_t g = g_lsx_launch_id.fetch_add(1, std::memory_order_relaxed) + 1;
    if (g == 0) g = g_lsx_launch_id.fetch_add(1, std::memory_order_relaxed) + 1;  // (0 is the flag's initial value: never an id)
    a.sat_gen = g;
  } else {
    a.sat_gen = 0;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 2 * C::GROUP, stream, a);
  if constexpr (PREC == NA_PREC_F16X) {  // range guard: NaN output if any activation of this launch sat at the half clamp
    if constexpr (MODEL == 4 || MODEL == 5)
      hipLaunchKernelGGL(lsx_poison_kernel, dim3(grid_for((int64_t)a.T * a.R * a.y_ld, 256, 1024)), dim3(256), 0, stream, a.sat_gen, a.y,
                         (int64_t)a.T * a.R * a.y_ld);
    else
      hipLaunchKernelGGL(lsx_poison_kernel, dim3(grid_for(a.R * 3, 256, 256)), dim3(256), 0, stream, a.sat_gen, a.out, a.R * 3);
  }
  return check_launch(what);
}
}  // namespace ls
}  // namespace na
