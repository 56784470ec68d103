// NeRFAE's front (src/nerf.py:766-840): encode = SkipConnMLP(3 -> Fourier 128 -> 5 x 128 -> E), optional F.normalize, density_tform =
// SkipConnMLP(E -> 5 x 64 -> 1 + I), as ONE launch that writes one finished row per sample -- the `feat` row of na_render_view_ls.
//
// Structure.  A wave owns AE_NB blocks of 32 consecutive samples and runs both networks on them alone: no LDS, no barrier.  Every
// Linear is Y^T [out, sample] = W [out, K] . X^T [K, sample] on v_mfma_f32_32x32x16_bf16 with the WEIGHTS as the A operand and the
// activations as the B operand.  A 32 x 32 result tile then has its sample on the lane and its 16 output rows in the lane's
// registers, which is exactly a B fragment of the next Linear: registers 8 s .. 8 s + 7 of a tile are K16 step s, element j of lane
// half h being row 16 s + 8 (j >> 2) + 4 h + (j & 3).  The pack kernel lays every weight matrix out in that k order, so an activation
// goes from accumulator to operand through LeakyReLU and the bf16 split only -- it never leaves the register file.  The 256 Fourier
// features are generated per K16 step (four frequencies per lane: sin, cos) in front of the MFMAs that consume them, in init and
// again, through the activation, in the two skip layers.  Weights stream from L2 as 32 bytes per lane and (tile, K16 step): 16 bytes
// of bf16 hi parts, 16 of lo parts, consumption order.
//
// Arithmetic: the three-product bf16 split, w x ~ w_hi x_hi + w_hi x_lo + w_lo x_hi with fp32 accumulation (operands keep fp32's
// range: no range guard), for every precision the entry point accepts.  A sample's row depends on nothing but its own position: the
// result is bitwise independent of R, of the sample's place in its wave and of the launch shape.
//
// Also here: the two row operators of the model's differentiable path (na_row_normalize, na_row_sqnorm_mean and their backwards).
#include <initializer_list>
#include "common.h"

namespace na {
namespace ae {

typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

constexpr int kFreqs = 128;    // FourierEncoder(input_dims=3): 128 frequencies -> 256 features
constexpr int kLayers = 14;    // 7 Linears per network: init, layers.0..4, out
constexpr int kHE = 128, kHD = 64;
constexpr int AE_NB = 2;       // sample blocks (of 32) per wave

// ---- packed stream.  Linear l: tiles x chunks records of 64 lanes x 32 bytes (hi[8] | lo[8] bf16: A fragment of the 32-row tile for
// one K16 step), then tiles x 32 fp32 biases.  A Linear's K axis is a list of segments in CONSUMPTION order:
//   SEG_ROWS     `width` columns from col0 that arrive as accumulator tiles (hidden activations, the encoding): slot (c, h, e) <->
//                column col0 + 16 c + 8 (e >> 2) + 4 h + (e & 3)
//   SEG_FOURIER  16 steps: slot (c, h, e) <-> frequency f = 8 c + 4 h + (e >> 1), sin (e even, column col0 + f) | cos (col0 + 128 + f)
//   SEG_POS      1 step: slots (0, 0, 0..2) <-> the position columns col0 .. col0 + 2, the rest zero
enum { SEG_ROWS = 0, SEG_FOURIER = 1, SEG_POS = 2 };
struct Seg { int kind, col0, width, chunks; };
struct Layer {
  int out_dim, in_dim, tiles, chunks, nseg;
  Seg seg[3];
  uint32_t w_off, b_off;
};
struct Plan {
  Layer l[kLayers];
  uint32_t bytes;
};
struct Offs { uint32_t w[kLayers], b[kLayers]; };

inline bool supported(int E, int I) { return (E == 16 || E == 32 || E == 64) && (I == 32 || I == 64); }

inline Plan make_plan(int E, int I) {
  Plan p;
  auto rows = [](int col0, int width) { return Seg{SEG_ROWS, col0, width, (width + 15) / 16}; };
  int n = 0;
  auto add = [&](int out_dim, int in_dim, std::initializer_list<Seg> segs) {
    Layer& L = p.l[n++];
    L.out_dim = out_dim; L.in_dim = in_dim; L.tiles = (out_dim + 31) / 32; L.chunks = 0; L.nseg = 0;
    for (const Seg& s : segs) { L.seg[L.nseg++] = s; L.chunks += s.chunks; }
    for (int i = L.nseg; i < 3; ++i) L.seg[i] = Seg{SEG_ROWS, 0, 0, 0};
  };
  const int P = 3 + 2 * kFreqs;  // init row of `encode`: [p | sin | cos]
  const Seg four0 = {SEG_FOURIER, 3, 2 * kFreqs, 16}, pos0 = {SEG_POS, 0, 3, 1};
  const Seg four1 = {SEG_FOURIER, kHE + 3, 2 * kFreqs, 16}, pos1 = {SEG_POS, kHE, 3, 1};
  add(kHE, P, {four0, pos0});                                // encode.init
  add(kHE, kHE + P, {rows(0, kHE), four1, pos1});            // encode.layers.0 (skip)
  add(kHE, kHE, {rows(0, kHE)});
  add(kHE, kHE, {rows(0, kHE)});
  add(kHE, kHE + P, {rows(0, kHE), four1, pos1});            // encode.layers.3 (skip)
  add(kHE, kHE, {rows(0, kHE)});
  add(E, kHE, {rows(0, kHE)});                               // encode.out
  add(kHD, E, {rows(0, E)});                                 // density_tform.init
  add(kHD, kHD + E, {rows(0, kHD), rows(kHD, E)});           // density_tform.layers.0 (skip)
  add(kHD, kHD, {rows(0, kHD)});
  add(kHD, kHD, {rows(0, kHD)});
  add(kHD, kHD + E, {rows(0, kHD), rows(kHD, E)});           // density_tform.layers.3 (skip)
  add(kHD, kHD, {rows(0, kHD)});
  add(1 + I, kHD, {rows(0, kHD)});                           // density_tform.out
  uint32_t off = 0;
  for (int i = 0; i < kLayers; ++i) {
    p.l[i].w_off = off;
    off += (uint32_t)p.l[i].tiles * p.l[i].chunks * 64 * 32;
    p.l[i].b_off = off;
    off += (uint32_t)p.l[i].tiles * 32 * 4;
  }
  p.bytes = off;
  return p;
}

// one thread per (tile, K16 step, lane): its 8 hi + 8 lo bf16; the first tiles * 32 threads also write the bias
__global__ __launch_bounds__(256) void pack_layer_kernel(const float* __restrict__ W, const float* __restrict__ B, Layer L,
                                                         char* __restrict__ packed) {
  const int total = L.tiles * L.chunks * 64;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int lane = idx & 63, rec = idx >> 6;
    const int tile = rec / L.chunks;
    int c = rec - tile * L.chunks;
    const int row = tile * 32 + (lane & 31), h = lane >> 5;
    int s = 0;
    while (s < L.nseg - 1 && c >= L.seg[s].chunks) { c -= L.seg[s].chunks; ++s; }
    const Seg sg = L.seg[s];
    bf16x8 hi, lo;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      int col = -1;
      if (sg.kind == SEG_ROWS) {
        const int k = 16 * c + 8 * (e >> 2) + 4 * h + (e & 3);
        if (k < sg.width) col = sg.col0 + k;
      } else if (sg.kind == SEG_FOURIER) {
        const int f = 8 * c + 4 * h + (e >> 1);
        col = sg.col0 + ((e & 1) ? kFreqs + f : f);
      } else if (h == 0 && e < 3) {
        col = sg.col0 + e;
      }
      const float v = (row < L.out_dim && col >= 0) ? W[(int64_t)row * L.in_dim + col] : 0.f;
      const __bf16 vh = (__bf16)v;
      hi[e] = vh;
      lo[e] = (__bf16)(v - (float)vh);
    }
    bf16x8* dst = (bf16x8*)(packed + L.w_off + (size_t)idx * 32);
    dst[0] = hi;
    dst[1] = lo;
    if (idx < L.tiles * 32) ((float*)(packed + L.b_off))[idx] = (B != nullptr && idx < L.out_dim) ? B[idx] : 0.f;
  }
}

// ---- the kernel
struct Args {
  const float* rays;   // [R,6] (unused with pts)
  const float* pts;    // [T,R,3] or null
  const float* ts;     // [T]
  const float* basis;  // [3,128]
  const char* packed;
  float* y;
  int64_t R, N, y_ld;  // N = T R samples
  int normalize;
  Offs o;
};

struct Frag { bf16x8 hi, lo; };

__device__ __forceinline__ Frag make_frag(const float (&v)[8]) {
  Frag f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 vh = (__bf16)v[j];
    f.hi[j] = vh;
    f.lo[j] = (__bf16)(v[j] - (float)vh);
  }
  return f;
}

// accumulators <- the bias of their rows (register r of a tile: row (r & 3) + 8 (r >> 2) + 4 h)
template <int NT, int NB>
__device__ __forceinline__ void bias_init(f32x16 (&acc)[NT][NB], const float* __restrict__ bias, int h) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *(const f32x4*)(bias + t * 32 + 8 * g + 4 * h);
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][b][4 * g + j] = bv[j];
    }
}

// one K16 step `c` of a Linear with `nch` steps: NT weight records against the NB sample blocks' fragments (small terms first)
template <int NT, int NB>
__device__ __forceinline__ void mma_step(f32x16 (&acc)[NT][NB], const char* __restrict__ w, int nch, int c, const Frag (&x)[NB], int lane) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const bf16x8* wp = (const bf16x8*)(w + ((size_t)(t * nch + c) * 64 + lane) * 32);
    const bf16x8 ah = wp[0], al = wp[1];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, x[b].hi, acc[t][b], 0, 0, 0);
      acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, x[b].lo, acc[t][b], 0, 0, 0);
      acc[t][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, x[b].hi, acc[t][b], 0, 0, 0);
    }
  }
}

// result tiles -> the NCH K16 fragments of the next Linear (step s: tile s / 2, registers 8 (s & 1) ..)
template <bool ACT, int NCH, int NT, int NB>
__device__ __forceinline__ void to_frags(const f32x16 (&acc)[NT][NB], Frag (&x)[NCH][NB]) {
  static_assert(NCH <= 2 * NT, "more steps than rows");
#pragma unroll
  for (int s = 0; s < NCH; ++s)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float r = acc[s >> 1][b][8 * (s & 1) + j];
        v[j] = ACT ? leaky_relu(r) : r;
      }
      x[s][b] = make_frag(v);
    }
}

template <int NCH, int NT, int NB>
__device__ __forceinline__ void rows_part(f32x16 (&acc)[NT][NB], const char* __restrict__ w, int nch, int c0, const Frag (&x)[NCH][NB], int lane) {
#pragma unroll
  for (int c = 0; c < NCH; ++c) mma_step<NT, NB>(acc, w, nch, c0 + c, x[c], lane);
}

// the 16 Fourier steps (src/utils.py:14-17: mapped = x @ basis, [sin | cos]; the argument in na_fourier_encode's order: one product,
// two fmas) + the position step, raw (init) or through the activation (skip layers: the reference activates the whole concatenation)
template <bool ACT, int NT, int NB>
__device__ __forceinline__ void fourier_pos_part(f32x16 (&acc)[NT][NB], const char* __restrict__ w, int nch, int c0,
                                                 const float* __restrict__ basis, const float (&px)[NB], const float (&py)[NB],
                                                 const float (&pz)[NB], int lane) {
  const int h = lane >> 5;
#pragma unroll 1
  for (int c = 0; c < 16; ++c) {
    const int f0 = 8 * c + 4 * h;
    const f32x4 b0 = *(const f32x4*)(basis + f0), b1 = *(const f32x4*)(basis + kFreqs + f0), b2 = *(const f32x4*)(basis + 2 * kFreqs + f0);
    Frag x[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float m = px[b] * b0[j];
        m = fmaf(py[b], b1[j], m);
        m = fmaf(pz[b], b2[j], m);
        float sn, cs;
        fourier_sincos(m, sn, cs);
        v[2 * j] = ACT ? leaky_relu(sn) : sn;
        v[2 * j + 1] = ACT ? leaky_relu(cs) : cs;
      }
      x[b] = make_frag(v);
    }
    mma_step<NT, NB>(acc, w, nch, c0 + c, x, lane);
  }
  Frag x[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (h == 0) {
      v[0] = ACT ? leaky_relu(px[b]) : px[b];
      v[1] = ACT ? leaky_relu(py[b]) : py[b];
      v[2] = ACT ? leaky_relu(pz[b]) : pz[b];
    }
    x[b] = make_frag(v);
  }
  mma_step<NT, NB>(acc, w, nch, c0 + 16, x, lane);
}

template <int E, int I, int NB>
__global__ __launch_bounds__(256) void ae_front_kernel(Args a) {
  constexpr int NTE = (E + 31) / 32, NCE = E / 16;     // tiles / K16 steps of the encoding
  constexpr int NTO = (1 + I + 31) / 32;               // tiles of density_tform.out
  const int lane = threadIdx.x & 63, n = lane & 31, h = lane >> 5;
  const int64_t s0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (32 * NB);
  if (s0 >= a.N) return;  // (wave-uniform; the kernel has no barrier)
  const char* __restrict__ pk = a.packed;
  auto W = [&](int l) { return pk + a.o.w[l]; };
  auto B = [&](int l) { return (const float*)(pk + a.o.b[l]); };

  // ---- positions: explicit, or r_o + t r_d in na_compute_pts's arithmetic
  float px[NB], py[NB], pz[NB];
  bool ok[NB];
  int64_t srow[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int64_t s = s0 + 32 * b + n;
    ok[b] = s < a.N;
    srow[b] = ok[b] ? s : a.N - 1;
    if (a.pts != nullptr) {
      const float* p = a.pts + srow[b] * 3;
      px[b] = p[0]; py[b] = p[1]; pz[b] = p[2];
    } else {
      const int64_t t = srow[b] / a.R, ray = srow[b] - t * a.R;
      const float* ry = a.rays + ray * 6;
      const float tt = a.ts[t];
      px[b] = ry[0] + tt * ry[3]; py[b] = ry[1] + tt * ry[4]; pz[b] = ry[2] + tt * ry[5];
    }
  }

  // ---- encode: init | layers.0 (skip) 1 2 | layers.3 (skip) 4 | out
  f32x16 enc[NTE][NB];
  {
    f32x16 acc[4][NB];
    Frag x[8][NB];
    bias_init<4, NB>(acc, B(0), h);
    fourier_pos_part<false, 4, NB>(acc, W(0), 17, 0, a.basis, px, py, pz, lane);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const int l = 1 + 3 * half;
      to_frags<true, 8>(acc, x);
      bias_init<4, NB>(acc, B(l), h);
      rows_part<8>(acc, W(l), 25, 0, x, lane);
      fourier_pos_part<true, 4, NB>(acc, W(l), 25, 8, a.basis, px, py, pz, lane);
#pragma unroll 1
      for (int i = 1; i < (half == 0 ? 3 : 2); ++i) {
        to_frags<true, 8>(acc, x);
        bias_init<4, NB>(acc, B(l + i), h);
        rows_part<8>(acc, W(l + i), 8, 0, x, lane);
      }
    }
    to_frags<true, 8>(acc, x);
    bias_init<NTE, NB>(enc, B(6), h);
    rows_part<8>(enc, W(6), 8, 0, x, lane);
  }

  // ---- F.normalize over the E columns (rows >= E of the last tile are zero: zero weights and bias); the halves of a sample's rows
  // sit on lanes n and n + 32
  if (a.normalize) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float ss = 0.f;
#pragma unroll
      for (int t = 0; t < NTE; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ss = fmaf(enc[t][b][r], enc[t][b][r], ss);
      ss += __shfl_xor(ss, 32);
      const float nrm = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
      for (int t = 0; t < NTE; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) enc[t][b][r] = enc[t][b][r] / nrm;
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (!ok[b]) continue;
    float* yrow = a.y + srow[b] * a.y_ld + 1;
#pragma unroll
    for (int t = 0; t < NTE; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = 32 * t + 8 * g + 4 * h;
        if (row < E) *(f32x4u*)(yrow + row) = f32x4u{enc[t][b][4 * g], enc[t][b][4 * g + 1], enc[t][b][4 * g + 2], enc[t][b][4 * g + 3]};
      }
  }

  // ---- density_tform: init | layers.0 (skip) 1 2 | layers.3 (skip) 4 | out
  f32x16 out[NTO][NB];
  {
    f32x16 acc[2][NB];
    Frag x[4][NB], xe[NCE][NB];
    to_frags<false, NCE>(enc, xe);
    bias_init<2, NB>(acc, B(7), h);
    rows_part<NCE>(acc, W(7), NCE, 0, xe, lane);
    to_frags<true, NCE>(enc, xe);  // the skip layers take the encoding through the activation
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
      const int l = 8 + 3 * half;
      to_frags<true, 4>(acc, x);
      bias_init<2, NB>(acc, B(l), h);
      rows_part<4>(acc, W(l), 4 + NCE, 0, x, lane);
      rows_part<NCE>(acc, W(l), 4 + NCE, 4, xe, lane);
#pragma unroll 1
      for (int i = 1; i < (half == 0 ? 3 : 2); ++i) {
        to_frags<true, 4>(acc, x);
        bias_init<2, NB>(acc, B(l + i), h);
        rows_part<4>(acc, W(l + i), 4, 0, x, lane);
      }
    }
    to_frags<true, 4>(acc, x);
    bias_init<NTO, NB>(out, B(13), h);
    rows_part<4>(out, W(13), 4, 0, x, lane);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    if (!ok[b]) continue;
    float* yrow = a.y + srow[b] * a.y_ld;
#pragma unroll
    for (int t = 0; t < NTO; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (row < 1 + I) yrow[row == 0 ? 0 : E + row] = out[t][b][r];  // the density logit | first_out[1:] behind the encoding
      }
  }
}

template <int E, int I>
int launch(const Args& a, hipStream_t stream) {
  const int64_t waves = (a.N + 32 * AE_NB - 1) / (32 * AE_NB), gx = (waves + 3) / 4;
  NA_REQUIRE(gx < (1ll << 31), NA_EINVAL, "na_ae_front: T * R too large");
  hipLaunchKernelGGL((ae_front_kernel<E, I, AE_NB>), dim3((unsigned)gx), dim3(256), 0, stream, a);
  return check_launch("na_ae_front");
}

// ---- row operators: one thread per row (W <= 64 floats)
__global__ __launch_bounds__(256) void row_normalize_kernel(const float* __restrict__ x, int64_t x_ld, int64_t N, int W,
                                                            float* __restrict__ y, int64_t y_ld) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const float* xr = x + i * x_ld;
    float ss = 0.f;
    for (int k = 0; k < W; ++k) ss = fmaf(xr[k], xr[k], ss);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);
    float* yr = y + i * y_ld;
    for (int k = 0; k < W; ++k) yr[k] = xr[k] / nrm;
  }
}

// y = x / m, m = max(|x|, eps):  g_x = (g - y <y, g>) / m where the norm is live, g / eps where it is clamped
__global__ __launch_bounds__(256) void row_normalize_backward_kernel(const float* __restrict__ x, int64_t x_ld,
                                                                     const float* __restrict__ g, int64_t g_ld, int64_t N, int W,
                                                                     float* __restrict__ gx, int64_t gx_ld) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const float* xr = x + i * x_ld;
    const float* gr = g + i * g_ld;
    float ss = 0.f, dot = 0.f;
    for (int k = 0; k < W; ++k) { ss = fmaf(xr[k], xr[k], ss); dot = fmaf(xr[k], gr[k], dot); }
    const float nrm = sqrtf(ss);
    float* o = gx + i * gx_ld;
    if (nrm > 1e-12f) {
      const float c = dot / (nrm * nrm);  // <y, g> / m = <x, g> / m^2
      for (int k = 0; k < W; ++k) o[k] = (gr[k] - xr[k] * c) / nrm;
    } else {
      for (int k = 0; k < W; ++k) o[k] = gr[k] / 1e-12f;
    }
  }
}

__global__ __launch_bounds__(256) void row_sqnorm_mean_kernel(const float* __restrict__ x, int64_t x_ld, int64_t N, int W, float inv_n,
                                                              float* __restrict__ out, long long* __restrict__ fix) {
  __shared__ float part[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    const float* xr = x + i * x_ld;
    float ss = 0.f;
    for (int k = 0; k < W; ++k) ss = fmaf(xr[k], xr[k], ss);
    acc += ss;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) accumulate(out, fix, 0, ((part[0] + part[1]) + (part[2] + part[3])) * inv_n);
}

__global__ __launch_bounds__(256) void row_sqnorm_mean_backward_kernel(const float* __restrict__ x, int64_t x_ld,
                                                                       const float* __restrict__ g, int64_t N, int W, float inv_n,
                                                                       float* __restrict__ gx, int64_t gx_ld) {
  const float c = g[0] * 2.f * inv_n;
  const int64_t total = N * W;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / W;
    const int k = (int)(i - r * W);
    gx[r * gx_ld + k] = c * x[r * x_ld + k];
  }
}

inline bool prec_ok(int precision) { return precision == NA_PREC_BF16 || precision == NA_PREC_BF16X3 || precision == NA_PREC_F16X; }

}  // namespace ae
}  // namespace na

extern "C" size_t na_ae_front_packed_bytes(int precision, int E, int I) {
  using namespace na;
  if (!ae::prec_ok(precision) || !ae::supported(E, I)) return 0;
  return ae::make_plan(E, I).bytes;
}

extern "C" int na_ae_front_pack(int precision, int E, int I, const float* const* w_enc, const float* const* b_enc,
                                const float* const* w_den, const float* const* b_den, void* packed, void* stream) {
  using namespace na;
  NA_REQUIRE(w_enc && b_enc && w_den && b_den && packed, NA_ENULL, "na_ae_front_pack: null pointer");
  NA_REQUIRE(ae::prec_ok(precision), NA_EUNSUPPORTED, "na_ae_front_pack: precision %d", precision);
  NA_REQUIRE(ae::supported(E, I), NA_EUNSUPPORTED, "na_ae_front_pack: E=%d I=%d (E in 16 | 32 | 64, I in 32 | 64)", E, I);
  NA_REQUIRE(((uintptr_t)packed & 15) == 0, NA_EINVAL, "na_ae_front_pack: packed must be 16-byte aligned");
  const ae::Plan p = ae::make_plan(E, I);
  for (int i = 0; i < ae::kLayers; ++i) {
    const float* w = i < 7 ? w_enc[i] : w_den[i - 7];
    const float* b = i < 7 ? b_enc[i] : b_den[i - 7];
    NA_REQUIRE(w, NA_ENULL, "na_ae_front_pack: weights[%d] is null", i);
    const int total = p.l[i].tiles * p.l[i].chunks * 64;
    hipLaunchKernelGGL(ae::pack_layer_kernel, dim3(grid_for(total, 256, 1024)), dim3(256), 0, (hipStream_t)stream, w, b, p.l[i],
                       (char*)packed);
  }
  return check_launch("na_ae_front_pack");
}

extern "C" int na_ae_front(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* basis,
                           const void* packed, int precision, int E, int I, int normalize, float* y, int64_t y_ld, void* stream) {
  using namespace na;
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_ae_front: bad shape T=%d R=%lld", T, (long long)R);
  if (R == 0) return NA_OK;
  NA_REQUIRE((rays || pts) && (pts || ts) && basis && packed && y, NA_ENULL, "na_ae_front: null pointer");
  NA_REQUIRE(ae::prec_ok(precision), NA_EUNSUPPORTED, "na_ae_front: precision %d", precision);
  NA_REQUIRE(ae::supported(E, I), NA_EUNSUPPORTED, "na_ae_front: E=%d I=%d (E in 16 | 32 | 64, I in 32 | 64)", E, I);
  NA_REQUIRE(y_ld >= 1 + E + I, NA_EINVAL, "na_ae_front: y_ld %lld < 1 + E + I = %d", (long long)y_ld, 1 + E + I);
  NA_REQUIRE(((uintptr_t)basis & 15) == 0 && ((uintptr_t)packed & 15) == 0, NA_EINVAL, "na_ae_front: basis and packed must be 16-byte aligned");
  const ae::Plan p = ae::make_plan(E, I);
  ae::Args a;
  a.rays = rays; a.pts = pts; a.ts = ts; a.basis = basis; a.packed = (const char*)packed; a.y = y;
  a.R = R; a.N = (int64_t)T * R; a.y_ld = y_ld; a.normalize = normalize ? 1 : 0;
  for (int i = 0; i < ae::kLayers; ++i) { a.o.w[i] = p.l[i].w_off; a.o.b[i] = p.l[i].b_off; }
  hipStream_t st = (hipStream_t)stream;
  if (E == 16) return I == 32 ? ae::launch<16, 32>(a, st) : ae::launch<16, 64>(a, st);
  if (E == 32) return I == 32 ? ae::launch<32, 32>(a, st) : ae::launch<32, 64>(a, st);
  return I == 32 ? ae::launch<64, 32>(a, st) : ae::launch<64, 64>(a, st);
}

extern "C" int na_row_normalize(const float* x, int64_t x_ld, int64_t N, int W, float* y, int64_t y_ld, void* stream) {
  using namespace na;
  if (N == 0) return NA_OK;
  NA_REQUIRE(x && y, NA_ENULL, "na_row_normalize: null pointer");
  NA_REQUIRE(N > 0 && W >= 1 && W <= 64 && x_ld >= W && y_ld >= W, NA_EINVAL, "na_row_normalize: bad shape N=%lld W=%d", (long long)N, W);
  hipLaunchKernelGGL(ae::row_normalize_kernel, dim3(grid_for(N, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, x_ld, N, W, y, y_ld);
  return check_launch("na_row_normalize");
}

extern "C" int na_row_normalize_backward(const float* x, int64_t x_ld, const float* g_y, int64_t g_ld, int64_t N, int W, float* g_x,
                                         int64_t gx_ld, void* stream) {
  using namespace na;
  if (N == 0) return NA_OK;
  NA_REQUIRE(x && g_y && g_x, NA_ENULL, "na_row_normalize_backward: null pointer");
  NA_REQUIRE(N > 0 && W >= 1 && W <= 64 && x_ld >= W && g_ld >= W && gx_ld >= W, NA_EINVAL,
             "na_row_normalize_backward: bad shape N=%lld W=%d", (long long)N, W);
  hipLaunchKernelGGL(ae::row_normalize_backward_kernel, dim3(grid_for(N, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, x_ld, g_y,
                     g_ld, N, W, g_x, gx_ld);
  return check_launch("na_row_normalize_backward");
}

extern "C" int na_row_sqnorm_mean(const float* x, int64_t x_ld, int64_t N, int W, float* out, void* stream) {
  using namespace na;
  NA_REQUIRE(x && out, NA_ENULL, "na_row_sqnorm_mean: null pointer");
  NA_REQUIRE(N > 0 && W >= 1 && W <= 64 && x_ld >= W, NA_EINVAL, "na_row_sqnorm_mean: bad shape N=%lld W=%d", (long long)N, W);
  int rc;
  long long* fix = det_begin(1, (hipStream_t)stream, "na_row_sqnorm_mean", &rc);
  if (rc != NA_OK) return rc;
  hipLaunchKernelGGL(ae::row_sqnorm_mean_kernel, dim3(grid_for(N, 256, 1024)), dim3(256), 0, (hipStream_t)stream, x, x_ld, N, W,
                     1.0f / (float)N, out, fix);
  if (fix != nullptr) return det_finish(fix, 1, out, (hipStream_t)stream, "na_row_sqnorm_mean");
  return check_launch("na_row_sqnorm_mean");
}

extern "C" int na_row_sqnorm_mean_backward(const float* x, int64_t x_ld, const float* g, int64_t N, int W, float* g_x, int64_t gx_ld,
                                           void* stream) {
  using namespace na;
  NA_REQUIRE(x && g && g_x, NA_ENULL, "na_row_sqnorm_mean_backward: null pointer");
  NA_REQUIRE(N > 0 && W >= 1 && W <= 64 && x_ld >= W && gx_ld >= W, NA_EINVAL, "na_row_sqnorm_mean_backward: bad shape N=%lld W=%d",
             (long long)N, W);
  hipLaunchKernelGGL(ae::row_sqnorm_mean_backward_kernel, dim3(grid_for(N * W, 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, x_ld,
                     g, N, W, 1.0f / (float)N, g_x, gx_ld);
  return check_launch("na_row_sqnorm_mean_backward");
}
