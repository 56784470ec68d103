// The Fourier encoder as a training node (src/utils.py:14-17 under autograd): the init rows [p | sin(pB) | cos(pB) | latent] of a
// Fourier-encoded SkipConnMLP written by ONE launch (the counterpart of na_hash_encode_rows), and the gradient of the features
// with respect to the POSITIONS -- what a deformation field in front of a Fourier-encoded canonical model needs (D-NeRF over
// VolSDF's MLP SDF network, reference makefile:127-133).  The argument m = x . be and its sine / cosine are the forward's, operation
// for operation (fourier_kernel of basic_ops.hip, fourier_sincos of common.h), so the rows are bit-identical to
// cat([x, na_fourier_encode(x), latent]) and the backward differentiates exactly the features the forward produced.
#include "common.h"

namespace na {

constexpr int kFgMaxD = 8;  // (mlp_layout.h's bound on the raw input width of a Fourier-encoded network: in_size <= 8)

__device__ __forceinline__ float fg_basis(const float* __restrict__ basis, int F, int d, int j, float scale) {
  const float b = basis[d * F + j];
  return scale == 1.0f ? b : scale * b;
}

// rows[n] = [x[n, 0:D] | sin(m) | cos(m) | latent[n, 0:L]], m_j = x[n] . be[:, j].  One thread per (sample, item): items 0..F-1 are the
// frequencies (one sincos, two stores), the D + L items behind them copy the raw input and the latent.  Consecutive lanes write
// consecutive floats of a row; the rows' pitch D + 2F + L (259 for VolSDF's network) has no 16-byte alignment to offer.
__global__ void fourier_rows_kernel(const float* __restrict__ x, int64_t N, int D, const float* __restrict__ basis, int F, float scale,
                                    const float* __restrict__ latent, int L, int64_t lat_ld, float* __restrict__ rows) {
  const int items = F + D + L;
  const int W = D + 2 * F + L;
  const int64_t total = N * items;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int j = (int)(i % items);
    const int64_t n = i / items;
    float* row = rows + n * W;
    if (j < F) {
      float m = 0.f;
      for (int d = 0; d < D; ++d) {
        const float be = fg_basis(basis, F, d, j, scale);
        m = d == 0 ? x[n * D + d] * be : fmaf(x[n * D + d], be, m);
      }
      float sn, cs;
      fourier_sincos(m, sn, cs);
      __builtin_nontemporal_store(sn, row + D + j);
      __builtin_nontemporal_store(cs, row + D + F + j);
    } else if (j < F + D) {
      __builtin_nontemporal_store(x[n * D + (j - F)], row + (j - F));
    } else {
      __builtin_nontemporal_store(latent[n * lat_ld + (j - F - D)], row + D + 2 * F + (j - F - D));
    }
  }
}

// gx[n, d] = (lead ? g[n, d] : 0) + sum_f be[d, f] (cos(m_f) g_sin[n, f] - sin(m_f) g_cos[n, f]).
// A half-wave (32 lanes) owns one sample.  VEC (F a multiple of 4): a lane takes 4 consecutive frequencies per step -- one 16-byte load
// each of g_sin, g_cos and the basis rows; F = 128: one step, a 512-byte line per half-wave and operand.  The loads are declared
// 4-byte aligned: the init rows' gradient has pitch D + 2F + L (259) and its feature columns start at D, so a row starts on no
// 16-byte boundary, and gfx950 serves a 16-byte access at dword alignment (tools/hw/unaligned_probe.hip; the training GEMMs store
// their unaligned rows the same way).  One form for every pitch also means ONE summation order: the rows' backward and the
// standalone encoder's give the same bits.  Any other F: the lanes stride over the frequencies one float at a time.  Each lane keeps
// D partial sums, the 32 lanes add them with a fixed xor tree, lane 0 stores: no atomics, no LDS, the same bits every run.
// SAVED: sin / cos are read back from the forward's rows (`saved`, pitch s_ld, the sine columns at s_col0) instead of recomputed --
// the measured alternative (tools/fourier_grad_bench.py), twice the bytes.
typedef float fg_f32x4 __attribute__((ext_vector_type(4), aligned(4)));

template <bool VEC, bool SAVED>
__global__ void fourier_bwd_input_kernel(const float* __restrict__ x, int64_t N, int D, const float* __restrict__ basis, int F, float scale,
                                         const float* __restrict__ g, int64_t g_ld, int col0, int lead,
                                         const float* __restrict__ saved, int64_t s_ld, int s_col0, float* __restrict__ gx) {
  const int lane = threadIdx.x & 31;
  const int64_t half0 = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 5;
  const int64_t nhalf = ((int64_t)gridDim.x * blockDim.x) >> 5;
  for (int64_t n = half0; n < N; n += nhalf) {
    float xv[kFgMaxD], acc[kFgMaxD];
#pragma unroll
    for (int d = 0; d < kFgMaxD; ++d) {
      xv[d] = d < D ? x[n * D + d] : 0.f;
      acc[d] = 0.f;
    }
    const float* gs = g + n * g_ld + col0;
    const float* gc = gs + F;
    const float* ss = SAVED ? saved + n * s_ld + s_col0 : nullptr;
    if constexpr (VEC) {
      for (int j = 4 * lane; j < F; j += 128) {
        const fg_f32x4 a4 = *(const fg_f32x4*)(gs + j), c4 = *(const fg_f32x4*)(gc + j);
        const float a[4] = {a4.x, a4.y, a4.z, a4.w}, c[4] = {c4.x, c4.y, c4.z, c4.w};
        float be[kFgMaxD][4], m[4];
#pragma unroll
        for (int d = 0; d < kFgMaxD; ++d) {
          if (d < D) {
            const fg_f32x4 bv = *(const fg_f32x4*)(basis + d * F + j);
            const float b[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              be[d][e] = scale == 1.0f ? b[e] : scale * b[e];
              m[e] = d == 0 ? xv[d] * be[d][e] : fmaf(xv[d], be[d][e], m[e]);
            }
          }
        }
        float sn[4], cs[4];
        if constexpr (SAVED) {
          const fg_f32x4 s4 = *(const fg_f32x4*)(ss + j), k4 = *(const fg_f32x4*)(ss + F + j);
          sn[0] = s4.x; sn[1] = s4.y; sn[2] = s4.z; sn[3] = s4.w;
          cs[0] = k4.x; cs[1] = k4.y; cs[2] = k4.z; cs[3] = k4.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) fourier_sincos(m[e], sn[e], cs[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = fmaf(cs[e], a[e], -(sn[e] * c[e]));
#pragma unroll
          for (int d = 0; d < kFgMaxD; ++d)
            if (d < D) acc[d] = fmaf(be[d][e], t, acc[d]);
        }
      }
    } else {
      for (int j = lane; j < F; j += 32) {
        float be[kFgMaxD], m = 0.f;
#pragma unroll
        for (int d = 0; d < kFgMaxD; ++d) {
          if (d < D) {
            be[d] = fg_basis(basis, F, d, j, scale);
            m = d == 0 ? xv[d] * be[d] : fmaf(xv[d], be[d], m);
          }
        }
        float sn, cs;
        if constexpr (SAVED) { sn = ss[j]; cs = ss[F + j]; }
        else fourier_sincos(m, sn, cs);
        const float t = fmaf(cs, gs[j], -(sn * gc[j]));
#pragma unroll
        for (int d = 0; d < kFgMaxD; ++d)
          if (d < D) acc[d] = fmaf(be[d], t, acc[d]);
      }
    }
    // (xor distances below 32 never leave the half-wave: a half whose loop has ended is not read)
#pragma unroll
    for (int d = 0; d < kFgMaxD; ++d) {
      if (d < D) {
#pragma unroll
        for (int s = 16; s >= 1; s >>= 1) acc[d] += __shfl_xor(acc[d], s);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < kFgMaxD; ++d)
        if (d < D) gx[n * D + d] = lead ? g[n * g_ld + d] + acc[d] : acc[d];
    }
  }
}

static int fourier_bwd_launch(const char* who, const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* g,
                              int g_ld, int col0, int lead, const float* saved, int s_ld, int s_col0, float* gx, void* stream) {
  NA_REQUIRE(N >= 0 && D >= 1 && D <= kFgMaxD && F >= 1, NA_EINVAL, "%s: bad shape (N=%lld D=%d (1..%d) F=%d)", who, (long long)N, D,
             kFgMaxD, F);
  NA_REQUIRE((lead == 0 || lead == 1) && col0 >= lead * D && g_ld >= col0 + 2 * F, NA_EINVAL,
             "%s: the 2F = %d feature columns at %d (lead = %d, D = %d) do not fit rows of pitch %d", who, 2 * F, col0, lead, D, g_ld);
  NA_REQUIRE(saved == nullptr || (s_col0 >= 0 && s_ld >= s_col0 + 2 * F), NA_EINVAL, "%s: the saved rows (pitch %d) do not hold 2F columns at %d",
             who, s_ld, s_col0);
  if (N == 0) return NA_OK;  // empty: zero-size tensors carry null pointers
  NA_REQUIRE(x && basis && g && gx, NA_ENULL, "%s: null pointer", who);
  const bool vec = (F & 3) == 0;
  const dim3 grid(grid_for(N * 32, 256, 1 << 20)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (saved == nullptr) {
    if (vec) hipLaunchKernelGGL((fourier_bwd_input_kernel<true, false>), grid, block, 0, st, x, N, D, basis, F, scale, g, (int64_t)g_ld, col0, lead, saved, (int64_t)s_ld, s_col0, gx);
    else hipLaunchKernelGGL((fourier_bwd_input_kernel<false, false>), grid, block, 0, st, x, N, D, basis, F, scale, g, (int64_t)g_ld, col0, lead, saved, (int64_t)s_ld, s_col0, gx);
  } else {
    if (vec) hipLaunchKernelGGL((fourier_bwd_input_kernel<true, true>), grid, block, 0, st, x, N, D, basis, F, scale, g, (int64_t)g_ld, col0, lead, saved, (int64_t)s_ld, s_col0, gx);
    else hipLaunchKernelGGL((fourier_bwd_input_kernel<false, true>), grid, block, 0, st, x, N, D, basis, F, scale, g, (int64_t)g_ld, col0, lead, saved, (int64_t)s_ld, s_col0, gx);
  }
  return check_launch(who);
}

}  // namespace na

using namespace na;

extern "C" int na_fourier_rows(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* latent, int L, int64_t lat_ld,
                    float* rows, void* stream) {
  NA_REQUIRE(N >= 0 && D >= 1 && D <= kFgMaxD && F >= 1 && L >= 0, NA_EINVAL, "na_fourier_rows: bad shape (N=%lld D=%d (1..%d) F=%d L=%d)",
             (long long)N, D, kFgMaxD, F, L);
  NA_REQUIRE(L == 0 || lat_ld >= L, NA_EINVAL, "na_fourier_rows: latent pitch %lld < L = %d", (long long)lat_ld, L);
  if (N == 0) return NA_OK;  // empty: zero-size tensors carry null pointers
  NA_REQUIRE(x && basis && rows && (L == 0 || latent), NA_ENULL, "na_fourier_rows: null pointer");
  hipLaunchKernelGGL(fourier_rows_kernel, dim3(grid_for(N * (F + D + L), 256, 16384)), dim3(256), 0, (hipStream_t)stream, x, N, D, basis, F,
                     scale, latent, L, lat_ld, rows);
  return check_launch("na_fourier_rows");
}

extern "C" int na_fourier_encode_backward_input(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* g, int g_ld,
                                     int col0, int lead, float* gx, void* stream) {
  return fourier_bwd_launch("na_fourier_encode_backward_input", x, N, D, basis, F, scale, g, g_ld, col0, lead, nullptr, 0, 0, gx, stream);
}

extern "C" int na_fourier_encode_backward_input_saved(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* g, int g_ld,
                                           int col0, int lead, const float* saved, int s_ld, int s_col0, float* gx, void* stream) {
  NA_REQUIRE(saved != nullptr || N == 0, NA_ENULL, "na_fourier_encode_backward_input_saved: null pointer");
  return fourier_bwd_launch("na_fourier_encode_backward_input_saved", x, N, D, basis, F, scale, g, g_ld, col0, lead, saved, s_ld, s_col0, gx,
                            stream);
}
