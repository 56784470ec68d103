// Spherical-harmonic colour head (src/refl.py:696-731, src/spherical_harmonics.py:55-106):
//     coeffs = mlp([elaz(view) | Fourier(elaz(view)) | latent]);   rgb = act( sum_k coeffs[c, k] Y_k(normalize(view)) )
//   na_sh_shade / na_sh_shade_backward   the expansion and its gradient w.r.t. the coefficients; the basis lives in registers
//   na_sh_view_terms                     the part of the MLP's three wide Linears that depends on the RAY only (258 of their 322 /
//                                        450 input columns): one [R, 128] bias row per ray and Linear instead of [N, 322] init rows
// All arithmetic fp32.  Rows are sample-major, n = t R + r.
#include "common.h"
#include "sh_basis.h"

namespace na {

// one thread per sample: 3 K consecutive coefficients (channel-major, column c K + k) against the basis of the sample's ray
__global__ __launch_bounds__(256) void sh_shade_kernel(const float* __restrict__ coeffs, int64_t ld, const float* __restrict__ dirs,
                                                       int64_t N, int64_t R, int order, int kind, float* __restrict__ rgb,
                                                       float* __restrict__ pre) {
  const int K = (order + 1) * (order + 1);
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = n % R;
    float Y[SH_MAX_K];
    sh_basis(order, dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], Y);
    const float* co = coeffs + n * ld;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float acc = Y[0] * co[c * K];
#pragma unroll
      for (int k = 1; k < SH_MAX_K; ++k)
        if (k < K) acc = fmaf(Y[k], co[c * K + k], acc);
      if (pre != nullptr) pre[n * 3 + c] = acc;
      rgb[n * 3 + c] = apply_sigmoid_kind(acc, kind);
    }
  }
}

// g_coeffs[n, c K + k] = g_rgb[n, c] act'(pre[n, c]) Y_k
__global__ __launch_bounds__(256) void sh_shade_backward_kernel(const float* __restrict__ g_rgb, const float* __restrict__ pre,
                                                                const float* __restrict__ dirs, int64_t N, int64_t R, int order,
                                                                int kind, float* __restrict__ g_coeffs) {
  const int K = (order + 1) * (order + 1);
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = n % R;
    float Y[SH_MAX_K];
    sh_basis(order, dirs[r * 3], dirs[r * 3 + 1], dirs[r * 3 + 2], Y);
    float* go = g_coeffs + n * 3 * K;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float g = g_rgb[n * 3 + c] * sigmoid_kind_grad(pre[n * 3 + c], kind);
#pragma unroll
      for (int k = 0; k < SH_MAX_K; ++k)
        if (k < K) go[c * K + k] = g * Y[k];
    }
  }
}

// ---- per-ray view terms.  A workgroup owns 32 consecutive rays: their features f = [elev, azim | sin | cos] (elev_azim and
// fourier_sincos of common.h, the arithmetic of na_view_elaz + na_fourier_encode) are built once in LDS, then multiplied with the
// view columns of the three Linears on the f32 matrix core (v_mfma_f32_32x32x2_f32, bitwise an fp32 fma chain in k order: a ray's
// terms do not depend on R or on the ray's place in its workgroup).  Weight chunks go through LDS like in linear_f32.hip; the
// 3 x 128 x 258 weights (396 KB) stay in L2 across workgroups.
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int VT_RAYS = 32;                     // rays per workgroup
constexpr int VT_MAXF = 128, VT_MAXH = 128;     // encoder frequencies / hidden width the LDS tiles are sized for
constexpr int VT_BK = 16;                       // K chunk
constexpr int VT_KPAD = ((2 + 2 * VT_MAXF + VT_BK - 1) / VT_BK) * VT_BK;  // 272
constexpr int VT_FLD = VT_KPAD + 1;             // 273: odd pitch, the 32 rays of an MFMA operand hit 32 banks
constexpr int VT_WLD = VT_BK + 1;
constexpr int VT_TILES = 3 * VT_MAXH / 32;      // 12 column tiles of 32, 3 per wave

__global__ __launch_bounds__(256) void sh_view_terms_kernel(const float* __restrict__ dirs, int64_t R, const float* __restrict__ basis,
                                                            int F, float scale, const float* __restrict__ w_init, int64_t ld_init,
                                                            const float* __restrict__ b_init, const float* __restrict__ w_a,
                                                            const float* __restrict__ b_a, const float* __restrict__ w_b,
                                                            const float* __restrict__ b_b, int64_t ld_skip, int H,
                                                            float* __restrict__ terms) {
  __shared__ float Fs[VT_RAYS * VT_FLD];
  __shared__ float Ws[3 * VT_MAXH * VT_WLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * VT_RAYS;
  const int K = 2 + 2 * F;
  for (int i = tid; i < VT_RAYS * VT_FLD; i += 256) Fs[i] = 0.f;
  __syncthreads();
  if (tid < VT_RAYS && r0 + tid < R) {
    const float* d = dirs + (r0 + tid) * 3;
    float e, a;
    elev_azim(d[0], d[1], d[2], e, a);
    Fs[tid * VT_FLD] = e;
    Fs[tid * VT_FLD + 1] = a;
  }
  __syncthreads();
  for (int i = tid; i < VT_RAYS * F; i += 256) {
    const int ray = i / F, j = i - ray * F;
    if (r0 + ray >= R) continue;
    // (na_fourier_encode's argument for D = 2: x0 * b0, then one fma)
    const float b0 = scale == 1.0f ? basis[j] : scale * basis[j];
    const float b1 = scale == 1.0f ? basis[F + j] : scale * basis[F + j];
    float m = Fs[ray * VT_FLD] * b0;
    m = fmaf(Fs[ray * VT_FLD + 1], b1, m);
    float sn, cs;
    fourier_sincos(m, sn, cs);
    Fs[ray * VT_FLD + 2 + j] = sn;
    Fs[ray * VT_FLD + 2 + F + j] = cs;
  }
  __syncthreads();

  const int ncol = 3 * H, ntile = ncol / 32;
  f32x16 acc[VT_TILES / 4];
#pragma unroll
  for (int t = 0; t < VT_TILES / 4; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  for (int k0 = 0; k0 < K; k0 += VT_BK) {
    for (int i = tid; i < ncol * VT_BK; i += 256) {
      const int col = i / VT_BK, kk = i - col * VT_BK, k = k0 + kk;
      const int mat = col / H, h = col - mat * H;
      float wv = 0.f;
      if (k < K) wv = mat == 0 ? w_init[h * ld_init + k] : (mat == 1 ? w_a : w_b)[h * ld_skip + k];
      Ws[col * VT_WLD + kk] = wv;
    }
    __syncthreads();
    const float* xa = Fs + (lane & 31) * VT_FLD + k0 + (lane >> 5);
#pragma unroll
    for (int t = 0; t < VT_TILES / 4; ++t) {
      const int tile = wave + 4 * t;
      if (tile < ntile) {
        const bool activated = tile * 32 >= H;  // (H is a multiple of 32: a tile lies inside one Linear)
        const float* wb = Ws + (tile * 32 + (lane & 31)) * VT_WLD + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < VT_BK; kk += 2) {
          const float xv = activated ? leaky_relu(xa[kk]) : xa[kk];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wb[kk], acc[t], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < VT_TILES / 4; ++t) {
    const int tile = wave + 4 * t;
    if (tile >= ntile) continue;
    const int col = tile * 32 + (lane & 31);
    const int mat = col / H, h = col - mat * H;
    const float bj = (mat == 0 ? b_init : (mat == 1 ? b_a : b_b))[h];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t ray = r0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (ray < R) terms[((int64_t)mat * R + ray) * H + h] = acc[t][r] + bj;
    }
  }
}

}  // namespace na

extern "C" int na_sh_shade(const float* coeffs, int64_t ld, const float* dirs, int64_t N, int64_t R, int order, int kind,
                           float* rgb, float* pre, void* stream) {
  using namespace na;
  NA_REQUIRE(coeffs && dirs && rgb, NA_ENULL, "na_sh_shade: null pointer");
  NA_REQUIRE(order >= 0 && order <= 4, NA_EINVAL, "na_sh_shade: order %d outside 0..4", order);
  NA_REQUIRE(N >= 0 && R >= 1 && N % R == 0 && ld >= 3 * (order + 1) * (order + 1), NA_EINVAL,
             "na_sh_shade: bad shape N=%lld R=%lld ld=%lld", (long long)N, (long long)R, (long long)ld);
  NA_REQUIRE(kind >= 0 && kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "na_sh_shade: kind %d", kind);
  if (N == 0) return NA_OK;
  hipLaunchKernelGGL(sh_shade_kernel, dim3(grid_for(N, 256, 16384)), dim3(256), 0, (hipStream_t)stream, coeffs, ld, dirs, N, R,
                     order, kind, rgb, pre);
  return check_launch("na_sh_shade");
}

extern "C" int na_sh_shade_backward(const float* g_rgb, const float* pre, const float* dirs, int64_t N, int64_t R, int order,
                                    int kind, float* g_coeffs, void* stream) {
  using namespace na;
  NA_REQUIRE(g_rgb && pre && dirs && g_coeffs, NA_ENULL, "na_sh_shade_backward: null pointer");
  NA_REQUIRE(order >= 0 && order <= 4, NA_EINVAL, "na_sh_shade_backward: order %d outside 0..4", order);
  NA_REQUIRE(N >= 0 && R >= 1 && N % R == 0, NA_EINVAL, "na_sh_shade_backward: bad shape N=%lld R=%lld", (long long)N, (long long)R);
  NA_REQUIRE(kind >= 0 && kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "na_sh_shade_backward: kind %d", kind);
  if (N == 0) return NA_OK;
  hipLaunchKernelGGL(sh_shade_backward_kernel, dim3(grid_for(N, 256, 16384)), dim3(256), 0, (hipStream_t)stream, g_rgb, pre, dirs,
                     N, R, order, kind, g_coeffs);
  return check_launch("na_sh_shade_backward");
}

extern "C" int na_sh_view_terms(const float* dirs, int64_t R, const float* basis, int F, float scale, const float* w_init,
                                int64_t ld_init, const float* b_init, const float* w_a, const float* b_a, const float* w_b,
                                const float* b_b, int64_t ld_skip, int hidden, float* terms, void* stream) {
  using namespace na;
  NA_REQUIRE(dirs && basis && w_init && b_init && w_a && b_a && w_b && b_b && terms, NA_ENULL, "na_sh_view_terms: null pointer");
  NA_REQUIRE(R >= 0 && F >= 1 && hidden >= 1 && ld_init >= 2 + 2 * F && ld_skip >= 2 + 2 * F, NA_EINVAL,
             "na_sh_view_terms: bad shape R=%lld F=%d hidden=%d", (long long)R, F, hidden);
  NA_REQUIRE(F <= VT_MAXF && hidden <= VT_MAXH && hidden % 32 == 0, NA_EUNSUPPORTED,
             "na_sh_view_terms: F=%d hidden=%d (the kernel holds F <= 128 and a hidden width of 32, 64, 96 or 128)", F, hidden);
  if (R == 0) return NA_OK;
  const int64_t gx = (R + VT_RAYS - 1) / VT_RAYS;
  NA_REQUIRE(gx < (1ll << 31), NA_EINVAL, "na_sh_view_terms: R too large");
  hipLaunchKernelGGL(sh_view_terms_kernel, dim3((unsigned)gx), dim3(256), 0, (hipStream_t)stream, dirs, R, basis, F, scale, w_init,
                     ld_init, b_init, w_a, b_a, w_b, b_b, ld_skip, hidden, terms);
  return check_launch("na_sh_view_terms");
}
