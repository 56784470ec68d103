// SSIM and the pieces of MS-SSIM (Wang et al.; the choices of pytorch_msssim, which the reference calls: src/utils.py:186-195;
// DESIGN.md 3r).  Images are fp32, channel-last [N,H,W,C], C = 1 .. 4, read in place: a workgroup walks the channels of its tile.
//   na_ssim            per (n, c) the mean over the (H-10) x (W-10) "valid" map of  ssim = l cs  and of  cs:
//                        mu1 = G*x, mu2 = G*y, s1 = G*(x x) - mu1^2, s2 = G*(y y) - mu2^2, s12 = G*(x y) - mu1 mu2,
//                        cs = (2 s12 + C2) / (s1 + s2 + C2),  l = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1)
//                      G the separable 11-tap Gaussian (sigma 1.5) below.
//   na_ssim_backward   g_x = (g[n,c] / count) (G^T[dm] + 2 x G^T[dS/ds1] + y G^T[dS/ds12]), one thread per output pixel, no atomics.
//   na_image_halve     F.avg_pool2d(kernel 2, padding (H % 2, W % 2), count_include_pad=True) of both images in one launch.
//
// THE VARIANCES ARE FORMED CENTRED.  s1 = G*(x x) - mu1^2 as written cancels: in a smooth region both terms are ~0.3 and their
// difference ~1e-3, divided by a denominator of the same size -- 24 u 0.3 / 1e-3 = 4e-4 per pixel, more than the difference between
// a right and a wrong window (tests/ssim_ref.py, the discrimination condition).  So a thread forms the means of ITS pixel first
// (separable: rows in LDS, then the column) and then sums the 121 products of the window about them,
//     c11 = sum_a g_a sum_b g_b (x_ab - mu1)^2,   c22, c12 alike,
// rows first, in tap order.  All addends of c11 / c22 are >= 0, so their error is RELATIVE (26 u c11), and |c12| <= sqrt(c11 c22).
// The taps are the fp32 roundings of the normalised Gaussian: the 121 products g_a g_b sum to 1 - kTapDefect, not to 1; the definition
// above uses the same table, so  s1 = c11 + kTapDefect mu1^2,  s12 = c12 + kTapDefect mu1 mu2  exactly, and the kernel adds that term.
// 363 multiply-adds per pixel instead of 110: the window is in LDS either way, and nothing but two partial sums per tile and
// channel leaves the CU.
//
// ORDER OF THE SUMS (the result is bit-identical from run to run in every mode; no atomics anywhere): a tile is 16 x 16 pixels of
// the valid map, one per thread (a pixel outside the map adds 0); wave_total_lane63 adds the 64 threads of a wave, thread 255 the
// four waves in wave order, and writes partial[n][c][tile][2] to the caller's workspace.  ssim_finish_kernel (one wave per (n, c))
// adds the tiles in double: lane l takes tiles l, l + 64, ... in order, lane 0 then adds the 64 lanes in lane order, divides by
// the count and rounds once.
// This unit is built with -ffp-contract=off: every product and sum below is rounded on its own, as tests/ssim_ref.py counts them.
#include "common.h"

namespace na {

constexpr int kTaps = 11;
constexpr int kHalo = kTaps - 1;
constexpr int kTile = 16;                    // output pixels per tile side (256 threads)
constexpr int kFwdIn = kTile + kHalo;        // 26: input rows / columns of a forward tile
constexpr int kFwdStride = 48;               // 16 mod 32: the two rows a 32-lane group reads sit on disjoint banks
constexpr int kBwdMap = kTile + kHalo;       // 26: pixels of the valid map under the transposed window of a backward tile
constexpr int kBwdIn = kBwdMap + kHalo;      // 36: input rows / columns behind them
constexpr int kBwdStride = 37;
constexpr int kBwdMapStride = 27;
constexpr int kSsimMaxSide = 32768;

// exp(-(i - 5)^2 / (2 1.5^2)) / sum, formed in double and rounded once
__device__ static const float kG[kTaps] = {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                                           0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
constexpr float kTapDefect = 2.7939677218948716e-09f;  // 1 - (the sum of the eleven fp32 taps)^2, exact arithmetic: the 121 products' sum

struct SsimPixel { float mu1, mu2, mu12, s12, A1, B1, N2, B2, cs, S; };

// the pixel whose window starts at (r, q) of the LDS tile (tx, ty: row stride STRIDE); mu1 / mu2: its means
template <int STRIDE>
__device__ __forceinline__ SsimPixel ssim_pixel(const float* tx, const float* ty, int r, int q, float mu1, float mu2, float C1, float C2) {
  float c11 = 0.f, c22 = 0.f, c12 = 0.f;
#pragma unroll 1
  for (int a = 0; a < kTaps; ++a) {
    const float* px = tx + (r + a) * STRIDE + q;
    const float* py = ty + (r + a) * STRIDE + q;
    float r11 = 0.f, r22 = 0.f, r12 = 0.f;
#pragma unroll
    for (int b = 0; b < kTaps; ++b) {
      const float dx = px[b] - mu1, dy = py[b] - mu2;
      r11 = r11 + kG[b] * (dx * dx);
      r22 = r22 + kG[b] * (dy * dy);
      r12 = r12 + kG[b] * (dx * dy);
    }
    c11 = c11 + kG[a] * r11;
    c22 = c22 + kG[a] * r22;
    c12 = c12 + kG[a] * r12;
  }
  SsimPixel p;
  p.mu1 = mu1;
  p.mu2 = mu2;
  const float mu1sq = mu1 * mu1, mu2sq = mu2 * mu2;
  p.mu12 = mu1 * mu2;
  const float s1 = c11 + kTapDefect * mu1sq, s2 = c22 + kTapDefect * mu2sq;
  p.s12 = c12 + kTapDefect * p.mu12;
  p.N2 = 2.f * p.s12 + C2;
  p.B2 = (s1 + s2) + C2;
  p.cs = p.N2 / p.B2;
  p.A1 = 2.f * p.mu12 + C1;
  p.B1 = (mu1sq + mu2sq) + C1;
  p.S = (p.A1 / p.B1) * p.cs;
  return p;
}

// dst[r * DS + q] = sum_k g_k src[r * SS + q + k], r < rows, q < cols (the caller's barrier follows)
template <int SS, int DS>
__device__ __forceinline__ void filter_rows(const float* src, float* dst, int rows, int cols) {
  for (int idx = threadIdx.x; idx < rows * cols; idx += 256) {
    const int r = idx / cols, q = idx - r * cols;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) acc = acc + kG[k] * src[r * SS + q + k];
    dst[r * DS + q] = acc;
  }
}

// sum_k g_k src[(r + k) * SS + q]
template <int SS>
__device__ __forceinline__ float filter_col(const float* src, int r, int q) {
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < kTaps; ++k) acc = acc + kG[k] * src[(r + k) * SS + q];
  return acc;
}

// rows x rows pixels from image row r0 / column c0 of channel c of image n into tx / ty (0 outside the image: r0, c0 may be negative)
template <int SIDE, int STRIDE>
__device__ __forceinline__ void load_tile(const float* __restrict__ x, const float* __restrict__ y, int64_t n, int H, int W, int C, int c, int r0,
                                          int c0, float* tx, float* ty) {
  for (int idx = threadIdx.x; idx < SIDE * SIDE; idx += 256) {
    const int r = idx / SIDE, q = idx - r * SIDE;
    const int gr = r0 + r, gc = c0 + q;
    const bool in = gr >= 0 && gr < H && gc >= 0 && gc < W;
    const int64_t at = ((n * H + (in ? gr : 0)) * W + (in ? gc : 0)) * C + c;
    const float xv = x[at], yv = y[at];  // (always an address inside the image)
    tx[r * STRIDE + q] = in ? xv : 0.f;
    ty[r * STRIDE + q] = in ? yv : 0.f;
  }
}

// grid: N * tiles workgroups of 256; partial [N][C][tiles][2]
__global__ __launch_bounds__(256) void ssim_tiles_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int C,
                                                         int tiles_x, int tiles, float C1, float C2, float* __restrict__ partial) {
  __shared__ float tx[kFwdIn * kFwdStride], ty[kFwdIn * kFwdStride], hx[kFwdIn * kTile], hy[kFwdIn * kTile], part[8];
  const int64_t n = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)(n * tiles);
  const int r0 = (tile / tiles_x) * kTile, c0 = (tile % tiles_x) * kTile;
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  const bool valid = r0 + i < H - kHalo && c0 + j < W - kHalo;
  for (int c = 0; c < C; ++c) {
    load_tile<kFwdIn, kFwdStride>(x, y, n, H, W, C, c, r0, c0, tx, ty);
    __syncthreads();
    filter_rows<kFwdStride, kTile>(tx, hx, kFwdIn, kTile);
    filter_rows<kFwdStride, kTile>(ty, hy, kFwdIn, kTile);
    __syncthreads();
    const SsimPixel p = ssim_pixel<kFwdStride>(tx, ty, i, j, filter_col<kTile>(hx, i, j), filter_col<kTile>(hy, i, j), C1, C2);
    const float ws = wave_total_lane63(valid ? p.S : 0.f), wc = wave_total_lane63(valid ? p.cs : 0.f);
    if ((threadIdx.x & 63) == 63) {
      part[threadIdx.x >> 6] = ws;
      part[4 + (threadIdx.x >> 6)] = wc;
    }
    __syncthreads();
    if (threadIdx.x == 255) {
      float* o = partial + ((n * C + c) * tiles + tile) * 2;
      o[0] = ((part[0] + part[1]) + part[2]) + part[3];
      o[1] = ((part[4] + part[5]) + part[6]) + part[7];
    }
  }
}

// grid: N * C workgroups of 64; out [N][C][2] = (mean ssim, mean cs)
__global__ __launch_bounds__(64) void ssim_finish_kernel(const float* __restrict__ partial, int tiles, double count, float* __restrict__ out) {
  __shared__ double acc[2][64];
  const float* p = partial + (int64_t)blockIdx.x * tiles * 2;
  double a = 0.0, b = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    a = a + (double)p[2 * t];
    b = b + (double)p[2 * t + 1];
  }
  acc[0][threadIdx.x] = a;
  acc[1][threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0.0;
  b = 0.0;
  for (int l = 0; l < 64; ++l) {
    a = a + acc[0][l];
    b = b + acc[1][l];
  }
  out[(int64_t)blockIdx.x * 2] = (float)(a / count);
  out[(int64_t)blockIdx.x * 2 + 1] = (float)(b / count);
}

// grid: N * tiles workgroups of 256 over the IMAGE's 16 x 16 tiles; the moments of the 26 x 26 map pixels whose windows reach the tile
// are recomputed from a 36 x 36 input tile
__global__ __launch_bounds__(256) void ssim_backward_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ g,
                                                            int H, int W, int C, int tiles_x, int tiles, float C1, float C2, double count,
                                                            float* __restrict__ g_x) {
  __shared__ float tx[kBwdIn * kBwdStride], ty[kBwdIn * kBwdStride], hx[kBwdIn * kBwdMap], hy[kBwdIn * kBwdMap];
  __shared__ float D[3][kBwdMap * kBwdMapStride], h2[3][kBwdMap * kTile];
  const int64_t n = blockIdx.x / tiles;
  const int tile = blockIdx.x - (int)(n * tiles);
  const int p0 = (tile / tiles_x) * kTile, q0 = (tile % tiles_x) * kTile;
  const int i = threadIdx.x >> 4, j = threadIdx.x & 15;
  for (int c = 0; c < C; ++c) {
    load_tile<kBwdIn, kBwdStride>(x, y, n, H, W, C, c, p0 - kHalo, q0 - kHalo, tx, ty);
    __syncthreads();
    filter_rows<kBwdStride, kBwdMap>(tx, hx, kBwdIn, kBwdMap);
    filter_rows<kBwdStride, kBwdMap>(ty, hy, kBwdIn, kBwdMap);
    __syncthreads();
    for (int idx = threadIdx.x; idx < kBwdMap * kBwdMap; idx += 256) {
      const int r = idx / kBwdMap, q = idx - r * kBwdMap;
      const int vr = p0 - kHalo + r, vq = q0 - kHalo + q;  // the pixel of the valid map
      float d1 = 0.f, d12 = 0.f, dm = 0.f;
      if (vr >= 0 && vr < H - kHalo && vq >= 0 && vq < W - kHalo) {
        const SsimPixel p = ssim_pixel<kBwdStride>(tx, ty, r, q, filter_col<kBwdMap>(hx, r, q), filter_col<kBwdMap>(hy, r, q), C1, C2);
        const float P = p.B1 * p.B2;
        d1 = -p.S / p.B2;
        d12 = 2.f * p.A1 / P;
        const float dmu1 = 2.f * p.mu2 * p.N2 / P - 2.f * p.mu1 * p.S / p.B1;
        dm = (dmu1 - 2.f * p.mu1 * d1) - p.mu2 * d12;
      }
      D[0][r * kBwdMapStride + q] = dm;
      D[1][r * kBwdMapStride + q] = d1;
      D[2][r * kBwdMapStride + q] = d12;
    }
    __syncthreads();
    // G^T over the map = the same window over the 26 x 26 local maps (the taps are symmetric; the map is 0 outside)
#pragma unroll
    for (int m = 0; m < 3; ++m) filter_rows<kBwdMapStride, kTile>(D[m], h2[m], kBwdMap, kTile);
    __syncthreads();
    if (p0 + i < H && q0 + j < W) {
      const float t_dm = filter_col<kTile>(h2[0], i, j), t_d1 = filter_col<kTile>(h2[1], i, j), t_d12 = filter_col<kTile>(h2[2], i, j);
      const float xv = tx[(i + kHalo) * kBwdStride + j + kHalo], yv = ty[(i + kHalo) * kBwdStride + j + kHalo];
      const float s = (float)((double)g[n * C + c] / count);
      g_x[((n * H + p0 + i) * W + q0 + j) * C + c] = ((t_dm + 2.f * xv * t_d1) + yv * t_d12) * s;
    }
    __syncthreads();
  }
}

// one thread per output element of [N,Ho,Wo,C]; z = 0: x -> ox, z = 1: y -> oy
__global__ __launch_bounds__(256) void image_halve_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W, int C, int Ho,
                                                          int Wo, int64_t total, float* __restrict__ ox, float* __restrict__ oy) {
  const float* src = blockIdx.y == 0 ? x : y;
  float* dst = blockIdx.y == 0 ? ox : oy;
  const int ph = H & 1, pw = W & 1;
  for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int c = (int)(e % C);
    const int64_t pix = e / C;
    const int wo = (int)(pix % Wo), ho = (int)((pix / Wo) % Ho);
    const int64_t n = pix / ((int64_t)Wo * Ho);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = 2 * ho - ph + (k >> 1), q = 2 * wo - pw + (k & 1);
      const bool in = r >= 0 && r < H && q >= 0 && q < W;
      const float s = src[((n * H + (in ? r : 0)) * W + (in ? q : 0)) * C + c];
      v[k] = in ? s : 0.f;
    }
    dst[e] = (((v[0] + v[1]) + v[2]) + v[3]) * 0.25f;
  }
}

struct SsimShape { int tiles_x, tiles; int64_t blocks; };

// the shape contract shared by the entry points; map: tiles over the valid map (forward) or over the image (backward)
static int ssim_check(const char* who, int64_t N, int H, int W, int C, float data_range, bool map, SsimShape* s) {
  NA_REQUIRE(N >= 0, NA_EINVAL, "%s: N = %lld", who, (long long)N);
  NA_REQUIRE(C >= 1 && C <= 4, NA_EUNSUPPORTED, "%s: C = %d channels (1 .. 4)", who, C);
  NA_REQUIRE(H >= kTaps && W >= kTaps, NA_EUNSUPPORTED, "%s: a %d x %d image is smaller than the %d-tap window", who, H, W, kTaps);
  NA_REQUIRE(H <= kSsimMaxSide && W <= kSsimMaxSide, NA_EUNSUPPORTED, "%s: a %d x %d image (sides up to %d)", who, H, W, kSsimMaxSide);
  NA_REQUIRE(data_range > 0.f && data_range <= 65536.f, NA_EINVAL, "%s: data_range %g", who, (double)data_range);
  const int h = map ? H - kHalo : H, w = map ? W - kHalo : W;
  s->tiles_x = (w + kTile - 1) / kTile;
  s->tiles = s->tiles_x * ((h + kTile - 1) / kTile);
  s->blocks = N * s->tiles;
  NA_REQUIRE(s->blocks <= 0x7fffffffLL, NA_EUNSUPPORTED, "%s: %lld tiles in one launch", who, (long long)s->blocks);
  return NA_OK;
}

}  // namespace na

using namespace na;

#define NA_SSIM_PTR(who, p) NA_REQUIRE((p) != nullptr, NA_ENULL, who ": " #p " is NULL")

extern "C" {

size_t na_ssim_workspace_bytes(int64_t N, int H, int W, int C) {
  SsimShape s;
  if (ssim_check("na_ssim_workspace_bytes", N, H, W, C, 1.f, true, &s) != NA_OK) return 0;
  return (size_t)s.blocks * C * 2 * sizeof(float);
}

int na_ssim(const float* x, const float* y, int64_t N, int H, int W, int C, float data_range, float* out, void* workspace,
            size_t workspace_bytes, void* stream) {
  SsimShape s;
  if (int rc = ssim_check("na_ssim", N, H, W, C, data_range, true, &s)) return rc;
  if (N == 0) return NA_OK;
  NA_SSIM_PTR("na_ssim", x);
  NA_SSIM_PTR("na_ssim", y);
  NA_SSIM_PTR("na_ssim", out);
  NA_SSIM_PTR("na_ssim", workspace);
  NA_REQUIRE(workspace_bytes >= (size_t)s.blocks * C * 2 * sizeof(float), NA_EWORKSPACE, "na_ssim: workspace of %zu bytes, %zu needed",
             workspace_bytes, (size_t)s.blocks * C * 2 * sizeof(float));
  const float C1 = (float)((0.01 * data_range) * (0.01 * data_range)), C2 = (float)((0.03 * data_range) * (0.03 * data_range));
  hipLaunchKernelGGL(ssim_tiles_kernel, dim3((unsigned)s.blocks), dim3(256), 0, (hipStream_t)stream, x, y, H, W, C, s.tiles_x, s.tiles, C1, C2,
                     (float*)workspace);
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)(N * C)), dim3(64), 0, (hipStream_t)stream, (const float*)workspace, s.tiles,
                     (double)(H - kHalo) * (double)(W - kHalo), out);
  return check_launch("na_ssim");
}

int na_ssim_backward(const float* x, const float* y, const float* g, int64_t N, int H, int W, int C, float data_range, float* g_x,
                     void* stream) {
  SsimShape s;
  if (int rc = ssim_check("na_ssim_backward", N, H, W, C, data_range, false, &s)) return rc;
  if (N == 0) return NA_OK;
  NA_SSIM_PTR("na_ssim_backward", x);
  NA_SSIM_PTR("na_ssim_backward", y);
  NA_SSIM_PTR("na_ssim_backward", g);
  NA_SSIM_PTR("na_ssim_backward", g_x);
  const float C1 = (float)((0.01 * data_range) * (0.01 * data_range)), C2 = (float)((0.03 * data_range) * (0.03 * data_range));
  hipLaunchKernelGGL(ssim_backward_kernel, dim3((unsigned)s.blocks), dim3(256), 0, (hipStream_t)stream, x, y, g, H, W, C, s.tiles_x, s.tiles, C1,
                     C2, (double)(H - kHalo) * (double)(W - kHalo), g_x);
  return check_launch("na_ssim_backward");
}

int na_image_halve(const float* x, const float* y, int64_t N, int H, int W, int C, float* out_x, float* out_y, void* stream) {
  NA_REQUIRE(N >= 0, NA_EINVAL, "na_image_halve: N = %lld", (long long)N);
  NA_REQUIRE(C >= 1 && C <= 4, NA_EUNSUPPORTED, "na_image_halve: C = %d channels (1 .. 4)", C);
  NA_REQUIRE(H >= 1 && W >= 1 && H <= kSsimMaxSide && W <= kSsimMaxSide, NA_EUNSUPPORTED, "na_image_halve: a %d x %d image (sides 1 .. %d)", H,
             W, kSsimMaxSide);
  if (N == 0) return NA_OK;
  NA_SSIM_PTR("na_image_halve", x);
  NA_SSIM_PTR("na_image_halve", out_x);
  NA_REQUIRE((y == nullptr) == (out_y == nullptr), NA_ENULL, "na_image_halve: y and out_y go together, one of them is NULL");
  const int Ho = H / 2 + (H & 1), Wo = W / 2 + (W & 1);
  const int64_t total = N * Ho * Wo * C;
  hipLaunchKernelGGL(image_halve_kernel, dim3(grid_for(total, 256, 1 << 16), y != nullptr ? 2 : 1), dim3(256), 0, (hipStream_t)stream, x, y, H, W,
                     C, Ho, Wo, total, out_x, out_y);
  return check_launch("na_image_halve");
}

}  // extern "C"
