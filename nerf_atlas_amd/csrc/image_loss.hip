// The reference's loss wrapper as one kernel each way (runner.py:552-594, src/utils.py:198-204, 279-314):
// --gamma-correct-loss, --tone-map, --color-spaces and --loss-fns l2 | l1 | rmse of an image pair got, ref [P,3] (fp32).
//   per channel   a = G == 1 ? x : (G == 0.5 ? sqrt : pow(., G))(clamp(x, min 1e-10));  the label takes no clamp
//                 b = tone map ? a / (1 + a) : a
//   per pixel     rgb        b                                                         3 channels
//                 hsv        (0, 0, max(b))  -- what the reference's rgb2hsv returns -- 3 channels, two of them identically 0
//                 luminance  (0.2126 r + 0.7152 g) + 0.0722 b                          1 channel
//                 xyz        ((m0 r + m1 g) + m2 b) / 0.17697 per row of the matrix    3 channels
//   per space     mse = mean d^2, mae = mean |d| over P x channels;  l2 = mse, l1 = mae, rmse = sqrt(clamp(mse, min 1e-10))
//   loss          (1 / S) sum over the S spaces of (1 / L) sum over the L functions
// na_image_loss            one launch: out[0] = loss, stats[0..3] = mse and stats[4..7] = mae of the spaces (bit order), 0 where off.
// na_image_loss_backward   one launch, one thread per pixel: g_got = g_up[0] d loss / d got from got, ref and stats.
//
// ORDER OF THE SUMS (bit-identical from run to run in every mode; no floating-point atomics): a thread adds its pixels (pixel
// p, p + grid, ...) in order, wave_total_lane63 adds the 64 threads of a wave, thread 255 the four waves in wave order and writes
// one row of eight partial sums per workgroup to the workspace.  The workgroup that arrives last (an integer counter in the
// workspace's first word: na_grid_tv's protocol) adds the rows in index order in double -- thread k column k --, and thread 0 forms
// the loss in double and rounds it once.  The counter wraps to 0 with the last arrival, so the workspace is ready for the next call.
//
// NaN: torch's clamp and max keep a NaN, fmaxf drops it; the clamps and the maximum below are comparisons.
// This unit is built with -ffp-contract=off: every product and sum is rounded on its own, as tests/image_loss_ref.py counts them.
#include "common.h"

namespace na {

constexpr int kLossBlock = 256;
constexpr int kLossMaxBlocks = 256;   // the grid stops growing at 65536 pixels; a thread then takes several
constexpr int kLossRow = 8;           // partial sums per workgroup: sum d^2 of the four spaces, then sum |d|
constexpr size_t kLossHeader = 64;    // bytes in front of the rows (the arrival counter)
constexpr int64_t kLossMaxP = (int64_t)1 << 40;
constexpr float kClampMin = 1e-10f;

struct LossCfg { int spaces, fns, tone_map; float G; };

__device__ __forceinline__ float gamma_fwd(float v, float G, bool clamp) {
  if (G == 1.f) return v;
  if (clamp) v = v < kClampMin ? kClampMin : v;  // (a NaN stays)
  return G == 0.5f ? sqrtf(v) : powf(v, G);
}
__device__ __forceinline__ float tone_fwd(float v, int tone_map) { return tone_map ? v / (1.f + v) : v; }

// torch.max over the channels: the value (NaN if any channel is), the LOWEST index on a tie
__device__ __forceinline__ float max3(float x0, float x1, float x2, int& k) {
  float m = x0;
  k = 0;
  if (m == m && (x1 > m || x1 != x1)) { m = x1; k = 1; }
  if (m == m && (x2 > m || x2 != x2)) { m = x2; k = 2; }
  return m;
}
__device__ __forceinline__ float luminance(const float* v) { return (0.2126f * v[0] + 0.7152f * v[1]) + 0.0722f * v[2]; }

__device__ static const float kXyz[3][3] = {{0.49f, 0.31f, 0.2f}, {0.17697f, 0.8124f, 0.01063f}, {0.f, 0.01f, 0.99f}};
constexpr float kXyzDiv = 0.17697f;
__device__ __forceinline__ float xyz_row(const float* v, int j) { return ((kXyz[j][0] * v[0] + kXyz[j][1] * v[1]) + kXyz[j][2] * v[2]) / kXyzDiv; }

// the chain up to the colour spaces for both images of pixel p
__device__ __forceinline__ void loss_pixel(const float* __restrict__ got, const float* __restrict__ ref, int64_t p, const LossCfg& c, float* a,
                                           float* b) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = tone_fwd(gamma_fwd(got[3 * p + k], c.G, true), c.tone_map);
    b[k] = tone_fwd(gamma_fwd(ref[3 * p + k], c.G, false), c.tone_map);
  }
}

__device__ __forceinline__ float agent_load(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// grid: min(ceil(P / 256), 256) workgroups of 256; ws: [counter | rows[gridDim.x][8]]
__global__ __launch_bounds__(kLossBlock) void image_loss_kernel(const float* __restrict__ got, const float* __restrict__ ref, int64_t P, LossCfg c,
                                                                 float* __restrict__ out, float* __restrict__ stats, unsigned* __restrict__ counter,
                                                                 float* __restrict__ rows) {
  __shared__ float part[4][kLossRow];
  __shared__ double col[kLossRow];
  __shared__ bool last;
  float acc[kLossRow];
#pragma unroll
  for (int k = 0; k < kLossRow; ++k) acc[k] = 0.f;
  for (int64_t p = blockIdx.x * (int64_t)kLossBlock + threadIdx.x; p < P; p += (int64_t)gridDim.x * kLossBlock) {
    float a[3], b[3];
    loss_pixel(got, ref, p, c, a, b);
    if (c.spaces & NA_SPACE_RGB) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float d = a[k] - b[k];
        acc[0] = acc[0] + d * d;
        acc[4] = acc[4] + fabsf(d);
      }
    }
    if (c.spaces & NA_SPACE_HSV) {
      int ka, kb;
      const float d = max3(a[0], a[1], a[2], ka) - max3(b[0], b[1], b[2], kb);
      acc[1] = acc[1] + d * d;
      acc[5] = acc[5] + fabsf(d);
    }
    if (c.spaces & NA_SPACE_LUMINANCE) {
      const float d = luminance(a) - luminance(b);
      acc[2] = acc[2] + d * d;
      acc[6] = acc[6] + fabsf(d);
    }
    if (c.spaces & NA_SPACE_XYZ) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float d = xyz_row(a, j) - xyz_row(b, j);
        acc[3] = acc[3] + d * d;
        acc[7] = acc[7] + fabsf(d);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kLossRow; ++k) {
    const float w = wave_total_lane63(acc[k]);
    if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6][k] = w;
  }
  __syncthreads();
  if (threadIdx.x == kLossBlock - 1) {
    float* row = rows + (int64_t)blockIdx.x * kLossRow;
#pragma unroll
    for (int k = 0; k < kLossRow; ++k) row[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    __threadfence();                                            // the agent-scope release of the row ...
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // ... drained before the ticket is drawn
    last = atomicInc(counter, gridDim.x - 1) == gridDim.x - 1;  // (wraps to 0 with the last arrival)
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  if (threadIdx.x < kLossRow) {
    double s = 0.0;
    for (unsigned r = 0; r < gridDim.x; ++r) s = s + (double)agent_load(rows + (int64_t)r * kLossRow + threadIdx.x);
    col[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int L = __popc(c.fns), S = __popc(c.spaces);
  double loss = 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    float mse = 0.f, mae = 0.f;
    if (c.spaces & (1 << s)) {
      const double n = (double)P * (s == 2 ? 1.0 : 3.0);  // (hsv's two zero channels count; luminance has one)
      mse = (float)(col[s] / n);
      mae = (float)(col[4 + s] / n);
      double f = 0.0;
      if (c.fns & NA_LOSS_L2) f = f + (double)mse;
      if (c.fns & NA_LOSS_L1) f = f + (double)mae;
      if (c.fns & NA_LOSS_RMSE) f = f + (double)sqrtf(mse < kClampMin ? kClampMin : mse);
      loss = loss + f / (double)L;
    }
    stats[s] = mse;
    stats[4 + s] = mae;
  }
  out[0] = (float)(loss / (double)S);
}

// d (mean over n of the functions of d) / d d, without the sign term: k2 d + k1 sign(d)
struct SpaceGrad { float k2, k1; };
__device__ __forceinline__ float space_term(const SpaceGrad& g, float d) { return g.k2 * d + (d > 0.f ? g.k1 : (d < 0.f ? -g.k1 : (d == d ? 0.f : d))); }

// grid: ceil(P / 256) workgroups (up to 2^20, then a thread takes several pixels); every element of g_got written once
__global__ __launch_bounds__(kLossBlock) void image_loss_backward_kernel(const float* __restrict__ got, const float* __restrict__ ref, int64_t P,
                                                                          LossCfg c, const float* __restrict__ stats, const float* __restrict__ g_up,
                                                                          float* __restrict__ g_got) {
  const int L = __popc(c.fns), S = __popc(c.spaces);
  const float w = g_up[0] / (float)(S * L);
  SpaceGrad sg[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const float n = (float)((double)P * (s == 2 ? 1.0 : 3.0));
    const float mse = stats[s];
    float k2 = 0.f;
    if (c.fns & NA_LOSS_L2) k2 = k2 + 2.f / n;
    // d sqrt(clamp(mse)) / d d = d / (n rmse) above the clamp (equality included), exactly 0 below; a NaN mse stays
    if (c.fns & NA_LOSS_RMSE) k2 = k2 + (mse < kClampMin ? 0.f : 1.f / (n * sqrtf(mse)));
    sg[s].k2 = w * k2;
    sg[s].k1 = (c.fns & NA_LOSS_L1) ? w / n : 0.f;
  }
  for (int64_t p = blockIdx.x * (int64_t)kLossBlock + threadIdx.x; p < P; p += (int64_t)gridDim.x * kLossBlock) {
    float a[3], b[3], g[3] = {0.f, 0.f, 0.f};
    loss_pixel(got, ref, p, c, a, b);
    if (c.spaces & NA_SPACE_RGB) {
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = g[k] + space_term(sg[0], a[k] - b[k]);
    }
    if (c.spaces & NA_SPACE_HSV) {
      int ka, kb;
      const float t = space_term(sg[1], max3(a[0], a[1], a[2], ka) - max3(b[0], b[1], b[2], kb));
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = g[k] + (k == ka ? t : 0.f);
    }
    if (c.spaces & NA_SPACE_LUMINANCE) {
      const float t = space_term(sg[2], luminance(a) - luminance(b));
      g[0] = g[0] + 0.2126f * t;
      g[1] = g[1] + 0.7152f * t;
      g[2] = g[2] + 0.0722f * t;
    }
    if (c.spaces & NA_SPACE_XYZ) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float t = space_term(sg[3], xyz_row(a, j) - xyz_row(b, j)) / kXyzDiv;
#pragma unroll
        for (int k = 0; k < 3; ++k) g[k] = g[k] + kXyz[j][k] * t;
      }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = got[3 * p + k];
      float v = g[k];
      float ag = x;  // the value after the gamma step
      float dg = 1.f;
      if (c.G != 1.f) {
        ag = gamma_fwd(x, c.G, true);
        dg = x >= kClampMin ? c.G * ag / x : 0.f;  // (torch's clamp: the gradient passes at equality, exactly 0 below and for a NaN)
      }
      if (c.tone_map) {
        const float q = 1.f + ag;
        v = v / (q * q);
      }
      g_got[3 * p + k] = dg == 0.f ? 0.f : v * dg;
    }
  }
}

static int loss_check(const char* who, int64_t P, int spaces, int fns, float G) {
  NA_REQUIRE(P >= 1 && P <= kLossMaxP, NA_EINVAL, "%s: P = %lld pixels (1 .. 2^40)", who, (long long)P);
  NA_REQUIRE(spaces != 0 && (spaces & ~15) == 0, NA_EINVAL, "%s: mask of colour spaces 0x%x (one or more of NA_SPACE_*)", who, spaces);
  NA_REQUIRE(fns != 0 && (fns & ~7) == 0, NA_EINVAL, "%s: mask of loss functions 0x%x (one or more of NA_LOSS_*)", who, fns);
  NA_REQUIRE(G > 0.f && G <= 3.4028234e38f, NA_EINVAL, "%s: gamma %g (finite and > 0)", who, (double)G);
  return NA_OK;
}

}  // namespace na

using namespace na;

extern "C" {

size_t na_image_loss_workspace_bytes(int64_t P) {
  if (P < 1 || P > kLossMaxP) return 0;
  return kLossHeader + (size_t)grid_for(P, kLossBlock, kLossMaxBlocks) * kLossRow * sizeof(float);
}

int na_image_loss(const float* got, const float* ref, int64_t P, int spaces, int fns, float gamma, int tone_map, float* out, float* stats,
                  void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = loss_check("na_image_loss", P, spaces, fns, gamma)) return rc;
  NA_REQUIRE(got && ref && out && stats && workspace, NA_ENULL, "na_image_loss: null pointer");
  NA_REQUIRE(workspace_bytes >= na_image_loss_workspace_bytes(P), NA_EWORKSPACE, "na_image_loss: workspace of %zu bytes, %zu needed",
             workspace_bytes, na_image_loss_workspace_bytes(P));
  const LossCfg c = {spaces, fns, tone_map != 0, gamma};
  hipLaunchKernelGGL(image_loss_kernel, dim3(grid_for(P, kLossBlock, kLossMaxBlocks)), dim3(kLossBlock), 0, (hipStream_t)stream, got, ref, P, c, out,
                     stats, (unsigned*)workspace, (float*)((char*)workspace + kLossHeader));
  return check_launch("na_image_loss");
}

int na_image_loss_backward(const float* got, const float* ref, int64_t P, int spaces, int fns, float gamma, int tone_map, const float* stats,
                           const float* g_up, float* g_got, void* stream) {
  if (int rc = loss_check("na_image_loss_backward", P, spaces, fns, gamma)) return rc;
  NA_REQUIRE(got && ref && stats && g_up && g_got, NA_ENULL, "na_image_loss_backward: null pointer");
  const LossCfg c = {spaces, fns, tone_map != 0, gamma};
  hipLaunchKernelGGL(image_loss_backward_kernel, dim3(grid_for(P, kLossBlock)), dim3(kLossBlock), 0, (hipStream_t)stream, got, ref, P, c, stats, g_up,
                     g_got);
  return check_launch("na_image_loss_backward");
}

}  // extern "C"
