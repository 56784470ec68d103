// Operators on a dense channel-last grid [s0,s1,s2,C] (NeRFVoxel's densities and rgb):
//   na_grid_tv, na_grid_tv_backward   total_variation (src/nerf.py:381-399) at given flat indices, and its gradient
//   na_grid_upsample                  upsample_grid (src/nerf.py:377-379): F.interpolate(mode="trilinear", align_corners=False)
//
// total_variation is reproduced, not improved:
//   decode      x = idx % s0, y = (idx / s0) % s1, z = (idx / (s0 s1)) % s2 -- x is the FASTEST digit of idx and the SLOWEST axis in
//               memory (row = (x s1 + y) s2 + z); the same draw names the same voxels as the reference
//   neighbour   v + 1, or v - 1 where v == s - 1, per axis
//   element     t = sqrt(clamp(dx^2 + dy^2 + dz^2, min = 1e-10)), d = voxel - neighbour, per (sample, channel); every operation is the
//               reference's fp32 operation in its order: subtract, square, (dx^2 + dy^2) + dz^2, clamp, sqrtf (this unit is built with
//               -ffp-contract=off).  The clamp keeps NaN (clamp_keep_nan; fmaxf would turn it into 1e-10).
//   value       mean of t over all K = samples x C elements
//   gradient    zero where q = dx^2 + dy^2 + dz^2 < fp32(1e-10) (torch's clamp passes the gradient where q >= min, and passes none for a
//               NaN q: the addends are then d x 0, NaN exactly where the difference is not finite); otherwise the voxel gets
//               (dx + dy + dz) w and each neighbour -d w with w = (g / K) / t.  idxs is drawn with replacement: duplicates add up.
//
// ORDER OF THE VALUE'S SUM (tests/grid_ref.py derives the bound from it): a thread adds the t of its sample's C channels in channel
// order (a grid-stride step further on: the next sample's, after them), the 64 threads of a wave are added by wave_total_lane63 (a tree
// of depth 6), and the waves' partials -- one per wave, one wave per workgroup -- are combined by one atomic each, in arrival order:
// fp32 atomics by default, 2^-40 fixed point under na_set_deterministic (integer addition: bitwise reproducible).  The wave that arrives
// last divides the total by K in double and stores the value with one rounding.
#include "common.h"
#include <math.h>

namespace na {

constexpr float kTvMin = 1e-10f;          // fp32(1e-10): what the fp32 tensor is compared with
constexpr int64_t kTvMaxWaves = 1 << 20;  // beyond 2^26 samples a thread takes a second sample

struct TvGrid {
  uint32_t s0, s1, s2, n_elem;
  int C;
};

struct TvRows { int64_t e, x, y, z; };  // offsets of channel 0 of the voxel's row and of its three neighbours' rows

// Memory safety is unconditional: the index is brought into 0 .. n_elem-1 by selects before anything is formed from it; its digits
// are then inside their axes and every neighbour is v + 1 <= s - 1 or v - 1 >= 0 (s >= 2 is checked by the entry points).
__device__ __forceinline__ TvRows tv_rows(int64_t idx, const TvGrid& g) {
  const int64_t top = (int64_t)g.n_elem - 1;
  idx = idx >= 0 ? (idx <= top ? idx : top) : 0;
  const uint32_t i = (uint32_t)idx;
  const uint32_t x = i % g.s0, y = (i / g.s0) % g.s1, z = (i / (g.s0 * g.s1)) % g.s2;
  const uint32_t ax = x == g.s0 - 1 ? x - 1 : x + 1, ay = y == g.s1 - 1 ? y - 1 : y + 1, az = z == g.s2 - 1 ? z - 1 : z + 1;
  TvRows r;
  r.e = (((int64_t)x * g.s1 + y) * g.s2 + z) * g.C;
  r.x = (((int64_t)ax * g.s1 + y) * g.s2 + z) * g.C;
  r.y = (((int64_t)x * g.s1 + ay) * g.s2 + z) * g.C;
  r.z = (((int64_t)x * g.s1 + y) * g.s2 + az) * g.C;  // (adjacent in memory to the voxel's own row)
  return r;
}

struct TvElem { float dx, dy, dz, q; };

__device__ __forceinline__ TvElem tv_elem(const float* __restrict__ grid, const TvRows& r, int c) {
  const float e = grid[r.e + c];
  TvElem t;
  t.dx = e - grid[r.x + c];
  t.dy = e - grid[r.y + c];
  t.dz = e - grid[r.z + c];
  t.q = (t.dx * t.dx + t.dy * t.dy) + t.dz * t.dz;
  return t;
}

// ------------------------------------------------------------------------------------ value
// one thread per sample, one wave per workgroup; out[0] and the arrival counter behind it (out[1]) are zeroed by the caller
__global__ __launch_bounds__(64) void grid_tv_kernel(const float* __restrict__ grid, TvGrid g, const int64_t* __restrict__ idxs, int64_t n,
                                                     float* __restrict__ out, long long* __restrict__ fix) {
  float acc = 0.f;
  for (int64_t base = blockIdx.x * (int64_t)64; base < n; base += (int64_t)gridDim.x * 64) {  // (the same trips for the whole wave)
    const int64_t i = base + threadIdx.x;
    if (i < n) {
      const TvRows r = tv_rows(idxs[i], g);
      for (int c = 0; c < g.C; ++c) {
        const TvElem t = tv_elem(grid, r, c);
        acc = acc + sqrtf(clamp_keep_nan(t.q, kTvMin, __builtin_inff()));
      }
    }
  }
  const float total = wave_total_lane63(acc);
  if (threadIdx.x != 63) return;
  // (a partial of 2^20 and more, or a non-finite one, goes to the fp32 side in the deterministic mode too, as accumulate() sends it)
  if (fix != nullptr && fabsf(total) < 1048576.0f) atomicAdd((unsigned long long*)fix, (unsigned long long)__float2ll_rn(total * kFixScale));
  else atomicAdd(out, total);
  __threadfence();
  unsigned* arrived = (unsigned*)(out + 1);
  if (atomicAdd(arrived, 1u) != gridDim.x - 1) return;
  __threadfence();
  double sum = (double)atomicAdd(out, 0.f);
  if (fix != nullptr) sum = sum + (double)(long long)atomicAdd((unsigned long long*)fix, 0ull) * (1.0 / 1099511627776.0);
  out[0] = (float)(sum / ((double)n * (double)g.C));
}

// ------------------------------------------------------------------------------------ gradient
// one thread per sample; d, q and t are recomputed.  Roundings of an addend (tests/grid_ref.py GRAD_C0): the difference 1, t 3.5
// (q: 2.5 on top of twice the difference's, halved by the root, + sqrtf's own), g / K 1, w = (g / K) / t 1, the product 1.  The
// voxel's own addend sums its three differences in double so that it carries the same count relative to (|dx| + |dy| + |dz|) w.
__global__ __launch_bounds__(256) void grid_tv_backward_kernel(const float* __restrict__ grid, TvGrid g, const int64_t* __restrict__ idxs,
                                                               int64_t n, const float* __restrict__ g_up, float* __restrict__ g_grid,
                                                               long long* __restrict__ fix) {
  const float s = (float)((double)g_up[0] / ((double)n * (double)g.C));
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const TvRows r = tv_rows(idxs[i], g);
    for (int c = 0; c < g.C; ++c) {
      const TvElem t = tv_elem(grid, r, c);
      if (t.q < kTvMin) continue;  // below the clamp: no gradient (false for a NaN q, which stays loud below)
      const float w = t.q >= kTvMin ? s / sqrtf(t.q) : 0.f;
      accumulate(g_grid, fix, r.e + c, (float)((((double)t.dx + (double)t.dy) + (double)t.dz) * (double)w));
      accumulate(g_grid, fix, r.x + c, -(t.dx * w));
      accumulate(g_grid, fix, r.y + c, -(t.dy * w));
      accumulate(g_grid, fix, r.z + c, -(t.dz * w));
    }
  }
}

// ------------------------------------------------------------------------------------ upsample
// ATen's area_pixel_compute_source_index / guard_index_and_lambda in fp32: src = max(scale (i + 0.5) - 0.5, 0), i0 = floor(src) (at most
// S - 1), i1 = min(i0 + 1, S - 1), lambda = src - i0 (exact).  torch's builds contract `scale * (i + 0.5) - 0.5` into one fused
// multiply-add, so the fma is written out here (this unit is built with -ffp-contract=off): with the product rounded on its own, src
// is one ulp away at 4 -> 6, i = 3, and the result leaves the blend bound of torch's own fp32 output (tests/test_grid_ref.py).
struct UpAxis { int i0, i1; float l0, l1; };

// same: R == S, where ATen copies -- both sources are voxel i itself (weights 1 and 0), so a NaN neighbour does not reach the output
__device__ __forceinline__ UpAxis up_axis(uint32_t i, float scale, int S, bool same) {
  float src = fmaf(scale, (float)i + 0.5f, -0.5f);
  src = src >= 0.f ? src : 0.f;
  UpAxis a;
  a.i0 = min((int)src, S - 1);
  a.i1 = same ? a.i0 : min(a.i0 + 1, S - 1);
  a.l1 = fminf(fmaxf(src - (float)a.i0, 0.f), 1.f);
  a.l0 = 1.0f - a.l1;
  return a;
}

// one thread per output voxel over all its channels; consecutive threads run along z, so a wave's stores are one contiguous run.
// The output is the sum of 8 products (wx wy) wz v in corner order (bit 0 of the corner: z) -- every product is formed, a zero weight
// on a NaN voxel gives NaN as it does in ATen.
__global__ __launch_bounds__(256) void grid_upsample_kernel(const float* __restrict__ src, int S, float* __restrict__ dst, int R, int C,
                                                            float scale) {
  const uint32_t n_out = (uint32_t)R * R * R;
  for (uint32_t o = blockIdx.x * blockDim.x + threadIdx.x; o < n_out; o += gridDim.x * blockDim.x) {
    const bool same = R == S;
    const UpAxis az = up_axis(o % R, scale, S, same), ay = up_axis((o / R) % R, scale, S, same),
                 ax = up_axis(o / ((uint32_t)R * R), scale, S, same);
    float w[8];
    int64_t row[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ix = (u & 4) ? ax.i1 : ax.i0, iy = (u & 2) ? ay.i1 : ay.i0, iz = (u & 1) ? az.i1 : az.i0;
      w[u] = (((u & 4) ? ax.l1 : ax.l0) * ((u & 2) ? ay.l1 : ay.l0)) * ((u & 1) ? az.l1 : az.l0);
      row[u] = (((int64_t)ix * S + iy) * S + iz) * C;
    }
    float* d = dst + (int64_t)o * C;
    for (int c = 0; c < C; ++c) {
      float v = 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) v = v + w[u] * src[row[u] + c];
      d[c] = v;
    }
  }
}

static int tv_check(const char* who, int s0, int s1, int s2, int C, int64_t n, TvGrid* g) {
  NA_REQUIRE(s0 >= 2 && s1 >= 2 && s2 >= 2 && s0 <= 1024 && s1 <= 1024 && s2 <= 1024, NA_EINVAL, "%s: grid %d x %d x %d (2 .. 1024 per axis)",
             who, s0, s1, s2);
  NA_REQUIRE(C >= 1 && C <= 32, NA_EINVAL, "%s: C = %d channels (1 .. 32)", who, C);
  NA_REQUIRE(n >= 1, NA_EINVAL, "%s: %lld samples", who, (long long)n);
  g->s0 = (uint32_t)s0; g->s1 = (uint32_t)s1; g->s2 = (uint32_t)s2; g->n_elem = (uint32_t)s0 * s1 * s2; g->C = C;
  return NA_OK;
}

}  // namespace na

using namespace na;

extern "C" {

int na_grid_tv(const float* grid, int s0, int s1, int s2, int C, const int64_t* idxs, int64_t n, float* out, void* stream) {
  TvGrid g;
  if (int rc = tv_check("na_grid_tv", s0, s1, s2, C, n, &g)) return rc;
  NA_REQUIRE(grid && idxs && out, NA_ENULL, "na_grid_tv: null pointer");
  int rc;
  long long* fix = det_begin(1, (hipStream_t)stream, "na_grid_tv", &rc);
  if (rc != NA_OK) return rc;
  hipLaunchKernelGGL(grid_tv_kernel, dim3(grid_for(n, 64, kTvMaxWaves)), dim3(64), 0, (hipStream_t)stream, grid, g, idxs, n, out, fix);
  return check_launch("na_grid_tv");
}

int na_grid_tv_backward(const float* grid, int s0, int s1, int s2, int C, const int64_t* idxs, int64_t n, const float* g_up, float* g_grid,
                        void* stream) {
  TvGrid g;
  if (int rc = tv_check("na_grid_tv_backward", s0, s1, s2, C, n, &g)) return rc;
  NA_REQUIRE(grid && idxs && g_up && g_grid, NA_ENULL, "na_grid_tv_backward: null pointer");
  int rc;
  const size_t total = (size_t)g.n_elem * C;
  long long* fix = det_begin(total, (hipStream_t)stream, "na_grid_tv_backward", &rc);
  if (rc != NA_OK) return rc;
  hipLaunchKernelGGL(grid_tv_backward_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, (hipStream_t)stream, grid, g, idxs, n, g_up,
                     g_grid, fix);
  if (fix != nullptr) return det_finish(fix, total, g_grid, (hipStream_t)stream, "na_grid_tv_backward");
  return check_launch("na_grid_tv_backward");
}

int na_grid_upsample(const float* src, int S, float* dst, int R, int C, void* stream) {
  NA_REQUIRE(S >= 2 && S <= 1024 && S % 2 == 0 && R >= 2 && R <= 1024 && R % 2 == 0, NA_EINVAL,
             "na_grid_upsample: resolutions %d -> %d (even, 2 .. 1024)", S, R);
  NA_REQUIRE(C >= 1 && C <= 32, NA_EINVAL, "na_grid_upsample: C = %d channels (1 .. 32)", C);
  NA_REQUIRE(src && dst, NA_ENULL, "na_grid_upsample: null pointer");
  const int64_t n_out = (int64_t)R * R * R;
  hipLaunchKernelGGL(grid_upsample_kernel, dim3(grid_for(n_out, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, src, S, dst, R, C,
                     (float)S / (float)R);
  return check_launch("na_grid_upsample");
}

}  // extern "C"
