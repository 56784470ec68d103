// The spline-length regularisers of DynamicNeRFVoxel (arc_len, src/nerf.py:1509-1520; runner.py:784-796): the length
// of the polyline through M points of a Bezier spline,
//   p_j = de_casteljau(control points, t_j), j = 0 .. M-1        len = sum_j |p_{j+1} - p_j|_2
// with t an INPUT table (the host passes torch.linspace(0, 1, M)'s own fp32 values: j / (M - 1) formed here differs in the last bit).
//   na_grid_spline_len[_backward]        the m = spline - 1 control points stored in a row of a grid [rows, 3 m], at flat row indices
//                                        (--voxel-random-spline-len-decay: control point 0 is NOT prepended there); mean over the indices
//   na_dyn_voxel_spline_len[_backward]   per sample: control points 1 .. n-1 interpolated from ctrl_pts_grid by NeRFVoxel's lookup
//                                        (voxel_cell.h, as na_dyn_voxel_warp) behind the zero control point 0, all in registers;
//                                        mean over the samples of w[n] len[n] (--spline-len-decay)
// Every operation is fp32 in the reference's order (this unit is built with -ffp-contract=off): 1 - t, the n - 1 levels
// b_j <- b_j (1 - t) + b_{j+1} t, the difference, (dx^2 + dy^2) + dz^2, sqrtf, the sum over the segments in segment order.
// The levels and the Bernstein recurrence are dyn_voxel_spline.h's (dv_casteljau, dv_bernstein_levels), called directly: the length
// is de_casteljau at n == 4 as well, never dv_spline's cubic form.
//
// GRADIENT.  d len / d control point k = sum_j dir_j (B_k(t_{j+1}) - B_k(t_j)) with dir_j = (p_{j+1} - p_j) / |p_{j+1} - p_j|, and
// dir_j = 0 for a segment of length 0 (torch.linalg.vector_norm's gradient there: 0, not NaN); the points are recomputed by the same
// de Casteljau levels as the value, so that a segment has length 0 in both or in neither.  The Bernstein differences do not depend on
// the sample: a workgroup forms the (M - 1) x n table once, in LDS.  There is no gradient w.r.t. pts or w.
//
// ORDER OF THE VALUE'S SUM (tests/spline_len_ref.py derives the bound from it): a thread adds its samples' addends (one per
// grid-stride step), the 64 threads of a wave are added by wave_total_lane63, the four waves of a workgroup in wave order through
// LDS, and the workgroups' partials are combined by one atomic each: fp32 atomics by default, 2^-40 fixed point under
// na_set_deterministic (bitwise reproducible).  The workgroup that arrives last divides by the count in double and stores the value
// with one rounding (na_grid_tv's protocol: out[1] counts arriving waves).
#include "voxel_scatter.h"
#include "dyn_voxel_spline.h"

namespace na {

constexpr int kSlMaxM = 32;               // points on the spline at most (Python uses 16)
constexpr int64_t kSlMaxBlocks = 1 << 18;  // beyond 2^26 samples a thread takes a second sample

// dB[j * NP + k] = B_k(t_{j+1}) - B_k(t_j), j = 0 .. M-2, once per workgroup (ends with a barrier)
template <int NP>
__device__ __forceinline__ void sl_bernstein_steps(const float* __restrict__ t, int M, float* dB) {
  for (int j = threadIdx.x; j < M - 1; j += blockDim.x) {
    float B0[NP], B1[NP];
    dv_bernstein_levels<NP>(t[j], B0);
    dv_bernstein_levels<NP>(t[j + 1], B1);
#pragma unroll
    for (int k = 0; k < NP; ++k) dB[j * NP + k] = B1[k] - B0[k];
  }
  __syncthreads();
}

// the length; GRAD: G[k] <- d len / d P[k] as well (dB: sl_bernstein_steps' table)
template <int NP, bool GRAD>
__device__ __forceinline__ float sl_arc(const float (&P)[NP][3], const float* __restrict__ t, int M, const float* dB, float (&G)[NP][3]) {
  float prev[3], len = 0.f;
  dv_casteljau<NP>(P, t[0], prev);
  if (GRAD) {
#pragma unroll
    for (int k = 0; k < NP; ++k) G[k][0] = G[k][1] = G[k][2] = 0.f;
  }
#pragma unroll 1
  for (int j = 1; j < M; ++j) {
    float cur[3], d[3];
    dv_casteljau<NP>(P, t[j], cur);
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = cur[a] - prev[a];
    const float l = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    len = len + l;
    if (GRAD) {
      float dir[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) dir[a] = l == 0.f ? 0.f : d[a] / l;  // (a NaN length stays loud)
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        const float s = dB[(j - 1) * NP + k];
#pragma unroll
        for (int a = 0; a < 3; ++a) G[k][a] = G[k][a] + dir[a] * s;
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) prev[a] = cur[a];
  }
  return len;
}

// every thread of the launch (workgroups of 256) calls this once: out[0] <- (sum of acc over the launch) / count.  The four waves of a
// workgroup meet in LDS and arrive together: all partial sums land on ONE cache line (out[0], out[1]), whose atomics the L2 serialises,
// so a launch pays for them per workgroup, not per wave.
__device__ __forceinline__ void sl_mean(float acc, float* __restrict__ out, long long* __restrict__ fix, double count) {
  __shared__ float part[4];
  const float wave = wave_total_lane63(acc);
  if ((threadIdx.x & 63) == 63) part[threadIdx.x >> 6] = wave;
  __syncthreads();
  if (threadIdx.x != 255) return;
  const float total = ((part[0] + part[1]) + part[2]) + part[3];
  // (a partial of 2^20 and more, or a non-finite one, goes to the fp32 side in the deterministic mode too, as accumulate() sends it)
  if (fix != nullptr && fabsf(total) < 1048576.0f) atomicAdd((unsigned long long*)fix, (unsigned long long)__float2ll_rn(total * kFixScale));
  else atomicAdd(out, total);
  __threadfence();
  unsigned* arrived = (unsigned*)(out + 1);
  if (atomicAdd(arrived, 4u) != 4u * (gridDim.x - 1)) return;  // (the arriving waves, a workgroup's four at once)
  __threadfence();
  double sum = (double)atomicAdd(out, 0.f);
  if (fix != nullptr) sum = sum + (double)(long long)atomicAdd((unsigned long long*)fix, 0ull) * (1.0 / 1099511627776.0);
  out[0] = (float)(sum / count);
}

// Memory safety is unconditional: the index is brought into 0 .. rows-1 by selects before anything is formed from it.
__device__ __forceinline__ int64_t sl_row(int64_t idx, int64_t rows) {
  const int64_t top = rows - 1;
  return idx >= 0 ? (idx <= top ? idx : top) : 0;
}

// ------------------------------------------------------------------------------------ the grid term
// one thread per index; out[0] and the arrival counter behind it (out[1]) are zeroed by the caller
template <int NP>
__global__ __launch_bounds__(256) void grid_spline_len_kernel(const float* __restrict__ grid, int64_t rows, const int64_t* __restrict__ idxs,
                                                              int64_t K, const float* __restrict__ t, int M, float* __restrict__ lens,
                                                              float* __restrict__ out, long long* __restrict__ fix) {
  float acc = 0.f;
  for (int64_t base = blockIdx.x * (int64_t)256; base < K; base += (int64_t)gridDim.x * 256) {  // (the same trips for the whole workgroup)
    const int64_t i = base + threadIdx.x;
    if (i < K) {
      const float* q = grid + sl_row(idxs[i], rows) * (3 * NP);
      float P[NP][3], G[NP][3];
#pragma unroll
      for (int k = 0; k < NP; ++k) {
#pragma unroll
        for (int a = 0; a < 3; ++a) P[k][a] = q[3 * k + a];
      }
      const float len = sl_arc<NP, false>(P, t, M, nullptr, G);
      if (lens != nullptr) lens[i] = len;
      acc = acc + len;
    }
  }
  sl_mean(acc, out, fix, (double)K);
}

template <int NP>
__global__ __launch_bounds__(256) void grid_spline_len_backward_kernel(const float* __restrict__ grid, int64_t rows,
                                                                       const int64_t* __restrict__ idxs, int64_t K, const float* __restrict__ t,
                                                                       int M, const float* __restrict__ g_up, float* __restrict__ g_grid,
                                                                       long long* __restrict__ fix) {
  __shared__ float dB[(kSlMaxM - 1) * NP];
  sl_bernstein_steps<NP>(t, M, dB);
  const float s = (float)((double)g_up[0] / (double)K);
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < K; i += (int64_t)gridDim.x * 256) {
    const int64_t at = sl_row(idxs[i], rows) * (3 * NP);
    float P[NP][3], G[NP][3];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) P[k][a] = grid[at + 3 * k + a];
    }
    sl_arc<NP, true>(P, t, M, dB, G);
#pragma unroll
    for (int k = 0; k < NP; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) accumulate(g_grid, fix, at + 3 * k + a, G[k][a] * s);
    }
  }
}

// ------------------------------------------------------------------------------------ the per-sample term
// the control points of a sample: zero, then 1 .. NC-1 by na_dyn_voxel_warp's gather (dv_gather; P[1 ..] is 3(NC-1) floats in a row)
template <int NC>
__device__ __forceinline__ void sl_gather(const float* __restrict__ ctrl, const VoxCell& c, const VoxGrid& g, float (&P)[NC][3]) {
  P[0][0] = P[0][1] = P[0][2] = 0.f;
  dv_gather<NC, true, false, false>(c, g, ctrl, nullptr, nullptr, &P[1][0], nullptr, nullptr, nullptr);
}

// one thread per sample (S = 64, n = 4: 9.4 MiB of control points, L2 / Infinity Cache resident; the work is the VALU stream)
template <int NC>
__global__ __launch_bounds__(256) void dyn_voxel_spline_len_kernel(const float* __restrict__ pts, int64_t N, VoxGrid g,
                                                                   const float* __restrict__ ctrl, const float* __restrict__ w,
                                                                   const float* __restrict__ t, int M, float* __restrict__ lens,
                                                                   float* __restrict__ out, long long* __restrict__ fix) {
  float acc = 0.f;
  for (int64_t base = blockIdx.x * (int64_t)256; base < N; base += (int64_t)gridDim.x * 256) {
    const int64_t n = base + threadIdx.x;
    if (n < N) {
      const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
      float P[NC][3], G[NC][3];
      sl_gather<NC>(ctrl, c, g, P);
      const float len = sl_arc<NC, false>(P, t, M, nullptr, G);
      if (lens != nullptr) lens[n] = len;
      acc = acc + (w != nullptr ? w[n] * len : len);
    }
  }
  sl_mean(acc, out, fix, (double)N);
}

// corner u of a sample adds w_u (g_up w[n] / N) d len / d control point k to channels 3(k-1) .. 3k-1 of ctrl row_u: one wide row of
// W = 3(NC-1) sums per grid row on voxel_scatter.h's table
template <int NC>
__global__ __launch_bounds__(256) void dyn_voxel_spline_len_backward_kernel(const float* __restrict__ pts, int64_t N, VoxGrid g,
                                                                            const float* __restrict__ ctrl, const float* __restrict__ w,
                                                                            const float* __restrict__ t, int M, const float* __restrict__ g_up,
                                                                            float* __restrict__ g_ctrl, long long* __restrict__ fix) {
  constexpr int W = 3 * (NC - 1), ROWS = DvTable<W>::ROWS;
  static_assert(ROWS * W * 8 + ROWS * 4 + (kSlMaxM - 1) * NC * 4 <= 65536, "the table, its tags and the Bernstein steps stay inside 64 KB of LDS");
  __shared__ uint32_t tags[ROWS];
  __shared__ unsigned long long vals[ROWS * W];
  __shared__ float dB[(kSlMaxM - 1) * NC];
  const DvTable<W> table{tags, vals, fix};
  auto add_global = [&](uint32_t id, int e, float v) { accumulate(g_ctrl, fix, (int64_t)id * W + e, v); };
  table.clear();
  sl_bernstein_steps<NC>(t, M, dB);
  const float s0 = (float)((double)g_up[0] / (double)N);
  int64_t n_lo, n_hi;
  dv_run(N, n_lo, n_hi);
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    if (n >= n_hi) continue;  // (no barrier inside the loop)
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    float P[NC][3], G[NC][3], sv[W];
    sl_gather<NC>(ctrl, c, g, P);
    sl_arc<NC, true>(P, t, M, dB, G);
    const float s = w != nullptr ? s0 * w[n] : s0;
#pragma unroll
    for (int k = 1; k < NC; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) sv[3 * (k - 1) + a] = G[k][a] * s;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) table.add_row((uint32_t)vox_row(c, u, g.S), vox_weight(c, u), sv, add_global);
  }
  table.flush([&](uint32_t id, int e, unsigned long long v) { table.put(g_ctrl, fix, (int64_t)id * W + e, v); });
}

static int sl_check_table(const char* who, const float* t, int M) {
  NA_REQUIRE(M >= 2 && M <= kSlMaxM, NA_EUNSUPPORTED, "%s: M = %d points on the spline (2 .. %d)", who, M, kSlMaxM);
  NA_REQUIRE(t != nullptr, NA_ENULL, "%s: null pointer", who);
  return NA_OK;
}

static int sl_check_grid(const char* who, int64_t rows, int m, int64_t K) {
  NA_REQUIRE(rows >= 1 && rows <= ((int64_t)1 << 30), NA_EINVAL, "%s: %lld rows (1 .. 2^30)", who, (long long)rows);
  NA_REQUIRE(m >= 1 && m <= 10, NA_EUNSUPPORTED, "%s: %d control points per row (1 .. 10: spline 2 .. 11)", who, m);
  NA_REQUIRE(K >= 1, NA_EINVAL, "%s: %lld indices", who, (long long)K);
  return NA_OK;
}

}  // namespace na

using namespace na;

extern "C" {

int na_grid_spline_len(const float* grid, int64_t rows, int m, const int64_t* idxs, int64_t K, const float* t, int M, float* lens, float* out,
                       void* stream) {
  if (int rc = sl_check_grid("na_grid_spline_len", rows, m, K)) return rc;
  if (int rc = sl_check_table("na_grid_spline_len", t, M)) return rc;
  NA_REQUIRE(grid && idxs && out, NA_ENULL, "na_grid_spline_len: null pointer");
  int rc;
  long long* fix = det_begin(1, (hipStream_t)stream, "na_grid_spline_len", &rc);
  if (rc != NA_OK) return rc;
#define NA_SL_GRID_FWD(NC)                                                                                                             \
  hipLaunchKernelGGL(grid_spline_len_kernel<NC - 1>, dim3(grid_for(K, 256, kSlMaxBlocks)), dim3(256), 0, (hipStream_t)stream, grid, rows, \
                     idxs, K, t, M, lens, out, fix)
  NA_DV_DISPATCH(m + 1, NA_SL_GRID_FWD)
#undef NA_SL_GRID_FWD
  return check_launch("na_grid_spline_len");
}

int na_grid_spline_len_backward(const float* grid, int64_t rows, int m, const int64_t* idxs, int64_t K, const float* t, int M,
                                const float* g_up, float* g_grid, void* stream) {
  if (int rc = sl_check_grid("na_grid_spline_len_backward", rows, m, K)) return rc;
  if (int rc = sl_check_table("na_grid_spline_len_backward", t, M)) return rc;
  NA_REQUIRE(grid && idxs && g_up && g_grid, NA_ENULL, "na_grid_spline_len_backward: null pointer");
  int rc;
  const size_t total = (size_t)rows * 3 * m;
  long long* fix = det_begin(total, (hipStream_t)stream, "na_grid_spline_len_backward", &rc);
  if (rc != NA_OK) return rc;
#define NA_SL_GRID_BWD(NC)                                                                                                              \
  hipLaunchKernelGGL(grid_spline_len_backward_kernel<NC - 1>, dim3(grid_for(K, 256, 4096)), dim3(256), 0, (hipStream_t)stream, grid, rows, \
                     idxs, K, t, M, g_up, g_grid, fix)
  NA_DV_DISPATCH(m + 1, NA_SL_GRID_BWD)
#undef NA_SL_GRID_BWD
  if (fix != nullptr) return det_finish(fix, total, g_grid, (hipStream_t)stream, "na_grid_spline_len_backward");
  return check_launch("na_grid_spline_len_backward");
}

int na_dyn_voxel_spline_len(const float* pts, int64_t N, const float* ctrl_pts_grid, int S, int n_ctrl, double grid_radius, const float* w,
                            const float* t, int M, float* lens, float* out, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_spline_len", N, S, n_ctrl, grid_radius)) return rc;
  if (int rc = sl_check_table("na_dyn_voxel_spline_len", t, M)) return rc;
  NA_REQUIRE(N >= 1, NA_EINVAL, "na_dyn_voxel_spline_len: the mean over no samples");
  NA_REQUIRE(pts && ctrl_pts_grid && out, NA_ENULL, "na_dyn_voxel_spline_len: null pointer");
  int rc;
  long long* fix = det_begin(1, (hipStream_t)stream, "na_dyn_voxel_spline_len", &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
#define NA_SL_DYN_FWD(NC)                                                                                                                 \
  hipLaunchKernelGGL(dyn_voxel_spline_len_kernel<NC>, dim3(grid_for(N, 256, kSlMaxBlocks)), dim3(256), 0, (hipStream_t)stream, pts, N, g, \
                     ctrl_pts_grid, w, t, M, lens, out, fix)
  NA_DV_DISPATCH(n_ctrl, NA_SL_DYN_FWD)
#undef NA_SL_DYN_FWD
  return check_launch("na_dyn_voxel_spline_len");
}

int na_dyn_voxel_spline_len_backward(const float* pts, int64_t N, const float* ctrl_pts_grid, int S, int n_ctrl, double grid_radius,
                                     const float* w, const float* t, int M, const float* g_up, float* g_ctrl_pts_grid, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_spline_len_backward", N, S, n_ctrl, grid_radius)) return rc;
  if (int rc = sl_check_table("na_dyn_voxel_spline_len_backward", t, M)) return rc;
  NA_REQUIRE(N >= 1, NA_EINVAL, "na_dyn_voxel_spline_len_backward: the mean over no samples");
  NA_REQUIRE(pts && ctrl_pts_grid && g_up && g_ctrl_pts_grid, NA_ENULL, "na_dyn_voxel_spline_len_backward: null pointer");
  const size_t total = (size_t)S * S * S * 3 * (size_t)(n_ctrl - 1);
  int rc;
  long long* fix = det_begin(total, (hipStream_t)stream, "na_dyn_voxel_spline_len_backward", &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
#define NA_SL_DYN_BWD(NC)                                                                                                                   \
  hipLaunchKernelGGL(dyn_voxel_spline_len_backward_kernel<NC>, dim3(grid_for(N, 256, DV_WG)), dim3(256), 0, (hipStream_t)stream, pts, N, g, \
                     ctrl_pts_grid, w, t, M, g_up, g_ctrl_pts_grid, fix)
  NA_DV_DISPATCH(n_ctrl, NA_SL_DYN_BWD)
#undef NA_SL_DYN_BWD
  if (fix != nullptr) return det_finish(fix, total, g_ctrl_pts_grid, (hipStream_t)stream, "na_dyn_voxel_spline_len_backward");
  return check_launch("na_dyn_voxel_spline_len_backward");
}

}  // extern "C"
