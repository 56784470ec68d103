// DynamicNeRFVoxel (src/nerf.py:1526-1586): a D-NeRF without an MLP.  Two more dense grids over NeRFVoxel's S^3 cells --
// ctrl_pts_grid [S,S,S,3(n-1)], the control points 1 .. n-1 of a Bezier spline (control point 0 is zero), and rigidity_grid [S,S,S,1]
// -- are read by the SAME 8-neighbour lookup as the canonical grids (voxel_cell.h: cells and weights of the UNWARPED point in the
// reference's fp32 chain), and
//   dp       = cubic_bezier (n == 4, src/nerf.py:1201-1206) or de_casteljau (src/nerf.py:1173-1178) of the interpolated control points at t
//   rigidity = sigmoid(interpolated rigidity_grid)                 (the plain sigmoid, not na_bezier_warp's x / 2 form)
//   warped   = pts + dp * rigidity
// Two operators: the deformation as one launch (na_dyn_voxel_warp: a gather of 8 rows of 1 + 3(n-1) floats, the spline) and its
// backward (na_dyn_voxel_warp_backward: a scatter-add into the two grids on voxel_scatter.h's scheme).  There is no gradient
// w.r.t. pts: they are a leaf in the reference.  Kernels are instantiated per n = 2 .. 11 so that the control points stay in registers.
#include "voxel_scatter.h"
#include "dyn_voxel_spline.h"

namespace na {

// ------------------------------------------------------------------------------------ the deformation, one launch
// one thread per sample: 8 rows of 3(n-1) floats + 8 rigidity entries (S = 64, n = 4: 9.4 + 1 MiB of grids, L2 / Infinity Cache resident)
template <int NC>
__global__ __launch_bounds__(256) void dyn_voxel_warp_kernel(const float* __restrict__ pts, const float* __restrict__ t, int64_t N, VoxGrid g,
                                                             const float* __restrict__ ctrl, const float* __restrict__ rig,
                                                             float* __restrict__ warped, float* __restrict__ dp_out,
                                                             float* __restrict__ rig_out) {
  constexpr int CH = 3 * (NC - 1);
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    const float px = pts[n * 3], py = pts[n * 3 + 1], pz = pts[n * 3 + 2];
    const VoxCell c = vox_cell(px, py, pz, g);
    float cp[CH], rl, dp[3];
    dv_gather<NC, true, false, true>(c, g, ctrl, rig, nullptr, cp, &rl, nullptr, nullptr);
    dv_spline<NC>(cp, t[n], dp);
    const float r = sigmoidf_(rl);
    warped[n * 3] = px + dp[0] * r; warped[n * 3 + 1] = py + dp[1] * r; warped[n * 3 + 2] = pz + dp[2] * r;
    if (dp_out != nullptr) { dp_out[n * 3] = dp[0]; dp_out[n * 3 + 1] = dp[1]; dp_out[n * 3 + 2] = dp[2]; }
    if (rig_out != nullptr) rig_out[n] = r;
  }
}

// ------------------------------------------------------------------------------------ scatter-add into the two grids
// With r the rigidity, G = g_warped, D = G r + g_dp and q = (G . dp + g_rigidity) r (1 - r), corner u of a sample adds
//   w_u B_k(t) D  to channels 3(k-1) .. 3k-1 of ctrl row_u  (k = 1 .. n-1)      and      w_u q  to rigidity row_u:
// one "wide row" of W = 1 + 3(n-1) sums per grid row, [rigidity | control channels], summed by the scheme of voxel_scatter.h (a
// contiguous run of samples per workgroup, a hashed LDS table, one flush).  dp and rigidity are the forward's outputs (16 bytes per
// sample instead of gathering the 8 rows again).  Deterministic mode: every contribution to 2^-40 fixed point on its own, as
// every scatter on that table.
template <int NC>
__global__ __launch_bounds__(256) void dyn_voxel_warp_backward_kernel(const float* __restrict__ pts, const float* __restrict__ t, int64_t N,
                                                                      VoxGrid g, const float* __restrict__ dp, const float* __restrict__ rigidity,
                                                                      const float* __restrict__ g_warped, const float* __restrict__ g_dp,
                                                                      const float* __restrict__ g_rigidity, float* __restrict__ g_ctrl,
                                                                      float* __restrict__ g_rig, long long* __restrict__ fix) {
  constexpr int CH = 3 * (NC - 1), W = CH + 1, ROWS = DvTable<W>::ROWS;
  const int64_t S3 = (int64_t)g.S * g.S * g.S;
  long long* fix_rig = fix != nullptr ? fix + S3 * CH : nullptr;
  auto add_global = [&](uint32_t id, int e, float v) {
    if (e == 0) accumulate(g_rig, fix_rig, (int64_t)id, v);
    else accumulate(g_ctrl, fix, (int64_t)id * CH + (e - 1), v);
  };
  __shared__ uint32_t tags[ROWS];
  __shared__ unsigned long long vals[ROWS * W];
  const DvTable<W> table{tags, vals, fix};
  table.clear();
  int64_t n_lo, n_hi;
  dv_run(N, n_lo, n_hi);
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    if (n >= n_hi) continue;  // (no barrier inside the loop)
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    const float r = rigidity[n];
    float G[3] = {0.f, 0.f, 0.f}, D[3], gd = 0.f;
    if (g_warped != nullptr) { G[0] = g_warped[n * 3]; G[1] = g_warped[n * 3 + 1]; G[2] = g_warped[n * 3 + 2]; }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      D[a] = G[a] * r + (g_dp != nullptr ? g_dp[n * 3 + a] : 0.f);
      gd = gd + G[a] * dp[n * 3 + a];
    }
    if (g_rigidity != nullptr) gd = gd + g_rigidity[n];
    float B[NC], sv[W];
    dv_bernstein<NC>(t[n], B);
    sv[0] = gd * (r * (1.f - r));
#pragma unroll
    for (int k = 1; k < NC; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) sv[1 + 3 * (k - 1) + a] = B[k] * D[a];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) table.add_row((uint32_t)vox_row(c, u, g.S), vox_weight(c, u), sv, add_global);
  }
  table.flush([&](uint32_t id, int e, unsigned long long v) {
    table.put(e == 0 ? g_rig : g_ctrl, e == 0 ? fix_rig : fix, e == 0 ? (int64_t)id : (int64_t)id * CH + (e - 1), v);
  });
}

}  // namespace na

using namespace na;

extern "C" {

int na_dyn_voxel_warp(const float* pts, const float* t, int64_t N, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int n_ctrl,
                      double grid_radius, float* warped, float* dp, float* rigidity, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_warp", N, S, n_ctrl, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts && t && ctrl_pts_grid && rigidity_grid && warped, NA_ENULL, "na_dyn_voxel_warp: null pointer");
  const VoxGrid g = vox_grid(S, grid_radius);
#define NA_DV_FWD(NC)                                                                                                                    \
  hipLaunchKernelGGL(dyn_voxel_warp_kernel<NC>, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, t, N, g, ctrl_pts_grid, \
                     rigidity_grid, warped, dp, rigidity)
  NA_DV_DISPATCH(n_ctrl, NA_DV_FWD)
#undef NA_DV_FWD
  return check_launch("na_dyn_voxel_warp");
}

int na_dyn_voxel_warp_backward(const float* pts, const float* t, int64_t N, const float* dp, const float* rigidity, const float* g_warped,
                               const float* g_dp, const float* g_rigidity, int S, int n_ctrl, double grid_radius, float* g_ctrl_pts_grid,
                               float* g_rigidity_grid, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_warp_backward", N, S, n_ctrl, grid_radius)) return rc;
  if (N == 0 || (!g_warped && !g_dp && !g_rigidity)) return NA_OK;
  NA_REQUIRE(pts && t && dp && rigidity && g_ctrl_pts_grid && g_rigidity_grid, NA_ENULL, "na_dyn_voxel_warp_backward: null pointer");
  const size_t S3 = (size_t)S * S * S, CH = 3 * (size_t)(n_ctrl - 1);
  int rc;
  long long* fix = det_begin(S3 * (CH + 1), (hipStream_t)stream, "na_dyn_voxel_warp_backward", &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
#define NA_DV_BWD(NC)                                                                                                                        \
  hipLaunchKernelGGL(dyn_voxel_warp_backward_kernel<NC>, dim3(grid_for(N, 256, DV_WG)), dim3(256), 0, (hipStream_t)stream, pts, t, N, g, dp, \
                     rigidity, g_warped, g_dp, g_rigidity, g_ctrl_pts_grid, g_rigidity_grid, fix)
  NA_DV_DISPATCH(n_ctrl, NA_DV_BWD)
#undef NA_DV_BWD
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3 * CH, g_ctrl_pts_grid, (hipStream_t)stream, "na_dyn_voxel_warp_backward")) return rc2;
    return det_finish(fix + S3 * CH, S3, g_rigidity_grid, (hipStream_t)stream, "na_dyn_voxel_warp_backward");
  }
  return check_launch("na_dyn_voxel_warp_backward");
}

}  // extern "C"
