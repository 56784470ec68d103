// The divergence regularisers of DynamicNeRFVoxel (runner.py:694-700; src/utils.py:461-478): quadratic forms v . (J v) of
// the Jacobian of the deformation w.r.t. the UNWARPED sample position.  Inside the reference's lookup only
//   xyzs = (pts - neighbor_centers[..., 0, :]) / voxel_len
// carries a gradient (floor kills the rest, the clamps sit in front of a floor), so with w_u = wx wy wz the trilinear weights of
// corner u (voxel_cell.h), sx = +1 if u & 1 else -1 (sy, sz likewise) and vl = voxel_len
//   grad w_u  = (sx wy wz, wx sy wz, wx wy sz) / vl
//   J_dp v    = spline_t(sum_u (v . grad w_u) c_{u,k})           (the spline is linear in its control points; control point 0 is zero)
//   J_rigid v = s (J_dp v) + dp s (1 - s) sum_u (v . grad w_u) r_u,    s = sigmoid(sum_u w_u r_u),   dp = spline_t(sum_u w_u c_{u,k})
// Two operators:
//   na_dyn_voxel_jac_quad           out[n] = v . (J v), J = J_dp (rigidity_grid NULL: --dyn-diverge-decay with v = 1) or J_rigid
//                                   (--ffjord-div-decay with v the caller's normal draw).  One launch, one thread per sample; the
//                                   eight rows are read once and the tangent control points sum_u (v . grad w_u) c_{u,k} (and, for
//                                   J_rigid, the control points themselves) stay in registers.
//   na_dyn_voxel_jac_quad_backward  the J_dp form's gradient w.r.t. ctrl_pts_grid: row u, block k, axis a gets
//                                   g[n] (v . grad w_u) B_k(t) v_a, summed by voxel_scatter.h's table.  The J_rigid form has no
//                                   graph in the reference and gets no backward.  There is no gradient w.r.t. pts, t or v.
// ORDER OF THE OPERATIONS (tests/dyn_voxel_div_ref.py derives its bound from it; the unit is built with -ffp-contract=off):
//   d_u = ((v_x gx_u + v_y gy_u) + v_z gz_u) / vl with gx_u = +-(wy wz), gy_u = +-(wx wz), gz_u = +-(wx wy) (dv_tangent over
//   vox_dweight); sums over the corners in corner order, acc <- acc + d_u q (dv_gather's tangent sums, dyn_voxel_spline.h); dv_spline;
//   out = (v_x j_x + v_y j_y) + v_z j_z.
#include "voxel_scatter.h"
#include "dyn_voxel_spline.h"

namespace na {

__device__ __forceinline__ void jq_direction(const float* __restrict__ v, int64_t n, float e[3]) {
  e[0] = e[1] = e[2] = 1.f;
  if (v != nullptr) { e[0] = v[n * 3]; e[1] = v[n * 3 + 1]; e[2] = v[n * 3 + 2]; }
}

// one thread per sample: 8 rows of 3(n-1) floats (+ 8 rigidity logits for RIGID), as dyn_voxel_warp_kernel reads them
template <int NC, bool RIGID>
__global__ __launch_bounds__(256) void dyn_voxel_jac_quad_kernel(const float* __restrict__ pts, const float* __restrict__ t, int64_t N, VoxGrid g,
                                                                 const float* __restrict__ ctrl, const float* __restrict__ rig,
                                                                 const float* __restrict__ v, float* __restrict__ out) {
  constexpr int CH = 3 * (NC - 1);
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    float e[3];
    jq_direction(v, n, e);
    float tcp[CH], cp[RIGID ? CH : 1], rl = 0.f, trl = 0.f;
    dv_gather<NC, RIGID, true, RIGID>(c, g, ctrl, rig, e, cp, &rl, tcp, &trl);
    const float tn = t[n];
    float j[3];
    dv_spline<NC>(tcp, tn, j);
    if (RIGID) {
      float dp[3];
      dv_spline<NC>(cp, tn, dp);
      const float s = sigmoidf_(rl);
      const float ds = (s * (1.f - s)) * trl;
#pragma unroll
      for (int a = 0; a < 3; ++a) j[a] = s * j[a] + dp[a] * ds;
    }
    out[n] = (e[0] * j[0] + e[1] * j[1]) + e[2] * j[2];
  }
}

// corner u of a sample adds (v . grad w_u) g[n] B_k(t) v_a to channel 3(k-1) + a of ctrl row_u: one wide row of W = 3(NC-1) sums per
// grid row on voxel_scatter.h's table (add_row's weight is v . grad w_u)
template <int NC>
__global__ __launch_bounds__(256) void dyn_voxel_jac_quad_backward_kernel(const float* __restrict__ pts, const float* __restrict__ t, int64_t N,
                                                                          VoxGrid g, const float* __restrict__ v, const float* __restrict__ g_up,
                                                                          float* __restrict__ g_ctrl, long long* __restrict__ fix) {
  constexpr int W = 3 * (NC - 1), ROWS = DvTable<W>::ROWS;
  __shared__ uint32_t tags[ROWS];
  __shared__ unsigned long long vals[ROWS * W];
  const DvTable<W> table{tags, vals, fix};
  auto add_global = [&](uint32_t id, int e, float x) { accumulate(g_ctrl, fix, (int64_t)id * W + e, x); };
  table.clear();
  int64_t n_lo, n_hi;
  dv_run(N, n_lo, n_hi);
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    if (n >= n_hi) continue;  // (no barrier inside the loop)
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    float e[3], B[NC], sv[W];
    jq_direction(v, n, e);
    dv_bernstein<NC>(t[n], B);
    const float gn = g_up[n];
#pragma unroll
    for (int k = 1; k < NC; ++k) {
      const float gb = gn * B[k];
#pragma unroll
      for (int a = 0; a < 3; ++a) sv[3 * (k - 1) + a] = gb * e[a];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) table.add_row((uint32_t)vox_row(c, u, g.S), dv_tangent(c, u, e, g.vl), sv, add_global);
  }
  table.flush([&](uint32_t id, int e, unsigned long long x) { table.put(g_ctrl, fix, (int64_t)id * W + e, x); });
}

}  // namespace na

using namespace na;

extern "C" {

int na_dyn_voxel_jac_quad(const float* pts, const float* t, int64_t N, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int n_ctrl,
                          double grid_radius, const float* v, float* out, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_jac_quad", N, S, n_ctrl, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts, NA_ENULL, "na_dyn_voxel_jac_quad: null pointer pts");
  NA_REQUIRE(t, NA_ENULL, "na_dyn_voxel_jac_quad: null pointer t");
  NA_REQUIRE(ctrl_pts_grid, NA_ENULL, "na_dyn_voxel_jac_quad: null pointer ctrl_pts_grid");
  NA_REQUIRE(out, NA_ENULL, "na_dyn_voxel_jac_quad: null pointer out");
  const VoxGrid g = vox_grid(S, grid_radius);
#define NA_JQ_FWD(NC)                                                                                                                         \
  if (rigidity_grid != nullptr)                                                                                                               \
    hipLaunchKernelGGL((dyn_voxel_jac_quad_kernel<NC, true>), dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, t, N, g,         \
                       ctrl_pts_grid, rigidity_grid, v, out);                                                                                 \
  else                                                                                                                                        \
    hipLaunchKernelGGL((dyn_voxel_jac_quad_kernel<NC, false>), dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, t, N, g,        \
                       ctrl_pts_grid, rigidity_grid, v, out)
  NA_DV_DISPATCH(n_ctrl, NA_JQ_FWD)
#undef NA_JQ_FWD
  return check_launch("na_dyn_voxel_jac_quad");
}

int na_dyn_voxel_jac_quad_backward(const float* pts, const float* t, int64_t N, int S, int n_ctrl, double grid_radius, const float* v,
                                   const float* g, float* g_ctrl_pts_grid, void* stream) {
  if (int rc = dv_check("na_dyn_voxel_jac_quad_backward", N, S, n_ctrl, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts, NA_ENULL, "na_dyn_voxel_jac_quad_backward: null pointer pts");
  NA_REQUIRE(t, NA_ENULL, "na_dyn_voxel_jac_quad_backward: null pointer t");
  NA_REQUIRE(g, NA_ENULL, "na_dyn_voxel_jac_quad_backward: null pointer g");
  NA_REQUIRE(g_ctrl_pts_grid, NA_ENULL, "na_dyn_voxel_jac_quad_backward: null pointer g_ctrl_pts_grid");
  const size_t total = (size_t)S * S * S * 3 * (size_t)(n_ctrl - 1);
  int rc;
  long long* fix = det_begin(total, (hipStream_t)stream, "na_dyn_voxel_jac_quad_backward", &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid vg = vox_grid(S, grid_radius);
#define NA_JQ_BWD(NC)                                                                                                                      \
  hipLaunchKernelGGL(dyn_voxel_jac_quad_backward_kernel<NC>, dim3(grid_for(N, 256, DV_WG)), dim3(256), 0, (hipStream_t)stream, pts, t, N, \
                     vg, v, g, g_ctrl_pts_grid, fix)
  NA_DV_DISPATCH(n_ctrl, NA_JQ_BWD)
#undef NA_JQ_BWD
  if (fix != nullptr) return det_finish(fix, total, g_ctrl_pts_grid, (hipStream_t)stream, "na_dyn_voxel_jac_quad_backward");
  return check_launch("na_dyn_voxel_jac_quad_backward");
}

}  // extern "C"
