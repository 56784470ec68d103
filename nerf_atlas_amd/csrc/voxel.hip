// NeRFVoxel (src/nerf.py:401-524): a dense S^3 grid of density and colour parameters read by the reference's 8-neighbour lookup
// (grid_coords_trilin_weights, src/nerf.py:493-515).  Four operators: the gather (na_voxel_sample), its scatter-add backward
// (na_voxel_sample_backward), its gradient w.r.t. explicit positions (na_voxel_sample_backward_pts) and the eval route as one launch (na_voxel_render: positions -> gather -> activation -> compositing).
//
// The lookup is NOT a textbook trilinear interpolation and is reproduced, not improved:
//   neighbours  p -+ voxel_len / 2 per axis, clamped to +-grid_radius; corner u takes + on axis i when bit i of u is set
//   centres     (floor(n / voxel_len + 1e-10) + 0.5) * voxel_len, clamped to +-(grid_radius - voxel_len / 2)
//   xyz         (p - centre of corner 0) / voxel_len, unclamped: a point outside the grid is EXTRAPOLATED with weights that
//               alternate in sign, grow polynomially and still sum to 1
//   ids         floor(centre / voxel_len + 1e-10) + S / 2 -- always inside 0 .. S-1 because the centres were clamped
// The lower and the upper neighbour come from two independent floors, so on the planes p = (k + 0.5) voxel_len one ulp decides
// between the pairs (k, k+1), (k+1, k+2) and (k, k+2): cell membership is part of the operator's definition and every operation
// up to and including xyz is the reference's fp32 operation in the reference's order (this unit is built with -ffp-contract=off
// and hipcc's correctly rounded division; tests/voxel_ref.py restates the chain in fp32 torch and the g23 fixtures pin it).
// The kernels are voxel_plv.h's templates at K = -1 (no basis, no sh output, rows of 3 floats, no linear scale); this unit has the entry
// points of the RGB head.
#include "voxel_plv.h"

using namespace na;

extern "C" {

int na_voxel_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, float* raw, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_sample: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_sample", S, C, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(densities && rgb && raw && (pts || (rays && ts)), NA_ENULL, "na_voxel_sample: null pointer");
  hipLaunchKernelGGL(plv_sample_kernel<-1>, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts, R, N,
                     vox_grid(S, grid_radius), densities, rgb, raw, nullptr);
  return check_launch("na_voxel_sample");
}

int na_voxel_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                             double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_sample_backward: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_sample_backward", S, C, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(g_raw && g_densities && g_rgb && (pts || (rays && ts)), NA_ENULL, "na_voxel_sample_backward: null pointer");
  int rc;
  const size_t S3 = (size_t)S * S * S;
  long long* fix = det_begin(S3 * 4, (hipStream_t)stream, "na_voxel_sample_backward", &rc);
  if (rc != NA_OK) return rc;
  plv_launch_backward<-1, 2>(grid_for(N, 256, DV_WG), (hipStream_t)stream, pts, rays, ts, R, N, vox_grid(S, grid_radius), g_raw, nullptr,
                             g_densities, g_rgb, fix);
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3, g_densities, (hipStream_t)stream, "na_voxel_sample_backward")) return rc2;
    return det_finish(fix + S3, S3 * 3, g_rgb, (hipStream_t)stream, "na_voxel_sample_backward");
  }
  return check_launch("na_voxel_sample_backward");
}

int na_voxel_sample_backward_pts(const float* pts, int64_t N, const float* densities, const float* rgb, const float* g_raw, int S, int C,
                                 double grid_radius, float* g_pts, void* stream) {
  NA_REQUIRE(N >= 0, NA_EINVAL, "na_voxel_sample_backward_pts: bad shape N=%lld", (long long)N);
  if (int rc = vox_check_grid("na_voxel_sample_backward_pts", S, C, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts && densities && rgb && g_raw && g_pts, NA_ENULL, "na_voxel_sample_backward_pts: null pointer");
  hipLaunchKernelGGL(plv_backward_pts_kernel<-1>, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, nullptr, 1, N,
                     vox_grid(S, grid_radius), densities, rgb, g_raw, nullptr, g_pts);
  return check_launch("na_voxel_sample_backward_pts");
}

int na_voxel_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                    void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_render: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_render", S, C, grid_radius)) return rc;
  NA_REQUIRE(act_kind >= NA_SIG_NORMAL && act_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "na_voxel_render: activation kind %d", act_kind);
  NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "na_voxel_render: bg kind %d", bg_kind);
  if (R == 0) return NA_OK;
  NA_REQUIRE(rays && ts && densities && rgb && out, NA_ENULL, "na_voxel_render: null pointer");
  hipLaunchKernelGGL(plv_render_kernel<-1>, dim3(grid_for(R, 64)), dim3(64), 0, (hipStream_t)stream, rays, pts, ts, T, R,
                     vox_grid(S, grid_radius), densities, rgb, act_kind, bg_kind, alpha, weights, out);
  return check_launch("na_voxel_render");
}

}  // extern "C"
