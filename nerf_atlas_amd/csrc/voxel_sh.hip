// NeRFVoxel with the per-voxel spherical-harmonic colour head (SphericalHarmonic.to_voxel, src/refl.py:715-722): the grid
// row is 3 channel blocks of (K+1)^2 coefficients, C = 3 (K+1)^2 with coefficient k of channel c at c (K+1)^2 + k, and a sample's colour
// is act(s_c), s_c = sum_u w_u sum_k Y_k(normalize(view)) row_u[c (K+1)^2 + k].  The entry points of four operators; their kernels are
// voxel_plv.h's templates under the tag SH at K = order (the lookup, cells and weights of the other two heads; each channel block
// contracted with the ray's basis as it arrives), and its sh_backward_kernel:
//   na_voxel_sh_sample               raw [N, 4] = [density | s_r s_g s_b]: the RGB head's layout
//   na_voxel_sh_sample_backward      scatter-add of w_u [g_raw[n, 0] | (w_u g_raw[n, 1 + c]) Y_k] into the two grids
//   na_voxel_sh_sample_backward_pts  the gradient w.r.t. explicit positions (a gather)
//   na_voxel_sh_render               the eval route as one launch: basis once per ray, lookup, activation, compositing
// C does not identify the head (3 is the RGB head's count, 12 the pos-linear-view head's at K = 2): every entry point takes the order.
// Built like voxel.hip (-ffp-contract=off; the only fused operations are the explicit fmaf of sh_contract_row).
#include "voxel_plv.h"

// the scatter variant na_voxel_sh_sample_backward runs in each mode (voxel_plv.h: 1 whole rows in the LDS table, 2 a pass per channel)
#ifndef NA_SH_SCATTER
#define NA_SH_SCATTER 2
#endif
#ifndef NA_SH_SCATTER_DET
#define NA_SH_SCATTER_DET 2
#endif

using namespace na;

// `order` was checked (0 .. 4): expands the statement once with K bound to it
#define NA_SH_ORDER(order, ...)                           \
  switch (order) {                                        \
    case 0: { constexpr int K = 0; __VA_ARGS__; } break;  \
    case 1: { constexpr int K = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int K = 2; __VA_ARGS__; } break;  \
    case 3: { constexpr int K = 3; __VA_ARGS__; } break;  \
    default: { constexpr int K = 4; __VA_ARGS__; } break; \
  }

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// rows of 4 C bytes are read with 16-byte loads when C % 4 == 0 (orders 1 and 3): the grid must then start on a 16-byte boundary
static bool grid_aligned(const float* rgb, int order) { return (3 * (order + 1) * (order + 1)) % 4 != 0 || aligned16(rgb); }

static int sh_check_grid(const char* who, int S, int C, int order, double grid_radius) {
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  NA_REQUIRE(C == 3 * (order + 1) * (order + 1), NA_EINVAL, "%s: C = %d, the spherical-harmonic head of order %d holds 3 (order + 1)^2 = %d", who,
             C, order, 3 * (order + 1) * (order + 1));
  return NA_OK;
}

extern "C" {

int na_voxel_sh_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, float* raw, void* stream) {
  const char* who = "na_voxel_sh_sample";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = sh_check_grid(who, S, C, order, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(pts || ts, NA_ENULL, "%s: pts and ts are both null", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(raw, NA_ENULL, "%s: raw is null", who);
  NA_REQUIRE(aligned16(raw), NA_EINVAL, "%s: raw must be 16-byte aligned", who);
  NA_REQUIRE(grid_aligned(rgb, order), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, order);
  const VoxGrid g = vox_grid(S, grid_radius);
  NA_SH_ORDER(order, hipLaunchKernelGGL((plv_sample_kernel<K, true>), dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts,
                                        R, N, g, densities, rgb, raw, nullptr));
  return check_launch(who);
}

int na_voxel_sh_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S,
                                        int C, int order, double grid_radius, float* g_densities, float* g_rgb, int variant, void* stream) {
  const char* who = "na_voxel_sh_sample_backward";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = sh_check_grid(who, S, C, order, grid_radius)) return rc;
  NA_REQUIRE(variant == 1 || variant == 2, NA_EINVAL, "%s: scatter variant %d (1: whole rows in LDS, 2: a pass per colour channel)", who, variant);
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(pts || ts, NA_ENULL, "%s: pts and ts are both null", who);
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(g_densities, NA_ENULL, "%s: g_densities is null", who);
  NA_REQUIRE(g_rgb, NA_ENULL, "%s: g_rgb is null", who);
  NA_REQUIRE(aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  const size_t S3 = (size_t)S * S * S, Cn = (size_t)C;
  int rc;
  long long* fix = det_begin(S3 * (1 + Cn), (hipStream_t)stream, who, &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
  const unsigned wg = grid_for(N, 256, DV_WG);
  NA_SH_ORDER(order, if (variant == 1) sh_launch_backward<K, 1>(wg, (hipStream_t)stream, pts, rays, ts, R, N, g, g_raw, g_densities, g_rgb, fix);
              else sh_launch_backward<K, 2>(wg, (hipStream_t)stream, pts, rays, ts, R, N, g, g_raw, g_densities, g_rgb, fix));
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3, g_densities, (hipStream_t)stream, who)) return rc2;
    return det_finish(fix + S3, S3 * Cn, g_rgb, (hipStream_t)stream, who);
  }
  return check_launch(who);
}

int na_voxel_sh_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                                int order, double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  const int variant = det_workspace().ptr != nullptr ? NA_SH_SCATTER_DET : NA_SH_SCATTER;
  return na_voxel_sh_sample_backward_variant(pts, rays, R, ts, T, g_raw, S, C, order, grid_radius, g_densities, g_rgb, variant, stream);
}

int na_voxel_sh_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                    const float* g_raw, int S, int C, int order, double grid_radius, float* g_pts, void* stream) {
  const char* who = "na_voxel_sh_sample_backward_pts";
  NA_REQUIRE(N >= 0 && R >= 0 && (N == 0 || (R >= 1 && N % R == 0)), NA_EINVAL, "%s: bad shape N=%lld R=%lld", who, (long long)N, (long long)R);
  if (int rc = sh_check_grid(who, S, C, order, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts, NA_ENULL, "%s: pts is null", who);
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(g_pts, NA_ENULL, "%s: g_pts is null", who);
  NA_REQUIRE(aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  NA_REQUIRE(grid_aligned(rgb, order), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, order);
  const VoxGrid g = vox_grid(S, grid_radius);
  NA_SH_ORDER(order, hipLaunchKernelGGL((plv_backward_pts_kernel<K, true>), dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts,
                                        rays, R, N, g, densities, rgb, g_raw, nullptr, g_pts));
  return check_launch(who);
}

int na_voxel_sh_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                       void* stream) {
  const char* who = "na_voxel_sh_render";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = sh_check_grid(who, S, C, order, grid_radius)) return rc;
  NA_REQUIRE(act_kind >= NA_SIG_NORMAL && act_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "%s: activation kind %d", who, act_kind);
  NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "%s: bg kind %d", who, bg_kind);
  if (R == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null", who);
  NA_REQUIRE(ts, NA_ENULL, "%s: ts is null", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(out, NA_ENULL, "%s: out is null", who);
  NA_REQUIRE(grid_aligned(rgb, order), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, order);
  const VoxGrid g = vox_grid(S, grid_radius);
  NA_SH_ORDER(order, hipLaunchKernelGGL((plv_render_kernel<K, true>), dim3(grid_for(R, 64)), dim3(64), 0, (hipStream_t)stream, rays, pts, ts, T,
                                        R, g, densities, rgb, act_kind, bg_kind, alpha, weights, out));
  return check_launch(who);
}

}  // extern "C"
