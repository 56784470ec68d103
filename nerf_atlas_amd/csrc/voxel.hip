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
//
// This unit has the entry points of the four operators for all three colour heads; the kernels are voxel_plv.h's templates <K, SH>
// and every entry point is a forwarder that names its head (VoxHead, voxel_head.h) to ONE implementation per operator:
//   na_voxel_*      the per-voxel RGB head, K = -1: no basis, no sh output, rows of 3 floats, no linear scale
//   na_voxel_plv_*  the pos-linear-view head (src/refl.py:265-280), K = order: rows [raw rgb (3) | (K+1)^2 coefficients],
//                   raw [N, 4] and sh [N] = s; the scatter adds w_u [g_raw | g_sh Y_k]
//   na_voxel_sh_*   the spherical-harmonic colour head (src/refl.py:715-722), K = order under the tag SH: rows of 3 channel
//                   blocks of (K+1)^2 coefficients, raw [N, 4] = [density | s_r s_g s_b]; the scatter adds w_u [g_raw[n, 0] | (w_u
//                   g_raw[n, 1 + c]) Y_k].  C does not identify the head (3 is the RGB head's count, 12 the pos-linear-view head's at
//                   K = 2): these entry points take C and the order.
// K is a template parameter: every loop over the coefficients unrolls and the basis stays in VGPRs.  The ray of sample n is n % R.
// The only fused operations are the explicit fmaf of plv_contract / sh_contract_row.
#include "voxel_plv.h"

// the scatter variant na_voxel_plv_sample_backward runs (voxel_plv.h: 1 whole rows in the LDS table, 2 leading sums only)
#ifndef NA_PLV_SCATTER
#define NA_PLV_SCATTER 1
#endif
// the scatter variant na_voxel_sh_sample_backward runs in each mode (voxel_plv.h: 1 whole rows in the LDS table, 2 a pass per channel)
#ifndef NA_SH_SCATTER
#define NA_SH_SCATTER 2
#endif
#ifndef NA_SH_SCATTER_DET
#define NA_SH_SCATTER_DET 2
#endif

using namespace na;

// the positions of a lookup: explicit pts, or rays x ts; a view-dependent head reads the rays' directions in both forms
static int vox_check_positions(const char* who, const VoxHead& h, const float* pts, const float* rays, const float* ts) {
  if (!h.view()) {
    NA_REQUIRE(pts || (rays && ts), NA_ENULL, "%s: needs pts, or rays and ts", who);
    return NA_OK;
  }
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(pts || ts, NA_ENULL, "%s: pts and ts are both null", who);
  return NA_OK;
}

// sh: the pos-linear-view head's second output [N] (not read otherwise).  The alignment of raw / g_raw is an argument check of the two
// view-dependent heads' entry points only, here and in the two backwards: the RGB head's never had it and keep their codes.
static int vox_sample(const char* who, VoxHead h, const float* pts, const float* rays, int64_t R, const float* ts, int T,
                      const float* densities, const float* rgb, int S, int C, double grid_radius, float* raw, float* sh, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  if (int rc = vox_check_positions(who, h, pts, rays, ts)) return rc;
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(raw, NA_ENULL, "%s: raw is null", who);
  NA_REQUIRE(h.kind != NA_VOX_HEAD_PLV || sh, NA_ENULL, "%s: sh is null", who);
  NA_REQUIRE(!h.view() || aligned16(raw), NA_EINVAL, "%s: raw must be 16-byte aligned", who);
  NA_REQUIRE(h.rgb_aligned(rgb), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, h.order);
  const VoxGrid g = vox_grid(S, grid_radius);
  vox_for_head(h, [&](auto k, auto tag) {
    hipLaunchKernelGGL((plv_sample_kernel<decltype(k)::value, decltype(tag)::value>), dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream,
                       pts, rays, ts, R, N, g, densities, rgb, raw, sh);
  });
  return check_launch(who);
}

// variant: the scatter geometry of a view-dependent head (voxel_plv.h); the RGB head has one (the leading sums ARE its row)
static int vox_sample_backward(const char* who, VoxHead h, const float* pts, const float* rays, int64_t R, const float* ts, int T,
                               const float* g_raw, const float* g_sh, int S, int C, double grid_radius, float* g_densities, float* g_rgb,
                               int variant, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  NA_REQUIRE(variant == 1 || variant == 2, NA_EINVAL, "%s: scatter variant %d (1: whole rows in LDS, 2: %s)", who, variant,
             h.kind == NA_VOX_HEAD_SH ? "a pass per colour channel" : "leading sums in LDS");
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  if (int rc = vox_check_positions(who, h, pts, rays, ts)) return rc;
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(h.kind != NA_VOX_HEAD_PLV || g_sh, NA_ENULL, "%s: g_sh is null", who);
  NA_REQUIRE(g_densities, NA_ENULL, "%s: g_densities is null", who);
  NA_REQUIRE(g_rgb, NA_ENULL, "%s: g_rgb is null", who);
  NA_REQUIRE(!h.view() || aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  const size_t S3 = (size_t)S * S * S, Cn = (size_t)h.row_floats();
  hipStream_t s = (hipStream_t)stream;
  int rc;
  long long* fix = det_begin(S3 * (1 + Cn), s, who, &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
  const unsigned wg = grid_for(N, 256, DV_WG);
  vox_for_head(h, [&](auto k, auto tag) {
    constexpr int K = decltype(k)::value;
    if constexpr (K < 0) {
      plv_launch_backward<-1, 2>(wg, s, pts, rays, ts, R, N, g, g_raw, nullptr, g_densities, g_rgb, fix);
    } else if constexpr (decltype(tag)::value) {
      if (variant == 1) sh_launch_backward<K, 1>(wg, s, pts, rays, ts, R, N, g, g_raw, g_densities, g_rgb, fix);
      else sh_launch_backward<K, 2>(wg, s, pts, rays, ts, R, N, g, g_raw, g_densities, g_rgb, fix);
    } else {
      if (variant == 1) plv_launch_backward<K, 1>(wg, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_densities, g_rgb, fix);
      else plv_launch_backward<K, 2>(wg, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_densities, g_rgb, fix);
    }
  });
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3, g_densities, s, who)) return rc2;
    return det_finish(fix + S3, S3 * Cn, g_rgb, s, who);
  }
  return check_launch(who);
}

// the ray of sample n is n % R (the RGB head reads no ray: its forwarder passes R = 1)
static int vox_sample_backward_pts(const char* who, VoxHead h, const float* pts, const float* rays, int64_t R, int64_t N,
                                   const float* densities, const float* rgb, const float* g_raw, const float* g_sh, int S, int C,
                                   double grid_radius, float* g_pts, void* stream) {
  NA_REQUIRE(N >= 0 && R >= 0 && (N == 0 || (R >= 1 && N % R == 0)), NA_EINVAL, "%s: bad shape N=%lld R=%lld", who, (long long)N, (long long)R);
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts, NA_ENULL, "%s: pts is null", who);
  NA_REQUIRE(!h.view() || rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(h.kind != NA_VOX_HEAD_PLV || g_sh, NA_ENULL, "%s: g_sh is null", who);
  NA_REQUIRE(g_pts, NA_ENULL, "%s: g_pts is null", who);
  NA_REQUIRE(!h.view() || aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  NA_REQUIRE(h.rgb_aligned(rgb), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, h.order);
  const VoxGrid g = vox_grid(S, grid_radius);
  vox_for_head(h, [&](auto k, auto tag) {
    hipLaunchKernelGGL((plv_backward_pts_kernel<decltype(k)::value, decltype(tag)::value>), dim3(grid_for(N, 256)), dim3(256), 0,
                       (hipStream_t)stream, pts, rays, R, N, g, densities, rgb, g_raw, g_sh, g_pts);
  });
  return check_launch(who);
}

static int vox_render(const char* who, VoxHead h, const float* rays, const float* pts, int64_t R, const float* ts, int T,
                      const float* densities, const float* rgb, int S, int C, double grid_radius, int act_kind, int bg_kind, float* alpha,
                      float* weights, float* out, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  if (int rc = vox_check_kinds(who, act_kind, bg_kind)) return rc;
  if (R == 0) return NA_OK;
  if (int rc = vox_check_render_ptrs(who, h, rays, ts, "ts", densities, rgb, out)) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
  vox_for_head(h, [&](auto k, auto tag) {
    hipLaunchKernelGGL((plv_render_kernel<decltype(k)::value, decltype(tag)::value>), dim3(grid_for(R, 64)), dim3(64), 0, (hipStream_t)stream,
                       rays, pts, ts, T, R, g, densities, rgb, act_kind, bg_kind, alpha, weights, out);
  });
  return check_launch(who);
}

extern "C" {

// ------------------------------------------------------------------------------------ the RGB head
int na_voxel_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, float* raw, void* stream) {
  return vox_sample("na_voxel_sample", {NA_VOX_HEAD_RGB, -1}, pts, rays, R, ts, T, densities, rgb, S, C, grid_radius, raw, nullptr, stream);
}

int na_voxel_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                             double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  return vox_sample_backward("na_voxel_sample_backward", {NA_VOX_HEAD_RGB, -1}, pts, rays, R, ts, T, g_raw, nullptr, S, C, grid_radius,
                             g_densities, g_rgb, 2, stream);
}

int na_voxel_sample_backward_pts(const float* pts, int64_t N, const float* densities, const float* rgb, const float* g_raw, int S, int C,
                                 double grid_radius, float* g_pts, void* stream) {
  return vox_sample_backward_pts("na_voxel_sample_backward_pts", {NA_VOX_HEAD_RGB, -1}, pts, nullptr, 1, N, densities, rgb, g_raw, nullptr, S,
                                 C, grid_radius, g_pts, stream);
}

int na_voxel_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                    void* stream) {
  return vox_render("na_voxel_render", {NA_VOX_HEAD_RGB, -1}, rays, pts, R, ts, T, densities, rgb, S, C, grid_radius, act_kind, bg_kind, alpha,
                    weights, out, stream);
}

// ------------------------------------------------------------------------------------ the pos-linear-view head
int na_voxel_plv_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, float* raw, float* sh, void* stream) {
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return vox_sample("na_voxel_plv_sample", h, pts, rays, R, ts, T, densities, rgb, S, h.row_floats(), grid_radius, raw, sh, stream);
}

int na_voxel_plv_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                         const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb,
                                         int variant, void* stream) {
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return vox_sample_backward("na_voxel_plv_sample_backward", h, pts, rays, R, ts, T, g_raw, g_sh, S, h.row_floats(), grid_radius, g_densities,
                             g_rgb, variant, stream);
}

int na_voxel_plv_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                 const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  return na_voxel_plv_sample_backward_variant(pts, rays, R, ts, T, g_raw, g_sh, S, order, grid_radius, g_densities, g_rgb, NA_PLV_SCATTER,
                                              stream);
}

int na_voxel_plv_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                     const float* g_raw, const float* g_sh, int S, int order, double grid_radius, float* g_pts,
                                     void* stream) {
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return vox_sample_backward_pts("na_voxel_plv_sample_backward_pts", h, pts, rays, R, N, densities, rgb, g_raw, g_sh, S, h.row_floats(),
                                 grid_radius, g_pts, stream);
}

int na_voxel_plv_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                        void* stream) {
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return vox_render("na_voxel_plv_render", h, rays, pts, R, ts, T, densities, rgb, S, h.row_floats(), grid_radius, act_kind, bg_kind, alpha,
                    weights, out, stream);
}

// ------------------------------------------------------------------------------------ the spherical-harmonic head
int na_voxel_sh_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, float* raw, void* stream) {
  return vox_sample("na_voxel_sh_sample", {NA_VOX_HEAD_SH, order}, pts, rays, R, ts, T, densities, rgb, S, C, grid_radius, raw, nullptr, stream);
}

int na_voxel_sh_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S,
                                        int C, int order, double grid_radius, float* g_densities, float* g_rgb, int variant, void* stream) {
  return vox_sample_backward("na_voxel_sh_sample_backward", {NA_VOX_HEAD_SH, order}, pts, rays, R, ts, T, g_raw, nullptr, S, C, grid_radius,
                             g_densities, g_rgb, variant, stream);
}

int na_voxel_sh_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                                int order, double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  const int variant = det_workspace().ptr != nullptr ? NA_SH_SCATTER_DET : NA_SH_SCATTER;
  return na_voxel_sh_sample_backward_variant(pts, rays, R, ts, T, g_raw, S, C, order, grid_radius, g_densities, g_rgb, variant, stream);
}

int na_voxel_sh_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                    const float* g_raw, int S, int C, int order, double grid_radius, float* g_pts, void* stream) {
  return vox_sample_backward_pts("na_voxel_sh_sample_backward_pts", {NA_VOX_HEAD_SH, order}, pts, rays, R, N, densities, rgb, g_raw, nullptr, S,
                                 C, grid_radius, g_pts, stream);
}

int na_voxel_sh_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                       void* stream) {
  return vox_render("na_voxel_sh_render", {NA_VOX_HEAD_SH, order}, rays, pts, R, ts, T, densities, rgb, S, C, grid_radius, act_kind, bg_kind,
                    alpha, weights, out, stream);
}

}  // extern "C"
