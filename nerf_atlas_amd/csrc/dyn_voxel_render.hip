// DynamicNeRFVoxel's test-time render as ONE launch (na_dyn_voxel_render): positions -> deformation -> canonical lookup -> activation ->
// compositing -> the depth / accumulation / flow / rigidity maps of runner.py:894-916, all inside one kernel.
// It replaces, for a model without an MLP, the composition
//   na_compute_pts -> na_dyn_voxel_warp (warped, dp, rigidity per sample) -> na_voxel_render(pts = warped) (alpha, weights per sample)
//   -> na_integrate x 4 (weights x ts, weights x [1 .. 1 0], weights x dp * rigidity, weights x rigidity)
// and is bit for bit equal to it: every step calls the device functions those kernels call (voxel_cell.h, dyn_voxel_spline.h, voxel_plv.h, common.h) in
// their order, the running product is plv_render_kernel's, and every map is integrate_kernel's `acc = acc + w * other` in ascending t
// from 0 (this unit is built with -ffp-contract=off like the others).  No per-sample array is written unless alpha / weights are asked for.
//
// Decomposition.  Everything in a step but the running product and the sums is independent of the walk, and it is nearly all of the work:
// two lookups with five correctly rounded divisions per axis each, the spline, four transcendentals.  One thread per ray, as
// plv_render_kernel walks, leaves a 64 x 64 test tile with 64 waves for 1024 SIMDs, each issuing 80 steps' arithmetic back to back
// (measured: 0.36 ms a tile, no faster for a quarter of the rays, and FASTER with less look-ahead -- issue-bound, not latency-bound;
// DESIGN.md 3o).  So NA_DVR_LANES lanes share a ray: lane j computes steps t0 + j of a chunk of NA_DVR_LANES steps to the point where
// the walk needs them -- alpha, the three activated colours, dp * rigidity, rigidity -- and parks the eight floats in LDS; then ONE lane
// per ray walks the chunk in ascending t with plv_render_kernel's step and integrate_kernel's sums, every operation in their order.
// The gathers of a whole chunk are in flight ahead of the dependent updates (plv_render_kernel's habit, NA_DVR_LANES steps deep), a
// tile is 1024 waves, and the walk itself is 80 x ~20 instructions.  NA_DVR_LANES and NA_DVR_BLOCK are build-time constants; DESIGN.md 3o
// has the times of the other values.
//
// The canonical model's head is a template parameter (K), as in voxel_plv.h's kernels: -1 the per-voxel RGB head (na_dyn_voxel_render,
// C = 3), 0 .. 4 the pos-linear-view head of that order (na_dyn_voxel_plv_render, C = 3 + (K+1)^2: the ray's basis once per thread and
// the linear scale).  Lookup, alpha and the walk are plv_render_kernel<K>'s own functions (vox_gather<K>, vox_alpha, VoxWalk), so the
// result equals the composition over na_voxel_render / na_voxel_plv_render bit for bit; the deformation is na_dyn_voxel_warp's
// (dv_gather, dv_spline).  The tag SH is voxel_plv.h's: the per-voxel spherical-harmonic colour head (na_dyn_voxel_sh_render,
// C = 3 (K+1)^2; the step of na_voxel_sh_render: no linear scale).
#include "dyn_voxel_spline.h"
#include "voxel_plv.h"

namespace na {

#ifndef NA_DVR_LANES
#define NA_DVR_LANES 16   // lanes (steps of a chunk) per ray; a power of two <= 64
#endif
#ifndef NA_DVR_BLOCK
#define NA_DVR_BLOCK 64   // threads of a workgroup: NA_DVR_BLOCK / NA_DVR_LANES rays (one wave: its barriers cost nothing)
#endif
static_assert(NA_DVR_BLOCK % NA_DVR_LANES == 0 && (NA_DVR_LANES & (NA_DVR_LANES - 1)) == 0 && NA_DVR_LANES <= 64, "whole rays per workgroup");

// the optional outputs (NULL: not written)
struct DvrMaps {
  float* depth;     // [R]
  float* acc;       // [R]
  float* flow;      // [R,3]
  float* rigidity;  // [R]
  float* alpha;     // [T,R]
  float* weights;   // [T,R]
};

template <int NC, int K, bool SH = false>
__global__ __launch_bounds__(NA_DVR_BLOCK) void dyn_voxel_render_kernel(const float* __restrict__ rays, const float* __restrict__ t_ray,
                                                                        const float* __restrict__ ts, int T, int64_t R, VoxGrid g,
                                                                        const float* __restrict__ den, const float* __restrict__ rgb,
                                                                        const float* __restrict__ ctrl, const float* __restrict__ rig,
                                                                        int act_kind, int bg_kind, float* __restrict__ out, DvrMaps m) {
  constexpr int CH = 3 * (NC - 1), L = NA_DVR_LANES, RPB = NA_DVR_BLOCK / NA_DVR_LANES;
  // a step as the walk needs it: [alpha | 3 activated colours | 3 of dp * rigidity | rigidity]
  __shared__ float4 park[RPB][L][2];
  const int slot = threadIdx.x / L, j = threadIdx.x % L;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < R; base += (int64_t)gridDim.x * RPB) {  // (uniform: every thread meets the barriers)
    const int64_t r = base + slot;
    const bool live = r < R;
    const int64_t rr = live ? r : R - 1;  // (a dead slot computes the last ray again and writes nothing)
    const float* ry = rays + rr * 6 + 3;
    const float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
    const float time = t_ray[rr];
    float Y[SH_MAX_K];
    plv_ray_basis<K>(rays, rr, Y);
    VoxWalk walk;
    float depth = 0.f, accm = 0.f, fl0 = 0.f, fl1 = 0.f, fl2 = 0.f, rigm = 0.f;
    for (int t0 = 0; t0 < T; t0 += L) {
      const int t = t0 + j;
      if (t < T) {
        // the deformation (na_dyn_voxel_warp's arithmetic) at o + t d ...
        float px, py, pz;
        vox_position(nullptr, rays, ts, R, (int64_t)t * R + rr, px, py, pz);
        const VoxCell c = vox_cell(px, py, pz, g);
        float cp[CH], rl, dp[3], rdp[3], raw[5];
        dv_gather<NC, true, false, true>(c, g, ctrl, rig, nullptr, cp, &rl, nullptr, nullptr);
        dv_spline<NC>(cp, time, dp);
        const float rg = sigmoidf_(rl);
#pragma unroll
        for (int a = 0; a < 3; ++a) rdp[a] = dp[a] * rg;  // (rigid_dp: the product formed first, once)
        // ... the canonical lookup at the warped point, and plv_render_kernel's step up to the running product
        vox_gather<K, SH>(px + rdp[0], py + rdp[1], pz + rdp[2], g, den, rgb, Y, raw);
        const float a = vox_alpha(raw[0], ts, t, T, nrm);
        if (live && m.alpha != nullptr) m.alpha[(int64_t)t * R + r] = a;
        const float3 col = vox_colour<K, SH>(raw, act_kind);
        park[slot][j][0] = make_float4(a, col.x, col.y, col.z);
        park[slot][j][1] = make_float4(rdp[0], rdp[1], rdp[2], rg);
      }
      __syncthreads();
      if (j == 0 && live) {
        // the dependent updates, in ascending t: plv_render_kernel's, then integrate_kernel's `acc = acc + w * other` for the four maps
        const int n = T - t0 < L ? T - t0 : L;
        for (int u = 0; u < n; ++u) {
          const int tu = t0 + u;
          const float4 p0 = park[slot][u][0], p1 = park[slot][u][1];
          const float w = walk.step(p0.x, p0.y, p0.z, p0.w, tu == T - 1);
          if (m.weights != nullptr) m.weights[(int64_t)tu * R + r] = w;
          depth = depth + w * ts[tu];
          accm = accm + w * (tu < T - 1 ? 1.0f : 0.0f);  // (the product with 0 is kept: a NaN weight stays a NaN map)
          fl0 = fl0 + w * p1.x;
          fl1 = fl1 + w * p1.y;
          fl2 = fl2 + w * p1.z;
          rigm = rigm + w * p1.w;
        }
      }
      __syncthreads();  // (the next chunk overwrites the parked steps)
    }
    if (j == 0 && live) {
      walk.finish(bg_kind, out + r * 3);
      if (m.depth != nullptr) m.depth[r] = depth;
      if (m.acc != nullptr) m.acc[r] = accm;
      if (m.flow != nullptr) { m.flow[r * 3] = fl0; m.flow[r * 3 + 1] = fl1; m.flow[r * 3 + 2] = fl2; }
      if (m.rigidity != nullptr) m.rigidity[r] = rigm;
    }
  }
}

}  // namespace na

using namespace na;

// every entry point ends here, its shape and n_ctrl checked: the head's grid check (C as VoxHead::check reads it), the checks common to all, the launch
static int dyn_voxel_render_any(const char* who, VoxHead h, int C, const float* rays, const float* t_ray, int64_t R, const float* ts, int T,
                                const float* densities, const float* rgb, const float* ctrl_pts_grid, const float* rigidity_grid, int S,
                                int n_ctrl, double grid_radius, int act_kind, int bg_kind, float* out, float* depth, float* acc,
                                float* flow, float* rigidity_map, float* alpha, float* weights, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  NA_REQUIRE(n_ctrl >= 2 && n_ctrl <= 11, NA_EUNSUPPORTED, "%s: n_ctrl %d (2 .. 11 control points: 3 (n - 1) <= 32 channels per voxel)", who, n_ctrl);
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  if (int rc = vox_check_kinds(who, act_kind, bg_kind)) return rc;
  if (R == 0) return NA_OK;
#define NA_DVR_PTR(p) NA_REQUIRE(p != nullptr, NA_ENULL, "%s: null pointer " #p, who)
  NA_DVR_PTR(rays); NA_DVR_PTR(t_ray); NA_DVR_PTR(ts); NA_DVR_PTR(densities); NA_DVR_PTR(rgb); NA_DVR_PTR(ctrl_pts_grid);
  NA_DVR_PTR(rigidity_grid); NA_DVR_PTR(out);
#undef NA_DVR_PTR
  NA_REQUIRE(h.rgb_aligned(rgb), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, h.order);
  const VoxGrid g = vox_grid(S, grid_radius);
  const DvrMaps m{depth, acc, flow, rigidity_map, alpha, weights};
  vox_for_head(h, [&](auto k, auto tag) {
#define NA_DVR_NC(NC)                                                                                                                     \
  hipLaunchKernelGGL((dyn_voxel_render_kernel<NC, decltype(k)::value, decltype(tag)::value>), dim3(grid_for(R, NA_DVR_BLOCK / NA_DVR_LANES)), \
                     dim3(NA_DVR_BLOCK), 0, (hipStream_t)stream, rays, t_ray, ts, T, R, g, densities, rgb, ctrl_pts_grid, rigidity_grid,  \
                     act_kind, bg_kind, out, m)
    NA_DV_DISPATCH(n_ctrl, NA_DVR_NC)
#undef NA_DVR_NC
  });
  return check_launch(who);
}

extern "C" {

int na_dyn_voxel_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        const float* ctrl_pts_grid, const float* rigidity_grid, int S, int C, int n_ctrl, double grid_radius, int act_kind,
                        int bg_kind, float* out, float* depth, float* acc, float* flow, float* rigidity_map, float* alpha, float* weights,
                        void* stream) {
  return dyn_voxel_render_any("na_dyn_voxel_render", {NA_VOX_HEAD_RGB, -1}, C, rays, t_ray, R, ts, T, densities, rgb, ctrl_pts_grid, rigidity_grid,
                              S, n_ctrl, grid_radius, act_kind, bg_kind, out, depth, acc, flow, rigidity_map, alpha, weights, stream);
}

int na_dyn_voxel_plv_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities,
                            const float* rgb, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int order, int n_ctrl,
                            double grid_radius, int act_kind, int bg_kind, float* out, float* depth, float* acc, float* flow,
                            float* rigidity_map, float* alpha, float* weights, void* stream) {
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return dyn_voxel_render_any("na_dyn_voxel_plv_render", h, h.row_floats(), rays, t_ray, R, ts, T, densities, rgb, ctrl_pts_grid, rigidity_grid, S,
                              n_ctrl, grid_radius, act_kind, bg_kind, out, depth, acc, flow, rigidity_map, alpha, weights, stream);
}

int na_dyn_voxel_sh_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities,
                           const float* rgb, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int C, int order, int n_ctrl,
                           double grid_radius, int act_kind, int bg_kind, float* out, float* depth, float* acc, float* flow,
                           float* rigidity_map, float* alpha, float* weights, void* stream) {
  return dyn_voxel_render_any("na_dyn_voxel_sh_render", {NA_VOX_HEAD_SH, order}, C, rays, t_ray, R, ts, T, densities, rgb, ctrl_pts_grid,
                              rigidity_grid, S, n_ctrl, grid_radius, act_kind, bg_kind, out, depth, acc, flow, rigidity_map, alpha, weights, stream);
}

}  // extern "C"
