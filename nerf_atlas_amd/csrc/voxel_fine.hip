// NeRFVoxel coarse -> fine (`--voxel-steps-fine`): the two kernels that na_resample_ts sits between.
//   na_voxel_proposal             alpha / weights [T,R] of the shared steps from the DENSITY grid alone: 8 floats gathered per step where
//                                 the renderers gather 8 rows of up to 75.  Bit for bit the alpha / weights of na_voxel_render /
//                                 na_voxel_plv_render / na_voxel_sh_render (the colours do not enter them).
//   na_voxel_render_rayts         the three one-launch renderers over PER-RAY steps ts_ray [R,M] (`merged` of na_resample_ts):
//   na_voxel_plv_render_rayts     positions o + t d, lookup of both grids, head, activation, compositing.  Rows that all equal one shared
//   na_voxel_sh_render_rayts      row give the shared-step renderer's out, alpha and weights bit for bit.
// ONE kernel template: the proposal is the renderer with every ray reading the same row (row stride 0) and no colour.  Every step
// calls what plv_render_kernel calls, in its order -- vox_cell / vox_weight / vox_gather (voxel_cell.h, voxel_plv.h), vox_alpha on the
// ray's OWN row (difference, clamp at 1e-5, 1e10 at the last step, times |d|: the expressions it applies to a shared row), VoxWalk --
// and this unit is built with -ffp-contract=off like the others.  The density-only lookup is vox_gather's v[0]: the same cell, the
// same weights, `v = v + w den[row]` in corner order from 0.
//
// Decomposition (dyn_voxel_render.hip's, which measured it: a thread per ray leaves a 64 x 64 tile with 64 waves and is issue-bound).
// L lanes share a ray: lane j computes step t0 + j of a chunk of L steps up to the point where the walk needs it -- alpha and the three
// activated colours -- and parks the four floats in LDS; then ONE lane per ray walks the chunk in ascending t.  The gathers of a whole
// chunk are in flight ahead of the dependent updates and a tile is L times the waves.  L is a template parameter: VFR_LANES is the
// shipped value, na_voxel_fine_lanes runs any other (tools/voxel_fine_bench.py; DESIGN.md 3v has the times).
#include "voxel_plv.h"

namespace na {

constexpr int VFR_BLOCK = 64;  // threads of a workgroup: VFR_BLOCK / L rays (one wave: its barriers cost nothing)

// v[0] of vox_gather: the density channel alone
__device__ __forceinline__ float vox_gather_density(float px, float py, float pz, const VoxGrid& g, const float* __restrict__ den) {
  const VoxCell c = vox_cell(px, py, pz, g);
  float v = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) v = v + vox_weight(c, u) * den[vox_row(c, u, g.S)];
  return v;
}

// PROP: the proposal (density grid only, no colour, no out).  `stride`: floats between two rays' rows of ts_ray (0: one shared row).
template <int K, bool SH, bool PROP, int L>
__global__ __launch_bounds__(VFR_BLOCK) void voxel_fine_kernel(const float* __restrict__ rays, const float* __restrict__ ts_ray, int64_t stride,
                                                               int M, int64_t R, VoxGrid g, const float* __restrict__ den,
                                                               const float* __restrict__ rgb, int act_kind, int bg_kind,
                                                               float* __restrict__ alpha_out, float* __restrict__ weights_out,
                                                               float* __restrict__ out) {
  constexpr int RPB = VFR_BLOCK / L;
  __shared__ float4 park[RPB][L];  // a step as the walk needs it: [alpha | 3 activated colours]
  const int slot = threadIdx.x / L, j = threadIdx.x % L;
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < R; base += (int64_t)gridDim.x * RPB) {  // (uniform: every thread meets the barriers)
    const int64_t r = base + slot;
    const bool live = r < R;
    const int64_t rr = live ? r : R - 1;  // (a dead slot computes the last ray again and writes nothing)
    const float* ry = rays + rr * 6;
    const float* row = ts_ray + rr * stride;
    const float nrm = sqrtf((ry[3] * ry[3] + ry[4] * ry[4]) + ry[5] * ry[5]);
    float Y[SH_MAX_K];
    if constexpr (!PROP) plv_ray_basis<K>(rays, rr, Y);
    VoxWalk walk;
    for (int t0 = 0; t0 < M; t0 += L) {
      const int t = t0 + j;
      if (t < M) {
        const float3 p = vox_ray_point(ry, row[t]);
        float a;
        float3 c = make_float3(0.f, 0.f, 0.f);
        if constexpr (PROP) {
          a = vox_alpha(vox_gather_density(p.x, p.y, p.z, g, den), row, t, M, nrm);
        } else {
          float raw[5];
          vox_gather<K, SH>(p.x, p.y, p.z, g, den, rgb, Y, raw);
          a = vox_alpha(raw[0], row, t, M, nrm);
          c = vox_colour<K, SH>(raw, act_kind);
        }
        if (live && alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = a;
        park[slot][j] = make_float4(a, c.x, c.y, c.z);
      }
      __syncthreads();
      if (j == 0 && live) {
        const int n = M - t0 < L ? M - t0 : L;
        for (int u = 0; u < n; ++u) {
          const int tu = t0 + u;
          const float4 p = park[slot][u];
          const float w = walk.weight(p.x);
          if (weights_out != nullptr) weights_out[(int64_t)tu * R + r] = w;
          if constexpr (!PROP) walk.add(w, p.y, p.z, p.w, tu == M - 1);
        }
      }
      __syncthreads();  // (the next chunk overwrites the parked steps)
    }
    if constexpr (!PROP) {
      if (j == 0 && live) walk.finish(bg_kind, out + r * 3);
    }
  }
}

}  // namespace na

using namespace na;

// lanes per ray of the shipped entry points, every head and the proposal (the other values' times)
constexpr int VFR_LANES = 16;

// every entry point ends here, its shape checked: the checks common to all (C as VoxHead::check reads it), and the launch.
// NA_VOX_HEAD_DENSITY is the proposal: no colour grid, no activation, no out.
static int vfr_any(const char* who, VoxHead h, int C, int lanes, const float* rays, int64_t R, const float* ts_ray, int64_t stride, int M,
                   const float* densities, const float* rgb, int S, double grid_radius, int act_kind, int bg_kind, float* alpha,
                   float* weights, float* out, void* stream) {
  const bool prop = h.kind == NA_VOX_HEAD_DENSITY;
  if (int rc = h.check(who, S, C, grid_radius)) return rc;
  NA_REQUIRE(vox_lanes_ok(lanes), NA_EINVAL, "%s: %d lanes per ray (4, 8, 16, 32, 64)", who, lanes);
  if (!prop) {
    if (int rc = vox_check_kinds(who, act_kind, bg_kind)) return rc;
  }
  if (R == 0) return NA_OK;
  if (prop) {
    NA_REQUIRE(rays, NA_ENULL, "%s: rays is null", who);
    NA_REQUIRE(ts_ray, NA_ENULL, "%s: ts is null", who);
    NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
    NA_REQUIRE(weights, NA_ENULL, "%s: weights is null", who);
  } else if (int rc = vox_check_render_ptrs(who, h, rays, ts_ray, "ts_ray", densities, rgb, out)) {
    return rc;
  }
  const VoxGrid g = vox_grid(S, grid_radius);
  vox_for_head(h, [&](auto k, auto tag) {
    vox_for_lanes(lanes, [&](auto l) {
      constexpr int K = decltype(k)::value, L = decltype(l)::value;
      constexpr bool SH = decltype(tag)::value;
      const dim3 grid(grid_for(R, VFR_BLOCK / L)), block(VFR_BLOCK);
      if constexpr (K < 0) {
        if (prop) {
          hipLaunchKernelGGL((voxel_fine_kernel<-1, false, true, L>), grid, block, 0, (hipStream_t)stream, rays, ts_ray, stride, M, R, g, densities,
                             nullptr, 0, 0, alpha, weights, nullptr);
          return;
        }
      }
      hipLaunchKernelGGL((voxel_fine_kernel<K, SH, false, L>), grid, block, 0, (hipStream_t)stream, rays, ts_ray, stride, M, R, g, densities, rgb,
                         act_kind, bg_kind, alpha, weights, out);
    });
  });
  return check_launch(who);
}

extern "C" {

int na_voxel_proposal(const float* rays, int64_t R, const float* ts, int T, const float* densities, int S, double grid_radius, float* alpha,
                      float* weights, void* stream) {
  const char* who = "na_voxel_proposal";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  return vfr_any(who, {NA_VOX_HEAD_DENSITY, -1}, 3, VFR_LANES, rays, R, ts, 0, T, densities, nullptr, S, grid_radius, 0, 0, alpha, weights,
                 nullptr, stream);
}

int na_voxel_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                          double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out, void* stream) {
  const char* who = "na_voxel_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  return vfr_any(who, {NA_VOX_HEAD_RGB, -1}, C, VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha, weights,
                 out, stream);
}

int na_voxel_plv_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S,
                              int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                              void* stream) {
  const char* who = "na_voxel_plv_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  const VoxHead h{NA_VOX_HEAD_PLV, order};
  return vfr_any(who, h, h.row_floats(), VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha, weights, out,
                 stream);
}

int na_voxel_sh_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                             int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                             void* stream) {
  const char* who = "na_voxel_sh_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  return vfr_any(who, {NA_VOX_HEAD_SH, order}, C, VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha,
                 weights, out, stream);
}

int na_voxel_fine_lanes(int head, int order, int lanes, int shared_row, const float* rays, int64_t R, const float* ts_ray, int M,
                        const float* densities, const float* rgb, int S, double grid_radius, int act_kind, int bg_kind, float* alpha,
                        float* weights, float* out, void* stream) {
  const char* who = "na_voxel_fine_lanes";
  NA_REQUIRE(head >= NA_VOX_HEAD_RGB && head <= NA_VOX_HEAD_DENSITY, NA_EINVAL, "%s: head %d (NA_VOX_HEAD_*)", who, head);
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  const VoxHead h{head, order};
  return vfr_any(who, h, h.row_floats(), lanes, rays, R, ts_ray, shared_row ? 0 : M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha,
                 weights, out, stream);
}

}  // extern "C"
