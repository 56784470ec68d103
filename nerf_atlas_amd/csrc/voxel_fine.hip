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
        // o + t d as vox_position forms it: an fp32 multiply, then an fp32 add
        const float tt = row[t];
        const float px = ry[0] + tt * ry[3], py = ry[1] + tt * ry[4], pz = ry[2] + tt * ry[5];
        float a, c0 = 0.f, c1 = 0.f, c2 = 0.f;
        if constexpr (PROP) {
          a = vox_alpha(vox_gather_density(px, py, pz, g, den), row, t, M, nrm);
        } else {
          float raw[5];
          vox_gather<K, SH>(px, py, pz, g, den, rgb, Y, raw);
          a = vox_alpha(raw[0], row, t, M, nrm);
          c0 = apply_sigmoid_kind(raw[1], act_kind); c1 = apply_sigmoid_kind(raw[2], act_kind); c2 = apply_sigmoid_kind(raw[3], act_kind);
          if constexpr (K >= 0 && !SH) {
            const float lin = plv_scale(raw[4]);
            c0 = lin * c0; c1 = lin * c1; c2 = lin * c2;
          }
        }
        if (live && alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = a;
        park[slot][j] = make_float4(a, c0, c1, c2);
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

enum { VFR_RGB = 0, VFR_PLV = 1, VFR_SH = 2, VFR_DENSITY = 3 };  // include/nerf_atlas_amd.h NA_VOX_HEAD_*

// lanes per ray of the shipped entry points, every head and the proposal (the other values' times)
constexpr int VFR_LANES = 16;

template <int K, bool SH, bool PROP>
static void vfr_launch(int lanes, hipStream_t s, const float* rays, const float* ts_ray, int64_t stride, int M, int64_t R, VoxGrid g,
                       const float* den, const float* rgb, int act_kind, int bg_kind, float* alpha, float* weights, float* out) {
#define NA_VFR_L(LN)                                                                                                                   \
  hipLaunchKernelGGL((voxel_fine_kernel<K, SH, PROP, LN>), dim3(grid_for(R, VFR_BLOCK / LN)), dim3(VFR_BLOCK), 0, s, rays, ts_ray, stride, M, R, \
                     g, den, rgb, act_kind, bg_kind, alpha, weights, out)
  switch (lanes) {
    case 4: NA_VFR_L(4); break;
    case 8: NA_VFR_L(8); break;
    case 16: NA_VFR_L(16); break;
    case 32: NA_VFR_L(32); break;
    default: NA_VFR_L(64); break;
  }
#undef NA_VFR_L
}

// every entry point ends here, its own checks done: the checks common to all, and the launch
static int vfr_any(const char* who, int head, int order, int lanes, const float* rays, int64_t R, const float* ts_ray, int64_t stride, int M,
                   const float* densities, const float* rgb, int S, double grid_radius, int act_kind, int bg_kind, float* alpha,
                   float* weights, float* out, void* stream) {
  NA_REQUIRE(lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64, NA_EINVAL, "%s: %d lanes per ray (4, 8, 16, 32, 64)", who, lanes);
  if (head != VFR_DENSITY) {
    NA_REQUIRE(act_kind >= NA_SIG_NORMAL && act_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "%s: activation kind %d", who, act_kind);
    NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "%s: bg kind %d", who, bg_kind);
  }
  if (R == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null", who);
  NA_REQUIRE(ts_ray, NA_ENULL, "%s: %s is null", who, head == VFR_DENSITY ? "ts" : "ts_ray");
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  if (head == VFR_DENSITY) {
    NA_REQUIRE(weights, NA_ENULL, "%s: weights is null", who);
  } else {
    NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
    NA_REQUIRE(out, NA_ENULL, "%s: out is null", who);
    const int row = head == VFR_RGB ? 3 : head == VFR_SH ? 3 * (order + 1) * (order + 1) : 3 + (order + 1) * (order + 1);  // floats of a grid row
    NA_REQUIRE(row % 4 != 0 || ((uintptr_t)rgb & 15) == 0, NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, order);
  }
  const VoxGrid g = vox_grid(S, grid_radius);
  hipStream_t s = (hipStream_t)stream;
#define NA_VFR_HEAD(K, SH) vfr_launch<K, SH, false>(lanes, s, rays, ts_ray, stride, M, R, g, densities, rgb, act_kind, bg_kind, alpha, weights, out)
  if (head == VFR_DENSITY) vfr_launch<-1, false, true>(lanes, s, rays, ts_ray, stride, M, R, g, densities, nullptr, 0, 0, alpha, weights, nullptr);
  else if (head == VFR_RGB) NA_VFR_HEAD(-1, false);
  else if (head == VFR_PLV) switch (order) {
    case 0: NA_VFR_HEAD(0, false); break;
    case 1: NA_VFR_HEAD(1, false); break;
    case 2: NA_VFR_HEAD(2, false); break;
    case 3: NA_VFR_HEAD(3, false); break;
    default: NA_VFR_HEAD(4, false); break;
  }
  else switch (order) {
    case 0: NA_VFR_HEAD(0, true); break;
    case 1: NA_VFR_HEAD(1, true); break;
    case 2: NA_VFR_HEAD(2, true); break;
    case 3: NA_VFR_HEAD(3, true); break;
    default: NA_VFR_HEAD(4, true); break;
  }
#undef NA_VFR_HEAD
  return check_launch(who);
}

extern "C" {

int na_voxel_proposal(const float* rays, int64_t R, const float* ts, int T, const float* densities, int S, double grid_radius, float* alpha,
                      float* weights, void* stream) {
  const char* who = "na_voxel_proposal";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = vox_check_grid(who, S, 3, grid_radius)) return rc;
  return vfr_any(who, VFR_DENSITY, -1, VFR_LANES, rays, R, ts, 0, T, densities, nullptr, S, grid_radius, 0, 0, alpha, weights,
                 nullptr, stream);
}

int na_voxel_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                          double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out, void* stream) {
  const char* who = "na_voxel_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  if (int rc = vox_check_grid(who, S, C, grid_radius)) return rc;
  return vfr_any(who, VFR_RGB, -1, VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha, weights,
                 out, stream);
}

int na_voxel_plv_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S,
                              int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                              void* stream) {
  const char* who = "na_voxel_plv_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  return vfr_any(who, VFR_PLV, order, VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha,
                 weights, out, stream);
}

int na_voxel_sh_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                             int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                             void* stream) {
  const char* who = "na_voxel_sh_render_rayts";
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  NA_REQUIRE(C == 3 * (order + 1) * (order + 1), NA_EINVAL, "%s: C = %d, the spherical-harmonic head of order %d holds 3 (order + 1)^2 = %d", who, C,
             order, 3 * (order + 1) * (order + 1));
  return vfr_any(who, VFR_SH, order, VFR_LANES, rays, R, ts_ray, M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha,
                 weights, out, stream);
}

int na_voxel_fine_lanes(int head, int order, int lanes, int shared_row, const float* rays, int64_t R, const float* ts_ray, int M,
                        const float* densities, const float* rgb, int S, double grid_radius, int act_kind, int bg_kind, float* alpha,
                        float* weights, float* out, void* stream) {
  const char* who = "na_voxel_fine_lanes";
  NA_REQUIRE(head >= VFR_RGB && head <= VFR_DENSITY, NA_EINVAL, "%s: head %d (NA_VOX_HEAD_*)", who, head);
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  if (head == VFR_PLV || head == VFR_SH) {
    if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  } else if (int rc = vox_check_grid(who, S, 3, grid_radius)) {
    return rc;
  }
  return vfr_any(who, head, order, lanes, rays, R, ts_ray, shared_row ? 0 : M, M, densities, rgb, S, grid_radius, act_kind, bg_kind, alpha, weights,
                 out, stream);
}

}  // extern "C"
