// NeRFVoxel with the per-voxel pos-linear-view head (src/refl.py:265-280): the grid row is [raw rgb (3) | (K+1)^2
// spherical-harmonic coefficients], C = 3 + (K+1)^2, and a sample's colour is act(raw rgb) * (sigmoid(s) / 2 + 0.5) with
// s = sum_k Y_k(normalize(view)) c_k.  Four operators over voxel_plv.h's lookup (vox_plv_gather: cells and weights of voxel_cell.h, the
// coefficients contracted with the ray's basis in registers):
//   na_voxel_plv_sample               raw [N, 4] = [density | 3 colour parameters] and sh [N] = s
//   na_voxel_plv_sample_backward      scatter-add of w_u [g_raw | g_sh Y_k] into the two grids
//   na_voxel_plv_sample_backward_pts  the gradient w.r.t. explicit positions (a gather)
//   na_voxel_plv_render               the eval route as one launch: basis once per ray, lookup, activation, linear scale, compositing
// K is a template parameter: every loop over the coefficients unrolls and the basis stays in VGPRs.  The ray of sample n is n % R.
// Built like voxel.hip (-ffp-contract=off; the only fused operations are the explicit fmaf of plv_contract).
#include "voxel_plv.h"
#include <type_traits>

namespace na {

// ------------------------------------------------------------------------------------ gather
template <int K>
__global__ __launch_bounds__(256) void plv_sample_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                         const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                         const float* __restrict__ den, const float* __restrict__ rgb,
                                                         float* __restrict__ raw, float* __restrict__ sh) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    float Y[SH_MAX_K], px, py, pz, v[5];
    plv_ray_basis<K>(rays, n % R, Y);
    vox_position(pts, rays, ts, R, n, px, py, pz);
    vox_plv_gather<K>(px, py, pz, g, den, rgb, Y, v);
    *(float4*)(raw + n * 4) = make_float4(v[0], v[1], v[2], v[3]);
    sh[n] = v[4];
  }
}

// ------------------------------------------------------------------------------------ gather: gradient w.r.t. the positions
// voxel_backward_pts_kernel with the per-corner value g_d den[row] + sum_c g_c rgb[row, c] + g_sh sum_k Y_k rgb[row, 3 + k]
template <int K>
__global__ __launch_bounds__(256) void plv_backward_pts_kernel(const float* __restrict__ pts, const float* __restrict__ rays, int64_t R,
                                                               int64_t N, VoxGrid g, const float* __restrict__ den,
                                                               const float* __restrict__ rgb, const float* __restrict__ g_raw,
                                                               const float* __restrict__ g_sh, float* __restrict__ g_pts) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    float Y[SH_MAX_K];
    plv_ray_basis<K>(rays, n % R, Y);
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    const float4 gv = *(const float4*)(g_raw + n * 4);
    const float gs = g_sh[n];
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = vox_row(c, u, g.S);
      float q[Plv<K>::C];
      plv_load_row<K>(rgb + row * Plv<K>::C, q);
      const float v = (((gv.x * den[row] + gv.y * q[0]) + gv.z * q[1]) + gv.w * q[2]) + gs * plv_contract<K>(q, Y);
      const float wx = (u & 1) ? c.x : 1.f - c.x, wy = (u & 2) ? c.y : 1.f - c.y, wz = (u & 4) ? c.z : 1.f - c.z;
      const float dx = wy * wz, dy = wx * wz, dz = wx * wy;
      gx = gx + ((u & 1) ? dx : -dx) * v;
      gy = gy + ((u & 2) ? dy : -dy) * v;
      gz = gz + ((u & 4) ? dz : -dz) * v;
    }
    const bool bad = (c.x != c.x) | (c.y != c.y) | (c.z != c.z);
    const float nan = __builtin_nanf("");
    g_pts[n * 3] = bad ? nan : gx / g.vl;
    g_pts[n * 3 + 1] = bad ? nan : gy / g.vl;
    g_pts[n * 3 + 2] = bad ? nan : gz / g.vl;
  }
}

// ------------------------------------------------------------------------------------ scatter-add
// Corner u of sample n receives w_u [g_raw[n, 0] | g_raw[n, 1..3] | g_sh[n] Y_k]: 1 + C sums per grid row, 29 at K = 4.  The scheme
// of voxel_backward_kernel -- a workgroup takes a contiguous run of samples and sums into a hashed LDS table of grid rows that
// is flushed once -- with the table redesigned for 1 + C sums per row (1024 rows x 29 sums x 8 B do not fit a CU's 160 KiB):
//   variant 1 (FULL)  whole rows in the table, as many rows as fit 60 KiB (two workgroups per CU): fp32 mode keeps 4-byte
//                     entries (512 rows at K = 4), the deterministic mode 8-byte fixed-point entries (256 rows)
//   variant 2 (LEAD)  the table of voxel_backward_kernel, 1024 rows x 4 sums x 8 B, for [density | rgb]; the SH block goes
//                     straight to the global accumulators
// A row whose slots are taken falls through to the global accumulators, so the result does not depend on the table at all in
// exact arithmetic.  Deterministic mode (fix != nullptr): every contribution is converted to 2^-40 fixed point on its own and
// only integers are added, in LDS and in memory alike: the bits do not depend on the order of the samples.
// NA_PLV_SCATTER picks the variant na_voxel_plv_sample_backward runs (DESIGN.md 3p has the times of both).
#ifndef NA_PLV_SCATTER
#define NA_PLV_SCATTER 1
#endif
constexpr int PLV_WG = 4096;     // workgroups at most (voxel.hip's NA_VOXEL_MAX_WG)
constexpr int PLV_PROBES = 4;    // (voxel.hip's NA_VOXEL_PROBES)
constexpr int PLV_LDS_BUDGET = 60 * 1024;  // table bytes of a workgroup: two workgroups share a CU's 160 KiB

template <int K, int VARIANT, bool DET> struct PlvTable {
  static constexpr int SUMS = VARIANT == 1 ? 1 + Plv<K>::C : 4;   // sums of a table row
  static constexpr int ENTRY = (DET || VARIANT == 2) ? 8 : 4;     // bytes of a sum
  static constexpr int rows_for(int r) { return (r * 2 * (SUMS * ENTRY + 4) <= PLV_LDS_BUDGET && r < 1024) ? rows_for(r * 2) : r; }
  static constexpr int ROWS = rows_for(1);                        // a power of two, 1024 at most
  static constexpr int LOG2 = ROWS == 1024 ? 10 : ROWS == 512 ? 9 : ROWS == 256 ? 8 : ROWS == 128 ? 7 : ROWS == 64 ? 6 : -1;
  static_assert(LOG2 > 0, "table rows");
};

template <int K, int VARIANT, bool DET>
__global__ __launch_bounds__(256) void plv_backward_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                           const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                           const float* __restrict__ g_raw, const float* __restrict__ g_sh,
                                                           float* __restrict__ g_den, float* __restrict__ g_rgb,
                                                           long long* __restrict__ fix) {
  using T = PlvTable<K, VARIANT, DET>;
  using E = typename std::conditional<T::ENTRY == 8, unsigned long long, float>::type;
  constexpr int C = Plv<K>::C, NK = Plv<K>::NK, SUMS = T::SUMS, ROWS = T::ROWS;
  const int64_t S3 = (int64_t)g.S * g.S * g.S;
  long long* fix_rgb = DET ? fix + S3 : nullptr;
  long long* fix_den = DET ? fix : nullptr;
  // sum e of grid row id: e = 0 density, e = 1 + c channel c of the rgb row
  auto add_global = [&](uint32_t id, int e, float v) {
    if (e == 0) accumulate(g_den, fix_den, (int64_t)id, v);
    else accumulate(g_rgb, fix_rgb, (int64_t)id * C + (e - 1), v);
  };
  __shared__ uint32_t tags[ROWS];
  __shared__ E vals[ROWS * SUMS];
  for (int i = threadIdx.x; i < ROWS; i += 256) tags[i] = 0xffffffffu;
  for (int i = threadIdx.x; i < ROWS * SUMS; i += 256) vals[i] = (E)0;
  __syncthreads();
  auto add_entry = [&](uint32_t id, int slot, int e, float v) {
    if constexpr (T::ENTRY == 4) {
      atomicAdd(&vals[slot * SUMS + e], v);
    } else {
      if (!DET) atomicAdd((float*)&vals[slot * SUMS + e], v);  // (the low word of a zeroed 8-byte entry)
      else if (fabsf(v) < 1048576.0f) atomicAdd(&vals[slot * SUMS + e], (unsigned long long)__float2ll_rn(v * kFixScale));
      else add_global(id, e, v);  // (out of the fixed-point range, NaN: the fp32 path, as accumulate() does)
    }
  };
  // the slot of grid row id, or -1: a multiplicative hash with PLV_PROBES linear probes; a slot is never freed, so an id finds the
  // same slot every time, or none
  auto find_slot = [&](uint32_t id) -> int {
    const uint32_t home = (id * 2654435761u) >> (32 - T::LOG2);
    for (int p = 0; p < PLV_PROBES; ++p) {
      const uint32_t slot = (home + p) & (ROWS - 1);
      const uint32_t old = atomicCAS(&tags[slot], 0xffffffffu, id);
      if (old == 0xffffffffu || old == id) return (int)slot;
    }
    return -1;
  };
  const int64_t per = ((N + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;  // samples of this workgroup: whole rounds
  const int64_t n_lo = blockIdx.x * per, n_hi = n_lo + per < N ? n_lo + per : N;
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    if (n < n_hi) {
      float Y[SH_MAX_K], px, py, pz;
      plv_ray_basis<K>(rays, n % R, Y);
      vox_position(pts, rays, ts, R, n, px, py, pz);
      const VoxCell c = vox_cell(px, py, pz, g);
      const float4 gv = *(const float4*)(g_raw + n * 4);
      const float gs = g_sh[n];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t id = (uint32_t)vox_row(c, u, g.S);
        const float w = vox_weight(c, u);
        const float lead[4] = {w * gv.x, w * gv.y, w * gv.z, w * gv.w};
        const float as = w * gs;
        const int slot = find_slot(id);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (slot >= 0) add_entry(id, slot, e, lead[e]);
          else add_global(id, e, lead[e]);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float a = as * Y[k];
          if (VARIANT == 1 && slot >= 0) add_entry(id, slot, 4 + k, a);
          else add_global(id, 4 + k, a);
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ROWS * SUMS; i += 256) {
    const int slot = i / SUMS, e = i - slot * SUMS;
    const uint32_t id = tags[slot];
    if (id == 0xffffffffu) continue;
    const int64_t at = e == 0 ? (int64_t)id : (int64_t)id * C + (e - 1);
    if constexpr (T::ENTRY == 4) {
      const float v = vals[i];
      if (v != 0.f) atomicAdd((e == 0 ? g_den : g_rgb) + at, v);
    } else {
      const unsigned long long v = vals[i];
      if (v == 0ull) continue;
      if (!DET) atomicAdd((e == 0 ? g_den : g_rgb) + at, __uint_as_float((uint32_t)v));
      else atomicAdd((unsigned long long*)((e == 0 ? fix_den : fix_rgb) + at), v);
    }
  }
}

// ------------------------------------------------------------------------------------ eval route, one launch
// voxel_render_kernel with the head: the basis is evaluated once per ray and held in registers over the walk; per step the lookup,
// act_kind on the colour parameters, the linear scale and na_composite's arithmetic on the same device functions.
template <int K>
__global__ __launch_bounds__(64) void plv_render_kernel(const float* __restrict__ rays, const float* __restrict__ pts,
                                                        const float* __restrict__ ts, int T, int64_t R, VoxGrid g,
                                                        const float* __restrict__ den, const float* __restrict__ rgb, int act_kind,
                                                        int bg_kind, float* __restrict__ alpha_out, float* __restrict__ weights_out,
                                                        float* __restrict__ out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    const float* ry = rays + r * 6 + 3;
    const float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
    float Y[SH_MAX_K];
    plv_ray_basis<K>(rays, r, Y);
    float trans = 1.0f, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum_head = 0.f;
    constexpr int U = K <= 1 ? 2 : 1;  // steps gathered ahead of the walk (wider rows: one, or the rows in flight leave the registers)
    for (int t0 = 0; t0 < T; t0 += U) {
      float raw[U][5];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;  // (clamped: the tail gathers the last step again and ignores it)
        float px, py, pz;
        vox_position(pts, rays, ts, R, (int64_t)t * R + r, px, py, pz);
        vox_plv_gather<K>(px, py, pz, g, den, rgb, Y, raw[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t < T) {
          const float sigma = fast_softplus(raw[u][0] - 1.0f);
          float dist = t < T - 1 ? fmaxf(ts[t + 1] - ts[t], 1e-5f) : 1e10f;
          dist = dist * nrm;
          const float a = 1.0f - fast_exp(-sigma * dist);
          const float w = a * trans;
          trans = trans * ((1.0f - a) + 1e-10f);
          if (alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = a;
          if (weights_out != nullptr) weights_out[(int64_t)t * R + r] = w;
          const float lin = plv_scale(raw[u][4]);
          acc0 = acc0 + w * (lin * apply_sigmoid_kind(raw[u][1], act_kind));
          acc1 = acc1 + w * (lin * apply_sigmoid_kind(raw[u][2], act_kind));
          acc2 = acc2 + w * (lin * apply_sigmoid_kind(raw[u][3], act_kind));
          if (t < T - 1) wsum_head = wsum_head + w;
        }
      }
    }
    const float sky = bg_kind == NA_BG_WHITE ? 1.0f - wsum_head : 0.f;
    out[r * 3] = acc0 + sky; out[r * 3 + 1] = acc1 + sky; out[r * 3 + 2] = acc2 + sky;
  }
}

template <int K, int VARIANT>
static void launch_backward(unsigned wg, hipStream_t s, const float* pts, const float* rays, const float* ts, int64_t R, int64_t N,
                            VoxGrid g, const float* g_raw, const float* g_sh, float* g_den, float* g_rgb, long long* fix) {
  if (fix != nullptr)
    hipLaunchKernelGGL((plv_backward_kernel<K, VARIANT, true>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_den, g_rgb, fix);
  else
    hipLaunchKernelGGL((plv_backward_kernel<K, VARIANT, false>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_den, g_rgb, fix);
}

}  // namespace na

using namespace na;

// `order` was checked (0 .. 4): expands the statement once with K bound to it
#define NA_PLV_ORDER(order, ...)                  \
  switch (order) {                                \
    case 0: { constexpr int K = 0; __VA_ARGS__; } break; \
    case 1: { constexpr int K = 1; __VA_ARGS__; } break; \
    case 2: { constexpr int K = 2; __VA_ARGS__; } break; \
    case 3: { constexpr int K = 3; __VA_ARGS__; } break; \
    default: { constexpr int K = 4; __VA_ARGS__; } break; \
  }

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// rows of 4 C bytes are read with 16-byte loads when C % 4 == 0: the grid must then start on a 16-byte boundary
static bool grid_aligned(const float* rgb, int order) { return ((order + 1) * (order + 1) + 3) % 4 != 0 || aligned16(rgb); }

extern "C" {

int na_voxel_plv_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, float* raw, float* sh, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_plv_sample: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_plv_check_grid("na_voxel_plv_sample", S, order, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "na_voxel_plv_sample: rays is null (the directions of the head)");
  NA_REQUIRE(pts || ts, NA_ENULL, "na_voxel_plv_sample: pts and ts are both null");
  NA_REQUIRE(densities, NA_ENULL, "na_voxel_plv_sample: densities is null");
  NA_REQUIRE(rgb, NA_ENULL, "na_voxel_plv_sample: rgb is null");
  NA_REQUIRE(raw, NA_ENULL, "na_voxel_plv_sample: raw is null");
  NA_REQUIRE(sh, NA_ENULL, "na_voxel_plv_sample: sh is null");
  NA_REQUIRE(aligned16(raw), NA_EINVAL, "na_voxel_plv_sample: raw must be 16-byte aligned");
  NA_REQUIRE(grid_aligned(rgb, order), NA_EINVAL, "na_voxel_plv_sample: rgb must be 16-byte aligned at order %d", order);
  const VoxGrid g = vox_grid(S, grid_radius);
  NA_PLV_ORDER(order, hipLaunchKernelGGL(plv_sample_kernel<K>, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts, R,
                                         N, g, densities, rgb, raw, sh));
  return check_launch("na_voxel_plv_sample");
}

int na_voxel_plv_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                         const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb,
                                         int variant, void* stream) {
  const char* who = "na_voxel_plv_sample_backward";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  NA_REQUIRE(variant == 1 || variant == 2, NA_EINVAL, "%s: scatter variant %d (1: whole rows in LDS, 2: leading sums in LDS)", who, variant);
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(pts || ts, NA_ENULL, "%s: pts and ts are both null", who);
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(g_sh, NA_ENULL, "%s: g_sh is null", who);
  NA_REQUIRE(g_densities, NA_ENULL, "%s: g_densities is null", who);
  NA_REQUIRE(g_rgb, NA_ENULL, "%s: g_rgb is null", who);
  NA_REQUIRE(aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  const size_t S3 = (size_t)S * S * S, Cn = 3 + (size_t)(order + 1) * (order + 1);
  int rc;
  long long* fix = det_begin(S3 * (1 + Cn), (hipStream_t)stream, who, &rc);
  if (rc != NA_OK) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
  const unsigned wg = grid_for(N, 256, PLV_WG);
  NA_PLV_ORDER(order, if (variant == 1) launch_backward<K, 1>(wg, (hipStream_t)stream, pts, rays, ts, R, N, g, g_raw, g_sh, g_densities,
                                                              g_rgb, fix);
               else launch_backward<K, 2>(wg, (hipStream_t)stream, pts, rays, ts, R, N, g, g_raw, g_sh, g_densities, g_rgb, fix));
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3, g_densities, (hipStream_t)stream, who)) return rc2;
    return det_finish(fix + S3, S3 * Cn, g_rgb, (hipStream_t)stream, who);
  }
  return check_launch(who);
}

int na_voxel_plv_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                 const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  return na_voxel_plv_sample_backward_variant(pts, rays, R, ts, T, g_raw, g_sh, S, order, grid_radius, g_densities, g_rgb, NA_PLV_SCATTER,
                                              stream);
}

int na_voxel_plv_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                     const float* g_raw, const float* g_sh, int S, int order, double grid_radius, float* g_pts,
                                     void* stream) {
  const char* who = "na_voxel_plv_sample_backward_pts";
  NA_REQUIRE(N >= 0 && R >= 0 && (N == 0 || (R >= 1 && N % R == 0)), NA_EINVAL, "%s: bad shape N=%lld R=%lld", who, (long long)N, (long long)R);
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts, NA_ENULL, "%s: pts is null", who);
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null (the directions of the head)", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(g_raw, NA_ENULL, "%s: g_raw is null", who);
  NA_REQUIRE(g_sh, NA_ENULL, "%s: g_sh is null", who);
  NA_REQUIRE(g_pts, NA_ENULL, "%s: g_pts is null", who);
  NA_REQUIRE(aligned16(g_raw), NA_EINVAL, "%s: g_raw must be 16-byte aligned", who);
  NA_REQUIRE(grid_aligned(rgb, order), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, order);
  const VoxGrid g = vox_grid(S, grid_radius);
  NA_PLV_ORDER(order, hipLaunchKernelGGL(plv_backward_pts_kernel<K>, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, R,
                                         N, g, densities, rgb, g_raw, g_sh, g_pts));
  return check_launch(who);
}

int na_voxel_plv_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                        void* stream) {
  const char* who = "na_voxel_plv_render";
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  if (int rc = vox_plv_check_grid(who, S, order, grid_radius)) return rc;
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
  NA_PLV_ORDER(order, hipLaunchKernelGGL(plv_render_kernel<K>, dim3(grid_for(R, 64)), dim3(64), 0, (hipStream_t)stream, rays, pts, ts, T, R,
                                         g, densities, rgb, act_kind, bg_kind, alpha, weights, out));
  return check_launch(who);
}

}  // extern "C"
