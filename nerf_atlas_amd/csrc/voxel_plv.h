// The kernels of a voxel model (NeRFVoxel, src/nerf.py:401-524) for both of its heads, as templates over K:
//   K = -1      the per-voxel RGB head: grid rows of C = 3 colour parameters (voxel.hip has the entry points of all three heads)
//   K = 0 .. 4  the view-dependent head (PosLinearView.to_voxel, src/refl.py:265-280): the grid row is
//               [raw rgb (3) | (K+1)^2 coefficients of ONE spherical-harmonic channel], C = 3 + (K+1)^2 floats, and
//     rgb = act(raw_rgb) * (sigmoid(s) / 2 + 0.5),   s = sum_k Y_k(normalize(view)) c_k,   c_k = the interpolated coefficient k.
// Interpolation and expansion are both linear in the grid, and Y depends on the ray only, so the lookup contracts every corner's
// coefficients with the ray's basis as the row arrives: the (K+1)^2 interpolated coefficients never exist.  At K = -1 there is no
// basis, no sh output and no linear scale: `if constexpr (K >= 0)` leaves the RGB head's own code.  The ray of sample n is n % R.
// Also here, for every renderer (this file's, voxel_fine.hip, voxel_sparse.hip, dyn_voxel_render.hip): the lookup (vox_gather), one
// shading step (vox_colour), the position of a ray's own step (vox_ray_point) and one compositing step (vox_alpha, VoxWalk).  The host side of a head -- VoxHead, vox_for_head -- is voxel_head.h's.
//
// A third head rides on the same kernels under the tag SH: the per-voxel spherical-harmonic
// colour (SphericalHarmonic.to_voxel, src/refl.py:715-722, the Plenoxels model).  The grid row is 3 channel blocks of NK = (K+1)^2
// coefficients, C = 3 NK floats, coefficient k of colour channel c at c NK + k, and
//     rgb_c = act(s_c),   s_c = sum_u w_u sum_k Y_k(normalize(view)) row_u[c NK + k].
// Each block is contracted as it arrives, with the association below (d_uc for row_u[c NK ..], then s_c = s_c + w_u d_uc), so a block that
// equals a pos-linear-view row's coefficients gives that head's s bit for bit; the outputs are v[0] = density, v[1..3] = s_c: the RGB
// head's raw [N, 4], with no sh output and no linear scale.
//
// ASSOCIATION (one function for every route; tests/voxel_plv_ref.py derives the bound from these counts):
//     d_u = fma(Y_k, row_u[3 + k], d_u) for k = 1 .. NK-1 in k order, from d_u = Y_0 * row_u[3]      (coefficients first: NK roundings)
//     s   = s + w_u * d_u for the corners u = 0 .. 7 in corner order, from s = 0                     (a product and a sum per corner)
// Density and the three colour parameters are v_i = v_i + w_u * row_u[i] in corner order from 0, the same for every K: with all
// coefficients zero the four leading outputs are na_voxel_sample's bits.
// Cells, weights and rows are voxel_cell.h's (the operator's definition and its memory-safety rule): the ids are
// integer-clamped whatever the coordinate is, and a non-finite coordinate makes xyz -- hence every weight and every output of that
// sample -- NaN.
#pragma once
#include "sh_basis.h"
#include "voxel_head.h"
#include "voxel_scatter.h"

namespace na {

template <int K, bool SH = false> struct Plv {
  static constexpr int NK = (K + 1) * (K + 1);  // coefficients per voxel and channel (none at K = -1)
  static constexpr int C = SH ? 3 * NK : 3 + NK;  // floats per grid row: 3 | 4, 7, 12, 19, 28 | SH: 3, 12, 27, 48, 75
  static constexpr bool ALIGNED = C % 4 == 0;   // rows of 4 C bytes are 16-byte aligned for K = 0, 2, 4 only (SH: K = 1, 3)
};

// one grid row into registers: 16-byte loads where every row is 16-byte aligned, 4-byte loads otherwise
template <int K> __device__ __forceinline__ void plv_load_row(const float* __restrict__ q, float (&r)[Plv<K>::C]) {
  constexpr int C = Plv<K>::C;
  if constexpr (Plv<K>::ALIGNED) {
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const float4 v = ((const float4*)q)[i];
      r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) r[i] = q[i];
  }
}

// d = sum_k Y_k row[3 + k], the association of the header comment (0 at K = -1: nothing reads it)
template <int K> __device__ __forceinline__ float plv_contract(const float (&r)[Plv<K>::C], const float (&Y)[SH_MAX_K]) {
  if constexpr (K < 0) {
    return 0.f;
  } else {
    float d = Y[0] * r[3];
#pragma unroll
    for (int k = 1; k < Plv<K>::NK; ++k) d = fmaf(Y[k], r[3 + k], d);
    return d;
  }
}

// vox_row for a corner loop that stays a loop (the SH head's rows are too wide to unroll over): the cell's ids are read once, in front
// of the loop, and corner u selects among scalars -- a run-time index into the cell's arrays would put the cell into scratch
struct VoxRows {
  int64_t x0, x1, y0, y1, z0, z1;
  __device__ __forceinline__ VoxRows(const VoxCell& c, int S)
      : x0((int64_t)c.ix[0] * S * S), x1((int64_t)c.ix[1] * S * S), y0((int64_t)c.iy[0] * S), y1((int64_t)c.iy[1] * S), z0(c.iz[0]), z1(c.iz[1]) {}
  // (by value: `bit ? x1 : x0` on the members is an lvalue, a select between two ADDRESSES, and the struct stays in memory)
  static __device__ __forceinline__ int64_t pick(bool hi, int64_t a, int64_t b) { return hi ? b : a; }
  __device__ __forceinline__ int64_t operator()(int u) const { return pick(u & 1, x0, x1) + pick(u & 2, y0, y1) + pick(u & 4, z0, z1); }
};

// SH head: d[c] = sum_k Y_k q[c NK + k] for the three channel blocks of one grid row, each block loaded (16 bytes at a time where the
// rows are aligned: NK is then a multiple of 4) and contracted on its own with plv_contract's association -- a row never sits in
// registers whole
template <int K> __device__ __forceinline__ void sh_contract_row(const float* __restrict__ q, const float (&Y)[SH_MAX_K], float (&d)[3]) {
  constexpr int NK = Plv<K, true>::NK;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float r[NK];
    if constexpr (Plv<K, true>::ALIGNED) {
#pragma unroll
      for (int i = 0; i < NK / 4; ++i) {
        const float4 v = ((const float4*)(q + c * NK))[i];
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < NK; ++k) r[k] = q[c * NK + k];
    }
    float a = Y[0] * r[0];
#pragma unroll
    for (int k = 1; k < NK; ++k) a = fmaf(Y[k], r[k], a);
    d[c] = a;
  }
}

// the basis of ray r (dirs = rays[:, 3:6], un-normalised: sh_basis normalises with F.normalize's eps like na_sh_shade)
template <int K> __device__ __forceinline__ void plv_ray_basis(const float* __restrict__ rays, int64_t r, float (&Y)[SH_MAX_K]) {
  if constexpr (K >= 0) {
    const float* d = rays + r * 6 + 3;
    sh_basis(K, d[0], d[1], d[2], Y);
  }
}

// v[0] = density, v[1..3] = colour parameters, v[4] = s (K >= 0): the per-sample lookup of every kernel.  Sums over the 8 corners
// in corner order (the S = 64 grid of the RGB head is 4 MiB and stays in the L2 / Infinity Cache).  SH: v[1..3] = s_c, v[4] unused.
template <int K, bool SH = false>
__device__ __forceinline__ void vox_gather(float px, float py, float pz, const VoxGrid& g, const float* __restrict__ den,
                                           const float* __restrict__ rgb, const float (&Y)[SH_MAX_K], float v[5]) {
  const VoxCell c = vox_cell(px, py, pz, g);
  v[0] = v[1] = v[2] = v[3] = v[4] = 0.f;
  if constexpr (SH) {
    // the corners as a real loop, one row in flight: unrolled, all 8 rows' loads are hoisted (600 registers at K = 4) and the render
    // kernels spill
    const VoxRows rows(c, g.S);
#pragma unroll 1
    for (int u = 0; u < 8; ++u) {
      const int64_t row = rows(u);
      const float w = vox_weight(c, u);
      float d[3];
      sh_contract_row<K>(rgb + row * Plv<K, true>::C, Y, d);
      v[0] = v[0] + w * den[row];
      v[1] = v[1] + w * d[0];
      v[2] = v[2] + w * d[1];
      v[3] = v[3] + w * d[2];
    }
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = vox_row(c, u, g.S);
      const float w = vox_weight(c, u);
      float r[Plv<K>::C];
      plv_load_row<K>(rgb + row * Plv<K>::C, r);
      const float d = plv_contract<K>(r, Y);
      v[0] = v[0] + w * den[row];
      v[1] = v[1] + w * r[0];
      v[2] = v[2] + w * r[1];
      v[3] = v[3] + w * r[2];
      if constexpr (K >= 0) v[4] = v[4] + w * d;
    }
  }
}

// (sigmoid(s) / 2 + 0.5) * act(p): pos_linear_combine_kernel's arithmetic behind apply_sigmoid_kind
__device__ __forceinline__ float plv_scale(float s) { return sigmoidf_(s) / 2.0f + 0.5f; }

// the shading step of every renderer: a gathered row's three colour logits through the activation, times the linear scale with the
// pos-linear-view head (lin * act(p)); SH and the RGB head: the activation alone
template <int K, bool SH>
__device__ __forceinline__ float3 vox_colour(const float raw[5], int act_kind) {
  float c0 = apply_sigmoid_kind(raw[1], act_kind), c1 = apply_sigmoid_kind(raw[2], act_kind), c2 = apply_sigmoid_kind(raw[3], act_kind);
  if constexpr (K >= 0 && !SH) {
    const float lin = plv_scale(raw[4]);
    c0 = lin * c0; c1 = lin * c1; c2 = lin * c2;
  }
  return make_float3(c0, c1, c2);
}

// o + tt d of the ray at ry = rays + r * 6 as vox_position forms it: an fp32 multiply, then an fp32 add
__device__ __forceinline__ float3 vox_ray_point(const float* ry, float tt) {
  return make_float3(ry[0] + tt * ry[3], ry[1] + tt * ry[4], ry[2] + tt * ry[5]);
}

// ------------------------------------------------------------------------------------ one compositing step
// composite_kernel's (basic_ops.hip) per-step arithmetic on the same device functions, for the three one-launch renderers.
// The per-sample part, independent of the walk: sigma = fast_softplus(raw0 - 1); dist = max(ts[t + 1] - ts[t], 1e-5), 1e10 at the
// last step, times nrm; alpha = 1 - fast_exp(-sigma dist).
__device__ __forceinline__ float vox_alpha(float raw0, const float* __restrict__ ts, int t, int T, float nrm) {
  const float sigma = fast_softplus(raw0 - 1.0f);
  float dist = t < T - 1 ? fmaxf(ts[t + 1] - ts[t], 1e-5f) : 1e10f;
  dist = dist * nrm;
  return 1.0f - fast_exp(-sigma * dist);
}

// The walk, in ascending t: w = a trans; trans <- trans ((1 - a) + 1e-10) (the reference's cumprod association);
// acc_i <- acc_i + w c_i; wsum_head <- wsum_head + w except at the last step.  finish: the sky is 1 - wsum_head on white, 0 on black.
struct VoxWalk {
  float trans = 1.0f, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum_head = 0.f;
  // the two halves of a step, for a kernel that stores a and w in between
  __device__ __forceinline__ float weight(float a) {
    const float w = a * trans;
    trans = trans * ((1.0f - a) + 1e-10f);
    return w;
  }
  __device__ __forceinline__ void add(float w, float c0, float c1, float c2, bool last) {
    acc0 = acc0 + w * c0;
    acc1 = acc1 + w * c1;
    acc2 = acc2 + w * c2;
    if (!last) wsum_head = wsum_head + w;
  }
  __device__ __forceinline__ float step(float a, float c0, float c1, float c2, bool last) {
    const float w = weight(a);
    add(w, c0, c1, c2, last);
    return w;
  }
  __device__ __forceinline__ void finish(int bg_kind, float* __restrict__ out) const {
    const float sky = bg_kind == NA_BG_WHITE ? 1.0f - wsum_head : 0.f;
    out[0] = acc0 + sky; out[1] = acc1 + sky; out[2] = acc2 + sky;
  }
};

// ------------------------------------------------------------------------------------ gather
// one thread per sample, one 16-byte row store (+ sh [N] = s with the view-dependent head).  The RGB head's instantiation is pinned to
// the 6 waves per SIMD it had as a kernel of its own (72 VGPRs; left alone the allocator takes 91 for the same instructions).
template <int K, bool SH = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(K < 0 ? 6 : 1, K < 0 ? 6 : 8)))
void plv_sample_kernel(const float* __restrict__ pts, const float* __restrict__ rays, const float* __restrict__ ts, int64_t R, int64_t N,
                       VoxGrid g, const float* __restrict__ den, const float* __restrict__ rgb, float* __restrict__ raw,
                       float* __restrict__ sh) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    float Y[SH_MAX_K], px, py, pz, v[5];
    plv_ray_basis<K>(rays, n % R, Y);
    vox_position(pts, rays, ts, R, n, px, py, pz);
    vox_gather<K, SH>(px, py, pz, g, den, rgb, Y, v);
    *(float4*)(raw + n * 4) = make_float4(v[0], v[1], v[2], v[3]);
    if constexpr (K >= 0 && !SH) sh[n] = v[4];
  }
}

// ------------------------------------------------------------------------------------ gather: gradient w.r.t. the positions
// g_pts[n, a] = (1 / voxel_len) sum_u (dw_u / dxyz_a) v_u with the per-corner value
//   v_u = ((g_raw[n, 0] den[row_u] + g_raw[n, 1] rgb[row_u, 0]) + g_raw[n, 2] rgb[row_u, 1]) + g_raw[n, 3] rgb[row_u, 2]
//         (+ g_sh[n] sum_k Y_k rgb[row_u, 3 + k] with the view-dependent head; SH: d_uc in the place of rgb[row_u, c], no g_sh),
// g_a <- g_a + (dw_u / dxyz_a) v_u in corner order, then the division.  In the reference only xyz = (p - centre of corner 0) /
// voxel_len depends on p -- the floors and both clamps carry no gradient -- so the derivative is the one of the polynomial this cell's
// weights are (vox_dweight), inside the grid and in the extrapolated region alike.  A gather (no atomics), one thread per sample.
// A non-finite coordinate makes the whole row NaN (one NaN fraction alone would leave the other two axes' sums finite).
template <int K, bool SH = false>
__global__ __launch_bounds__(256) void plv_backward_pts_kernel(const float* __restrict__ pts, const float* __restrict__ rays, int64_t R,
                                                               int64_t N, VoxGrid g, const float* __restrict__ den,
                                                               const float* __restrict__ rgb, const float* __restrict__ g_raw,
                                                               const float* __restrict__ g_sh, float* __restrict__ g_pts) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    float Y[SH_MAX_K];
    plv_ray_basis<K>(rays, n % R, Y);
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    const float4 gv = *(const float4*)(g_raw + n * 4);
    float gs = 0.f;
    if constexpr (K >= 0 && !SH) gs = g_sh[n];
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = vox_row(c, u, g.S);
      float dx, dy, dz, v;
      if constexpr (SH) {
        float d[3];
        sh_contract_row<K>(rgb + row * Plv<K, true>::C, Y, d);
        v = ((gv.x * den[row] + gv.y * d[0]) + gv.z * d[1]) + gv.w * d[2];
      } else {
        float q[Plv<K>::C];
        plv_load_row<K>(rgb + row * Plv<K>::C, q);
        v = ((gv.x * den[row] + gv.y * q[0]) + gv.z * q[1]) + gv.w * q[2];
        if constexpr (K >= 0) v = v + gs * plv_contract<K>(q, Y);
      }
      vox_dweight(c, u, dx, dy, dz);
      gx = gx + dx * v;
      gy = gy + dy * v;
      gz = gz + dz * v;
    }
    const bool bad = (c.x != c.x) | (c.y != c.y) | (c.z != c.z);
    const float nan = __builtin_nanf("");
    g_pts[n * 3] = bad ? nan : gx / g.vl;
    g_pts[n * 3 + 1] = bad ? nan : gy / g.vl;
    g_pts[n * 3 + 2] = bad ? nan : gz / g.vl;
  }
}

// ------------------------------------------------------------------------------------ scatter-add
// Corner u of sample n receives w_u [g_raw[n, 0] | g_raw[n, 1..3] | g_sh[n] Y_k]: 1 + C sums per grid row, 4 with the RGB head, 29 at
// K = 4, on voxel_scatter.h's table.  1024 rows x 29 sums x 8 B do not fit a CU's 160 KiB, so the table comes in two geometries:
//   variant 1 (FULL)  whole rows in the table, as many rows as fit 60 KiB (two workgroups per CU): fp32 mode keeps 4-byte
//                     entries (512 rows at K = 4), the deterministic mode 8-byte fixed-point entries (256 rows)
//   variant 2 (LEAD)  1024 rows x 4 sums x 8 B for [density | rgb]; the SH block goes straight to the global accumulators.  This
//                     is the RGB head's table (it has no SH block).
// NA_PLV_SCATTER (voxel.hip) picks the variant na_voxel_plv_sample_backward runs (DESIGN.md 3p has the times of both).
constexpr int PLV_LDS_BUDGET = 60 * 1024;  // table bytes of a workgroup: two workgroups share a CU's 160 KiB

// rows of a table of `sums` entries of `entry` bytes (and a 4-byte tag) inside the budget: a power of two, 1024 at most
constexpr int plv_table_rows(int sums, int entry, int r = 1) {
  return (r * 2 * (sums * entry + 4) <= PLV_LDS_BUDGET && r < 1024) ? plv_table_rows(sums, entry, r * 2) : r;
}

template <int K, int VARIANT, bool DET> struct PlvTable {
  static constexpr int SUMS = VARIANT == 1 ? 1 + Plv<K>::C : 4;   // sums of a table row
  static constexpr int ENTRY = (DET || VARIANT == 2) ? 8 : 4;     // bytes of a sum
  static constexpr int ROWS = plv_table_rows(SUMS, ENTRY);
  using type = VoxTable<SUMS, typename std::conditional<ENTRY == 8, unsigned long long, float>::type, ROWS, DET>;
};

template <int K, int VARIANT, bool DET>
__global__ __launch_bounds__(256) void plv_backward_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                           const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                           const float* __restrict__ g_raw, const float* __restrict__ g_sh,
                                                           float* __restrict__ g_den, float* __restrict__ g_rgb,
                                                           long long* __restrict__ fix) {
  using Table = typename PlvTable<K, VARIANT, DET>::type;
  constexpr int C = Plv<K>::C, NK = Plv<K>::NK, SUMS = PlvTable<K, VARIANT, DET>::SUMS, ROWS = PlvTable<K, VARIANT, DET>::ROWS;
  const int64_t S3 = (int64_t)g.S * g.S * g.S;
  long long* fix_rgb = DET ? fix + S3 : nullptr;
  long long* fix_den = DET ? fix : nullptr;
  // sum e of grid row id: e = 0 density, e = 1 + c channel c of the rgb row
  auto add_global = [&](uint32_t id, int e, float v) {
    if (e == 0) accumulate(g_den, fix_den, (int64_t)id, v);
    else accumulate(g_rgb, fix_rgb, (int64_t)id * C + (e - 1), v);
  };
  __shared__ uint32_t tags[ROWS];
  __shared__ typename Table::Entry vals[ROWS * SUMS];
  const Table table{tags, vals, fix_den};
  table.clear();
  int64_t n_lo, n_hi;
  dv_run(N, n_lo, n_hi);
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    if (n < n_hi) {
      float Y[SH_MAX_K], px, py, pz;
      plv_ray_basis<K>(rays, n % R, Y);
      vox_position(pts, rays, ts, R, n, px, py, pz);
      const VoxCell c = vox_cell(px, py, pz, g);
      const float4 gv = *(const float4*)(g_raw + n * 4);
      float gs = 0.f;
      if constexpr (K >= 0) gs = g_sh[n];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const uint32_t id = (uint32_t)vox_row(c, u, g.S);
        const float w = vox_weight(c, u);
        const float lead[4] = {w * gv.x, w * gv.y, w * gv.z, w * gv.w};
        const float as = w * gs;
        const int slot = table.find_slot(id);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (slot >= 0) table.add(id, slot, e, lead[e], add_global);
          else add_global(id, e, lead[e]);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const float a = as * Y[k];
          if (VARIANT == 1 && slot >= 0) table.add(id, slot, 4 + k, a, add_global);
          else add_global(id, 4 + k, a);
        }
      }
    }
  }
  table.flush([&](uint32_t id, int e, typename Table::Entry v) {
    if (v == 0) return;  // (most rows of a wide table hold no SH sums)
    const int64_t at = e == 0 ? (int64_t)id : (int64_t)id * C + (e - 1);
    table.put(e == 0 ? g_den : g_rgb, e == 0 ? fix_den : fix_rgb, at, v);
  });
}

template <int K, int VARIANT>
static void plv_launch_backward(unsigned wg, hipStream_t s, const float* pts, const float* rays, const float* ts, int64_t R, int64_t N,
                                VoxGrid g, const float* g_raw, const float* g_sh, float* g_den, float* g_rgb, long long* fix) {
  if (fix != nullptr)
    hipLaunchKernelGGL((plv_backward_kernel<K, VARIANT, true>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_den, g_rgb, fix);
  else
    hipLaunchKernelGGL((plv_backward_kernel<K, VARIANT, false>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_sh, g_den, g_rgb, fix);
}

// ------------------------------------------------------------------------------------ scatter-add, SH head
// Corner u of sample n receives w_u [g_raw[n, 0] | (w_u g_raw[n, 1 + c]) Y_k]: 1 + C = 1 + 3 NK sums per grid row, 76 at K = 4 -- whole
// rows at the 60 KiB budget leave 128 table rows in fp32 and 64 in fixed point, where the narrower heads have 512 .. 1024.  Two
// geometries, one kernel body (PASSES x CPP = 3 channel blocks):
//   variant 1 (ROWS)      one pass, whole rows [density | 3 blocks] in the table
//   variant 2 (CHANNELS)  three passes over the workgroup's run, one per colour channel, the table holding [density | ONE block]: a third
//                         of the sums per row buys up to four times the rows (512 / 256 at K = 4), for cells, weights and basis
//                         computed three times; the density sum rides in pass 0
// Every sum has one home whatever the geometry, and the deterministic mode adds integers only: the variants agree bit for bit there.
// NA_SH_SCATTER / NA_SH_SCATTER_DET (voxel.hip) pick the variant of each mode (DESIGN.md 3s has the times of both).
template <int K, int VARIANT, bool DET> struct ShTable {
  static constexpr int NK = Plv<K, true>::NK, CPP = VARIANT == 1 ? 3 : 1, PASSES = 3 / CPP;  // channel blocks per pass
  static constexpr int SUMS = 1 + CPP * NK, ENTRY = DET ? 8 : 4;
  static constexpr int ROWS = plv_table_rows(SUMS, ENTRY);
  using type = VoxTable<SUMS, typename std::conditional<DET, unsigned long long, float>::type, ROWS, DET>;
};

template <int K, int VARIANT, bool DET>
__global__ __launch_bounds__(256) void sh_backward_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                          const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                          const float* __restrict__ g_raw, float* __restrict__ g_den,
                                                          float* __restrict__ g_rgb, long long* __restrict__ fix) {
  using Geo = ShTable<K, VARIANT, DET>;
  using Table = typename Geo::type;
  constexpr int NK = Geo::NK, C = 3 * NK, CPP = Geo::CPP, SUMS = Geo::SUMS, ROWS = Geo::ROWS;
  const int64_t S3 = (int64_t)g.S * g.S * g.S;
  long long* fix_rgb = DET ? fix + S3 : nullptr;
  long long* fix_den = DET ? fix : nullptr;
  __shared__ uint32_t tags[ROWS];
  __shared__ typename Table::Entry vals[ROWS * SUMS];
  const Table table{tags, vals, fix_den};
  int64_t n_lo, n_hi;
  dv_run(N, n_lo, n_hi);
  for (int pass = 0; pass < Geo::PASSES; ++pass) {
    const int c0 = pass * CPP;  // first colour channel of this pass
    // sum e of a table row of this pass: e = 0 density, e = 1 + cc NK + k coefficient k of channel c0 + cc
    auto add_global = [&](uint32_t id, int e, float v) {
      if (e == 0) accumulate(g_den, fix_den, (int64_t)id, v);
      else accumulate(g_rgb, fix_rgb, (int64_t)id * C + c0 * NK + (e - 1), v);
    };
    if (pass > 0) __syncthreads();  // (the flush of the pass before has read the table)
    table.clear();
    for (int64_t base = n_lo; base < n_hi; base += 256) {
      const int64_t n = base + threadIdx.x;
      if (n < n_hi) {
        float Y[SH_MAX_K], px, py, pz;
        plv_ray_basis<K>(rays, n % R, Y);
        vox_position(pts, rays, ts, R, n, px, py, pz);
        const VoxCell c = vox_cell(px, py, pz, g);
        const float4 gv = *(const float4*)(g_raw + n * 4);
        float gc[CPP];
        if constexpr (CPP == 3) { gc[0] = gv.y; gc[1] = gv.z; gc[2] = gv.w; }
        else gc[0] = pass == 0 ? gv.y : pass == 1 ? gv.z : gv.w;
        const VoxRows rows(c, g.S);
#pragma unroll 1  // (the body is up to 76 table adds)
        for (int u = 0; u < 8; ++u) {
          const uint32_t id = (uint32_t)rows(u);
          const float w = vox_weight(c, u);
          const int slot = table.find_slot(id);
          if (pass == 0) {
            if (slot >= 0) table.add(id, slot, 0, w * gv.x, add_global);
            else add_global(id, 0, w * gv.x);
          }
#pragma unroll
          for (int cc = 0; cc < CPP; ++cc) {
            const float wg = w * gc[cc];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              const float a = wg * Y[k];
              if (slot >= 0) table.add(id, slot, 1 + cc * NK + k, a, add_global);
              else add_global(id, 1 + cc * NK + k, a);
            }
          }
        }
      }
    }
    table.flush([&](uint32_t id, int e, typename Table::Entry v) {
      if (v == 0) return;
      const int64_t at = e == 0 ? (int64_t)id : (int64_t)id * C + c0 * NK + (e - 1);
      table.put(e == 0 ? g_den : g_rgb, e == 0 ? fix_den : fix_rgb, at, v);
    });
  }
}

template <int K, int VARIANT>
static void sh_launch_backward(unsigned wg, hipStream_t s, const float* pts, const float* rays, const float* ts, int64_t R, int64_t N,
                               VoxGrid g, const float* g_raw, float* g_den, float* g_rgb, long long* fix) {
  if (fix != nullptr)
    hipLaunchKernelGGL((sh_backward_kernel<K, VARIANT, true>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_den, g_rgb, fix);
  else
    hipLaunchKernelGGL((sh_backward_kernel<K, VARIANT, false>), dim3(wg), dim3(256), 0, s, pts, rays, ts, R, N, g, g_raw, g_den, g_rgb, fix);
}

// ------------------------------------------------------------------------------------ eval route, one launch
// One thread per ray walks T in order like composite_kernel (vox_alpha, VoxWalk); the basis is evaluated once per ray and held in
// registers over the walk.  The rows of U steps are gathered first -- their addresses do not depend on the walk -- so 8 U independent
// row loads are in flight before the U dependent updates run: 4 steps with the RGB head, 2 / 1 with the wider rows (or the rows in
// flight leave the registers).  SH: one step, and the colour is the activation of s_c alone.
template <int K, bool SH = false>
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
    VoxWalk walk;
    constexpr int U = K < 0 ? 4 : (K <= 1 && !SH) ? 2 : 1;
    for (int t0 = 0; t0 < T; t0 += U) {
      float raw[U][5];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;  // (clamped: the tail gathers the last step again and ignores it)
        float px, py, pz;
        vox_position(pts, rays, ts, R, (int64_t)t * R + r, px, py, pz);
        vox_gather<K, SH>(px, py, pz, g, den, rgb, Y, raw[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t < T) {
          const float a = vox_alpha(raw[u][0], ts, t, T, nrm);
          const float w = walk.weight(a);
          if (alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = a;
          if (weights_out != nullptr) weights_out[(int64_t)t * R + r] = w;
          const float3 c = vox_colour<K, SH>(raw[u], act_kind);
          walk.add(w, c.x, c.y, c.z, t == T - 1);
        }
      }
    }
    walk.finish(bg_kind, out + r * 3);
  }
}

}  // namespace na
