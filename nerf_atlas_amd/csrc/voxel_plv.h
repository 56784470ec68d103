// NeRFVoxel's view-dependent head (PosLinearView.to_voxel, src/refl.py:265-280) as device functions shared by voxel_plv.hip: the grid
// row is [raw rgb (3) | (K+1)^2 coefficients of ONE spherical-harmonic channel], C = 3 + (K+1)^2 floats, and
//     rgb = act(raw_rgb) * (sigmoid(s) / 2 + 0.5),   s = sum_k Y_k(normalize(view)) c_k,   c_k = the interpolated coefficient k.
// Interpolation and expansion are both linear in the grid, and Y depends on the ray only, so the lookup contracts every corner's
// coefficients with the ray's basis as the row arrives: the (K+1)^2 interpolated coefficients never exist.
//
// ASSOCIATION (one function for every route; tests/voxel_plv_ref.py derives the bound from these counts):
//     d_u = fma(Y_k, row_u[3 + k], d_u) for k = 1 .. NK-1 in k order, from d_u = Y_0 * row_u[3]      (coefficients first: NK roundings)
//     s   = s + w_u * d_u for the corners u = 0 .. 7 in corner order, from s = 0                     (a product and a sum per corner)
// Density and the three colour parameters are vox_gather's arithmetic, operation for operation: with all coefficients zero the four
// leading outputs are na_voxel_sample's bits.
// Cells, weights and rows are voxel_cell.h's (the operator's definition and its memory-safety rule): the ids are
// integer-clamped whatever the coordinate is, and a non-finite coordinate makes xyz -- hence every weight and every output of that
// sample -- NaN.
#pragma once
#include "sh_basis.h"
#include "voxel_cell.h"

namespace na {

template <int K> struct Plv {
  static constexpr int NK = (K + 1) * (K + 1);  // coefficients per voxel
  static constexpr int C = 3 + NK;              // floats per grid row: 4, 7, 12, 19, 28
  static constexpr bool ALIGNED = C % 4 == 0;   // rows of 4 C bytes are 16-byte aligned for K = 0, 2, 4 only
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

// d = sum_k Y_k row[3 + k], the association of the header comment
template <int K> __device__ __forceinline__ float plv_contract(const float (&r)[Plv<K>::C], const float (&Y)[SH_MAX_K]) {
  float d = Y[0] * r[3];
#pragma unroll
  for (int k = 1; k < Plv<K>::NK; ++k) d = fmaf(Y[k], r[3 + k], d);
  return d;
}

// the basis of ray r (dirs = rays[:, 3:6], un-normalised: sh_basis normalises with F.normalize's eps like na_sh_shade)
template <int K> __device__ __forceinline__ void plv_ray_basis(const float* __restrict__ rays, int64_t r, float (&Y)[SH_MAX_K]) {
  const float* d = rays + r * 6 + 3;
  sh_basis(K, d[0], d[1], d[2], Y);
}

// v[0] = density, v[1..3] = colour parameters, v[4] = s: the per-sample lookup of every kernel of the head
template <int K>
__device__ __forceinline__ void vox_plv_gather(float px, float py, float pz, const VoxGrid& g, const float* __restrict__ den,
                                               const float* __restrict__ rgb, const float (&Y)[SH_MAX_K], float v[5]) {
  const VoxCell c = vox_cell(px, py, pz, g);
  v[0] = v[1] = v[2] = v[3] = v[4] = 0.f;
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
    v[4] = v[4] + w * d;
  }
}

// (sigmoid(s) / 2 + 0.5) * act(p): pos_linear_combine_kernel's arithmetic behind apply_sigmoid_kind
__device__ __forceinline__ float plv_scale(float s) { return sigmoidf_(s) / 2.0f + 0.5f; }

static int vox_plv_check_grid(const char* who, int S, int order, double grid_radius) {
  NA_REQUIRE(order >= 0 && order <= 4, NA_EINVAL, "%s: order %d outside 0..4", who, order);
  NA_REQUIRE(S >= 2 && S <= 1024 && S % 2 == 0, NA_EINVAL, "%s: resolution %d (even, 2 .. 1024)", who, S);
  NA_REQUIRE(grid_radius > 0 && grid_radius < 1e30, NA_EINVAL, "%s: grid_radius %g", who, grid_radius);
  return NA_OK;
}

}  // namespace na
