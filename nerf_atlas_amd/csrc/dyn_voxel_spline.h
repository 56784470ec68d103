// DynamicNeRFVoxel's spline evaluation (cubic_bezier / de_casteljau, src/nerf.py:1173-1206) as a device function shared by dyn_voxel.hip
// (na_dyn_voxel_warp) and dyn_voxel_render.hip (na_dyn_voxel_render): one definition, so that both units form dp with the same
// operations in the same order.
#pragma once
#include "common.h"

namespace na {

// the reference's two spline forms on control points b[0 .. NC-1][3] (b[0] = 0); dp <- b(t)
template <int NC>
__device__ __forceinline__ void dv_spline(const float* cp, float t, float dp[3]) {
  const float m1t = 1.f - t;
  if (NC == 4) {
    // (k * coeffs).sum(dim=0) with coeffs[0] = 0: k0 * 0 is the first addend
    const float m1t_sq = m1t * m1t, t_sq = t * t;
    const float k0 = m1t_sq * m1t, k1 = (3.f * m1t_sq) * t, k2 = (3.f * t_sq) * m1t, k3 = t_sq * t;
#pragma unroll
    for (int a = 0; a < 3; ++a) dp[a] = ((k0 * 0.f + k1 * cp[a]) + k2 * cp[3 + a]) + k3 * cp[6 + a];
    return;
  }
  float b[NC][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b[0][a] = 0.f;
#pragma unroll
    for (int k = 1; k < NC; ++k) b[k][a] = cp[3 * (k - 1) + a];
  }
#pragma unroll
  for (int i = 1; i < NC; ++i) {
#pragma unroll
    for (int j = 0; j < NC - i; ++j) {
#pragma unroll
      for (int a = 0; a < 3; ++a) b[j][a] = b[j][a] * m1t + b[j + 1][a] * t;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) dp[a] = b[0][a];
}

// d dp / d control point k, k = 0 .. NC-1: the cubic form's own coefficients, else the Bernstein polynomials by the de Casteljau
// recurrence on the weights (every step a convex combination for t in [0, 1])
template <int NC>
__device__ __forceinline__ void dv_bernstein(float t, float B[NC]) {
  const float m1t = 1.f - t;
  if (NC == 4) {
    const float m1t_sq = m1t * m1t, t_sq = t * t;
    B[0] = m1t_sq * m1t; B[1] = (3.f * m1t_sq) * t; B[2] = (3.f * t_sq) * m1t; B[3] = t_sq * t;
    return;
  }
  B[0] = 1.f;
#pragma unroll
  for (int k = 1; k < NC; ++k) B[k] = 0.f;
#pragma unroll
  for (int i = 1; i < NC; ++i) {
#pragma unroll
    for (int j = i; j >= 1; --j) B[j] = B[j] * m1t + B[j - 1] * t;
    B[0] = B[0] * m1t;
  }
}

}  // namespace na
