// DynamicNeRFVoxel's control points as device functions shared by dyn_voxel.hip, dyn_voxel_render.hip, dyn_voxel_div.hip and
// spline_len.hip: the gather of the interpolated control points (dv_gather) and the spline (cubic_bezier / de_casteljau,
// src/nerf.py:1173-1206: dv_casteljau, dv_spline, dv_bernstein).  One definition of each, so that every unit forms its values with the
// same fp32 operations in the same order (all are built with -ffp-contract=off); the order is written at each function.
#pragma once
#include "voxel_cell.h"

namespace na {

// v . grad w_u of corner u: ((v0 gx + v1 gy) + v2 gz) / vl with vox_dweight's (gx, gy, gz)
__device__ __forceinline__ float dv_tangent(const VoxCell& c, int u, const float v[3], float vl) {
  float gx, gy, gz;
  vox_dweight(c, u, gx, gy, gz);
  return ((v[0] * gx + v[1] * gy) + v[2] * gz) / vl;
}

// The 8 rows of 3(NC-1) control-point floats of a cell, each read once.  Over the corners u = 0 .. 7 in corner order, from 0:
//   VAL: cp[ch]  <- cp[ch]  + w_u q_u[ch]   (w_u = vox_weight)           RIG: rl  <- rl  + w_u rig[row_u]
//   TAN: tcp[ch] <- tcp[ch] + d_u q_u[ch]   (d_u = dv_tangent along v)   RIG: trl <- trl + d_u rig[row_u]
// Outputs of a sum that is not asked for are not touched (pass nullptr).
template <int NC, bool VAL, bool TAN, bool RIG>
__device__ __forceinline__ void dv_gather(const VoxCell& c, const VoxGrid& g, const float* __restrict__ ctrl, const float* __restrict__ rig,
                                          const float* v, float* cp, float* rl, float* tcp, float* trl) {
  constexpr int CH = 3 * (NC - 1);
  float a[VAL ? CH : 1], b[TAN ? CH : 1], ra = 0.f, rb = 0.f;  // (local sums: the outputs are written once)
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    if (VAL) a[ch] = 0.f;
    if (TAN) b[ch] = 0.f;
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t row = vox_row(c, u, g.S);
    const float w = VAL ? vox_weight(c, u) : 0.f, d = TAN ? dv_tangent(c, u, v, g.vl) : 0.f;
    const float* q = ctrl + row * CH;
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      if (VAL) a[ch] = a[ch] + w * q[ch];
      if (TAN) b[ch] = b[ch] + d * q[ch];
    }
    if (RIG) {
      const float r = rig[row];
      if (VAL) ra = ra + w * r;
      if (TAN) rb = rb + d * r;
    }
  }
#pragma unroll
  for (int ch = 0; ch < CH; ++ch) {
    if (VAL) cp[ch] = a[ch];
    if (TAN) tcp[ch] = b[ch];
  }
  if (VAL && RIG) *rl = ra;
  if (TAN && RIG) *trl = rb;
}

// de Casteljau on P[0 .. NP-1][3] at t: m1t = 1 - t, then NP - 1 levels b_j <- b_j m1t + b_{j+1} t on a copy of P; p <- b_0
template <int NP>
__device__ __forceinline__ void dv_casteljau(const float (&P)[NP][3], float t, float p[3]) {
  const float m1t = 1.f - t;
  float b[NP][3];
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int a = 0; a < 3; ++a) b[k][a] = P[k][a];
  }
#pragma unroll
  for (int i = 1; i < NP; ++i) {
#pragma unroll
    for (int j = 0; j < NP - i; ++j) {
#pragma unroll
      for (int a = 0; a < 3; ++a) b[j][a] = b[j][a] * m1t + b[j + 1][a] * t;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = b[0][a];
}

// the Bernstein polynomials of degree NP - 1 at t by the de Casteljau recurrence on the weights, from B = (1, 0, ..):
// B_j <- B_j m1t + B_{j-1} t for j = i .. 1, B_0 <- B_0 m1t (every step a convex combination for t in [0, 1])
template <int NP>
__device__ __forceinline__ void dv_bernstein_levels(float t, float (&B)[NP]) {
  const float m1t = 1.f - t;
  B[0] = 1.f;
#pragma unroll
  for (int k = 1; k < NP; ++k) B[k] = 0.f;
#pragma unroll
  for (int i = 1; i < NP; ++i) {
#pragma unroll
    for (int j = i; j >= 1; --j) B[j] = B[j] * m1t + B[j - 1] * t;
    B[0] = B[0] * m1t;
  }
}

// the reference's two spline forms on control points 1 .. NC-1 (cp[3 (k - 1) + a]) behind the zero control point 0; dp <- b(t).
// NC == 4 is cubic_bezier, every other n de_casteljau.  (The spline-length terms are de_casteljau at n == 4 too: they call
// dv_casteljau themselves.)
template <int NC>
__device__ __forceinline__ void dv_spline(const float* cp, float t, float dp[3]) {
  if (NC == 4) {
    // (k * coeffs).sum(dim=0) with coeffs[0] = 0: k0 * 0 is the first addend
    const float m1t = 1.f - t, m1t_sq = m1t * m1t, t_sq = t * t;
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
  dv_casteljau<NC>(b, t, dp);
}

// d dp / d control point k, k = 0 .. NC-1: the cubic form's own coefficients, else dv_bernstein_levels
template <int NC>
__device__ __forceinline__ void dv_bernstein(float t, float (&B)[NC]) {
  if (NC == 4) {
    const float m1t = 1.f - t, m1t_sq = m1t * m1t, t_sq = t * t;
    B[0] = m1t_sq * m1t; B[1] = (3.f * m1t_sq) * t; B[2] = (3.f * t_sq) * m1t; B[3] = t_sq * t;
    return;
  }
  dv_bernstein_levels<NC>(t, B);
}

}  // namespace na
