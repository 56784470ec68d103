// The reference's 8-neighbour grid lookup (grid_coords_trilin_weights, src/nerf.py:493-515) as device functions shared by every voxel unit:
// cell membership and xyz are the reference's fp32 chain, operation for operation (voxel.hip's header comment).  The lookup itself
// (vox_gather) and the kernels of a voxel model are voxel_plv.h's, the scatter table is voxel_scatter.h's.
#pragma once
#include "common.h"
#include <math.h>

namespace na {

// fp32 images of the reference's Python doubles (src/nerf.py:427-428, 500, 506)
struct VoxGrid {
  float vl;    // voxel_len = grid_radius * 2 / S
  float h;     // 0.5 * voxel_len
  float gr;    // grid_radius
  float cmax;  // grid_radius - voxel_len / 2
  float half;  // S / 2 (S even: an integer)
  int S;
};

static VoxGrid vox_grid(int S, double grid_radius) {
  const double vl = grid_radius * 2 / S;
  VoxGrid g;
  g.vl = (float)vl; g.h = (float)(0.5 * vl); g.gr = (float)grid_radius; g.cmax = (float)(grid_radius - vl / 2);
  g.half = (float)(S / 2); g.S = S;
  return g;
}

// id of a (clamped) centre.  Memory safety is unconditional: the float is brought into 0 .. S-1 by selects (a NaN fails both
// comparisons' "keep" side and becomes 0), converted, and clamped again as an integer.
__device__ __forceinline__ int vox_id(float c, const VoxGrid& g) {
  float f = floorf(c / g.vl + 1e-10f) + g.half;
  const float top = (float)(g.S - 1);
  f = f >= 0.f ? (f <= top ? f : top) : 0.f;
  const int i = (int)f;
  return min(max(i, 0), g.S - 1);
}

// one axis: ids of the lower / upper neighbour and the fraction x
__device__ __forceinline__ void vox_axis(float p, const VoxGrid& g, int& ilo, int& ihi, float& x) {
  const float nlo = clamp_keep_nan(p - g.h, -g.gr, g.gr);  // (-h) + p
  const float nhi = clamp_keep_nan(g.h + p, -g.gr, g.gr);
  const float clo = clamp_keep_nan((floorf(nlo / g.vl + 1e-10f) + 0.5f) * g.vl, -g.cmax, g.cmax);
  const float chi = clamp_keep_nan((floorf(nhi / g.vl + 1e-10f) + 0.5f) * g.vl, -g.cmax, g.cmax);
  x = (p - clo) / g.vl;
  // a non-finite coordinate (NaN; Inf, whose neighbours clamp to finite centres and leave x = +-Inf) is made NaN here: the
  // reference's weights are then a mixture of +-Inf and NaN whose sum is NaN or +-Inf depending on the signs of the corner
  // values -- this operator's outputs are NaN for that sample whatever the grid holds
  x = fabsf(x) <= 3.4028234663852886e38f ? x : __builtin_nanf("");
  ilo = vox_id(clo, g);
  ihi = vox_id(chi, g);
}

struct VoxCell { int ix[2], iy[2], iz[2]; float x, y, z; };

__device__ __forceinline__ VoxCell vox_cell(float px, float py, float pz, const VoxGrid& g) {
  VoxCell c;
  vox_axis(px, g, c.ix[0], c.ix[1], c.x);
  vox_axis(py, g, c.iy[0], c.iy[1], c.y);
  vox_axis(pz, g, c.iz[0], c.iz[1], c.z);
  return c;
}

// trilinear_weights (src/nerf.py:363-369): (to_val(x, bit 0) * to_val(y, bit 1)) * to_val(z, bit 2)
__device__ __forceinline__ float vox_weight(const VoxCell& c, int u) {
  const float wx = (u & 1) ? c.x : 1.f - c.x, wy = (u & 2) ? c.y : 1.f - c.y, wz = (u & 4) ? c.z : 1.f - c.z;
  return (wx * wy) * wz;
}

// d w_u / d xyz: (+-(wy wz), +-(wx wz), +-(wx wy)), + when corner u takes the upper cell on that axis.  One product each, then the
// sign; what the callers form from it (g += d * v in the position gradients, ((v0 gx + v1 gy) + v2 gz) / vl in dv_tangent) is theirs.
__device__ __forceinline__ void vox_dweight(const VoxCell& c, int u, float& gx, float& gy, float& gz) {
  const float wx = (u & 1) ? c.x : 1.f - c.x, wy = (u & 2) ? c.y : 1.f - c.y, wz = (u & 4) ? c.z : 1.f - c.z;
  const float yz = wy * wz, xz = wx * wz, xy = wx * wy;
  gx = (u & 1) ? yz : -yz; gy = (u & 2) ? xz : -xz; gz = (u & 4) ? xy : -xy;
}

__device__ __forceinline__ int64_t vox_row(const VoxCell& c, int u, int S) {
  return ((int64_t)c.ix[u & 1] * S + c.iy[(u >> 1) & 1]) * S + c.iz[(u >> 2) & 1];
}

// position of sample n = t * R + r: explicit, or o + t d as na_compute_pts forms it (an fp32 multiply, then an fp32 add)
__device__ __forceinline__ void vox_position(const float* __restrict__ pts, const float* __restrict__ rays, const float* __restrict__ ts,
                                             int64_t R, int64_t n, float& px, float& py, float& pz) {
  if (pts != nullptr) {
    px = pts[n * 3]; py = pts[n * 3 + 1]; pz = pts[n * 3 + 2];
    return;
  }
  const float* ry = rays + (n % R) * 6;
  const float tt = ts[n / R];
  px = ry[0] + tt * ry[3]; py = ry[1] + tt * ry[4]; pz = ry[2] + tt * ry[5];
}

static int vox_check_grid(const char* who, int S, int C, double grid_radius) {
  NA_REQUIRE(C == 3, NA_EUNSUPPORTED, "%s: C = %d colour parameters per voxel (3 has a kernel)", who, C);
  NA_REQUIRE(S >= 2 && S <= 1024 && S % 2 == 0, NA_EINVAL, "%s: resolution %d (even, 2 .. 1024)", who, S);
  NA_REQUIRE(grid_radius > 0 && grid_radius < 1e30, NA_EINVAL, "%s: grid_radius %g", who, grid_radius);
  return NA_OK;
}

}  // namespace na
