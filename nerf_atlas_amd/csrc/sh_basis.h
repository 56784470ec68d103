// The real spherical-harmonic basis of degrees 0..4 as device code shared by sh_head.hip (the sph-har head) and voxel_plv.h's
// kernels (the two per-voxel view-dependent heads: voxel.hip, voxel_fine.hip, voxel_sparse.hip, dyn_voxel_render.hip): one definition, so that every user evaluates the same arithmetic.
#pragma once
#include "common.h"

namespace na {

// ---- real spherical harmonics, degrees 0..4, from their closed forms.  Sign convention of the reference (the m < 0 and odd-m terms
// of its table carry a minus: no Condon-Shortley phase on top), pinned by tests/golden/g20_sh_eval.npz.
constexpr float SH_C0 = 0.28209479177387814f;    // 1 / (2 sqrt(pi))
constexpr float SH_C1 = 0.4886025119029199f;     // sqrt(3 / (4 pi))
constexpr float SH_C2A = 1.0925484305920792f;    // sqrt(15 / pi) / 2
constexpr float SH_C2B = 0.31539156525252005f;   // sqrt(5 / pi) / 4
constexpr float SH_C2C = 0.5462742152960396f;    // sqrt(15 / pi) / 4
constexpr float SH_C3A = 0.5900435899266435f;    // sqrt(35 / (2 pi)) / 4
constexpr float SH_C3B = 2.890611442640554f;     // sqrt(105 / pi) / 2
constexpr float SH_C3C = 0.4570457994644658f;    // sqrt(21 / (2 pi)) / 4
constexpr float SH_C3D = 0.3731763325901154f;    // sqrt(7 / pi) / 4
constexpr float SH_C3E = 1.445305721320277f;     // sqrt(105 / pi) / 4
constexpr float SH_C4A = 2.5033429417967046f;    // 3 sqrt(35 / pi) / 4
constexpr float SH_C4B = 1.7701307697799304f;    // 3 sqrt(35 / (2 pi)) / 4
constexpr float SH_C4C = 0.9461746957575601f;    // 3 sqrt(5 / pi) / 4
constexpr float SH_C4D = 0.6690465435572892f;    // 3 sqrt(5 / (2 pi)) / 4
constexpr float SH_C4E = 0.10578554691520431f;   // 3 / (16 sqrt(pi))
constexpr float SH_C4F = 0.47308734787878004f;   // 3 sqrt(5 / pi) / 8
constexpr float SH_C4G = 0.6258357354491761f;    // 3 sqrt(35 / pi) / 16
constexpr int SH_MAX_K = 25;

// Y[0 .. (order+1)^2) at the direction F.normalize(d, eps 1e-12); every index is a compile-time constant: the array stays in VGPRs
__device__ __forceinline__ void sh_basis(int order, float dx, float dy, float dz, float (&Y)[SH_MAX_K]) {
  const float nrm = fmaxf(sqrtf(dx * dx + dy * dy + dz * dz), 1e-12f);
  const float x = dx / nrm, y = dy / nrm, z = dz / nrm;
#pragma unroll
  for (int k = 0; k < SH_MAX_K; ++k) Y[k] = 0.f;
  Y[0] = SH_C0;
  if (order < 1) return;
  Y[1] = -SH_C1 * y;
  Y[2] = SH_C1 * z;
  Y[3] = -SH_C1 * x;
  if (order < 2) return;
  const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
  Y[4] = SH_C2A * xy;
  Y[5] = -SH_C2A * yz;
  Y[6] = SH_C2B * (2.f * zz - xx - yy);
  Y[7] = -SH_C2A * xz;
  Y[8] = SH_C2C * (xx - yy);
  if (order < 3) return;
  Y[9] = -SH_C3A * y * (3.f * xx - yy);
  Y[10] = SH_C3B * xy * z;
  Y[11] = -SH_C3C * y * (4.f * zz - xx - yy);
  Y[12] = SH_C3D * z * (2.f * zz - 3.f * xx - 3.f * yy);
  Y[13] = -SH_C3C * x * (4.f * zz - xx - yy);
  Y[14] = SH_C3E * z * (xx - yy);
  Y[15] = -SH_C3A * x * (xx - 3.f * yy);
  if (order < 4) return;
  Y[16] = SH_C4A * xy * (xx - yy);
  Y[17] = -SH_C4B * yz * (3.f * xx - yy);
  Y[18] = SH_C4C * xy * (7.f * zz - 1.f);
  Y[19] = -SH_C4D * yz * (7.f * zz - 3.f);
  Y[20] = SH_C4E * (zz * (35.f * zz - 30.f) + 3.f);
  Y[21] = -SH_C4D * xz * (7.f * zz - 3.f);
  Y[22] = SH_C4F * (xx - yy) * (7.f * zz - 1.f);
  Y[23] = -SH_C4B * xz * (xx - 3.f * yy);
  Y[24] = SH_C4G * (xx * (xx - 3.f * yy) - yy * (3.f * xx - yy));
}

}  // namespace na
