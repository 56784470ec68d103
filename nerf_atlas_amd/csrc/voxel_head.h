// The colour head of a voxel model as ONE thing on the host side (voxel_plv.h includes this):
//   VoxHead        {kind, order}: the floats of a grid row, the grid checks of an entry point, the alignment rule of the rgb grid
//   vox_for_head   the one place a run-time head becomes the kernels' template parameters <K, SH> (K = -1 the RGB head and the
//                  density-only proposal, 0 .. 4 the order; SH false the pos-linear-view rows, true the spherical-harmonic ones)
//   vox_for_lanes  the same for the lanes per ray of the chunked renderers (voxel_fine.hip, voxel_sparse.hip)
//   vox_check_*    the argument checks the renderers share, in the order every entry point runs them
// Every entry point builds a VoxHead from its own arguments and goes on with these; the kernels never see it.
#pragma once
#include "voxel_cell.h"
#include <type_traits>

namespace na {

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct VoxHead {
  int kind;   // NA_VOX_HEAD_* (include/nerf_atlas_amd.h)
  int order;  // 0 .. 4 of the two view-dependent heads; not read otherwise

  bool view() const { return kind == NA_VOX_HEAD_PLV || kind == NA_VOX_HEAD_SH; }
  // floats of a grid row: 3 | 3 + (order + 1)^2 | 3 (order + 1)^2 (an order outside 0 .. 4, which `check` refuses, counts no coefficients)
  int row_floats() const {
    const int nk = order >= 0 && order <= 4 ? (order + 1) * (order + 1) : 0;
    return kind == NA_VOX_HEAD_PLV ? 3 + nk : kind == NA_VOX_HEAD_SH ? 3 * nk : 3;
  }
  // rows of 4 C bytes are read with 16-byte loads when C % 4 == 0: the grid must then start on a 16-byte boundary
  bool rgb_aligned(const void* rgb) const { return row_floats() % 4 != 0 || aligned16(rgb); }

  // C: the caller's channel count (the RGB head has a kernel for 3 only; the SH head's must match its order; the pos-linear-view
  // head's follows from the order and is not passed).  An entry point without a C argument passes row_floats().
  int check(const char* who, int S, int C, double grid_radius) const {
    if (!view()) return vox_check_grid(who, S, C, grid_radius);
    NA_REQUIRE(order >= 0 && order <= 4, NA_EINVAL, "%s: order %d outside 0..4", who, order);
    NA_REQUIRE(S >= 2 && S <= 1024 && S % 2 == 0, NA_EINVAL, "%s: resolution %d (even, 2 .. 1024)", who, S);
    NA_REQUIRE(grid_radius > 0 && grid_radius < 1e30, NA_EINVAL, "%s: grid_radius %g", who, grid_radius);
    NA_REQUIRE(kind != NA_VOX_HEAD_SH || C == row_floats(), NA_EINVAL,
               "%s: C = %d, the spherical-harmonic head of order %d holds 3 (order + 1)^2 = %d", who, C, order, row_floats());
    return NA_OK;
  }
};

// f(std::integral_constant<int, K>, std::bool_constant<SH>) for the head's kernels; `order` was checked (0 .. 4)
template <bool SH, class F> static void vox_for_order(int order, F&& f) {
  switch (order) {
    case 0: f(std::integral_constant<int, 0>{}, std::bool_constant<SH>{}); break;
    case 1: f(std::integral_constant<int, 1>{}, std::bool_constant<SH>{}); break;
    case 2: f(std::integral_constant<int, 2>{}, std::bool_constant<SH>{}); break;
    case 3: f(std::integral_constant<int, 3>{}, std::bool_constant<SH>{}); break;
    default: f(std::integral_constant<int, 4>{}, std::bool_constant<SH>{}); break;
  }
}
template <class F> static void vox_for_head(const VoxHead& h, F&& f) {
  if (h.kind == NA_VOX_HEAD_PLV) vox_for_order<false>(h.order, f);
  else if (h.kind == NA_VOX_HEAD_SH) vox_for_order<true>(h.order, f);
  else f(std::integral_constant<int, -1>{}, std::false_type{});
}

static bool vox_lanes_ok(int lanes) { return lanes == 4 || lanes == 8 || lanes == 16 || lanes == 32 || lanes == 64; }
// f(std::integral_constant<int, L>); `lanes` was checked (vox_lanes_ok)
template <class F> static void vox_for_lanes(int lanes, F&& f) {
  switch (lanes) {
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{}); break;
  }
}

// the activation and the background of a renderer
static int vox_check_kinds(const char* who, int act_kind, int bg_kind) {
  NA_REQUIRE(act_kind >= NA_SIG_NORMAL && act_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "%s: activation kind %d", who, act_kind);
  NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "%s: bg kind %d", who, bg_kind);
  return NA_OK;
}

// the pointers of a renderer that has rays to render (R > 0), and the alignment of the rgb grid; ts_name: what the entry point calls its steps
static int vox_check_render_ptrs(const char* who, const VoxHead& h, const float* rays, const float* ts, const char* ts_name,
                                 const float* densities, const float* rgb, const float* out) {
  NA_REQUIRE(rays, NA_ENULL, "%s: rays is null", who);
  NA_REQUIRE(ts, NA_ENULL, "%s: %s is null", who, ts_name);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(rgb, NA_ENULL, "%s: rgb is null", who);
  NA_REQUIRE(out, NA_ENULL, "%s: out is null", who);
  NA_REQUIRE(h.rgb_aligned(rgb), NA_EINVAL, "%s: rgb must be 16-byte aligned at order %d", who, h.order);
  return NA_OK;
}

}  // namespace na
