// The scatter-add machinery of the operators that add "wide rows" of sums into the S^3 rows of DynamicNeRFVoxel's grids, shared by
// dyn_voxel.hip (na_dyn_voxel_warp_backward: W = 1 + 3(n-1) sums per row) and spline_len.hip (na_dyn_voxel_spline_len_backward:
// W = 3(n-1)), with the per-n dispatch and the shape check both units use.
//
// The scheme is voxel_backward_kernel's: a workgroup of 256 threads takes a contiguous run of samples (dv_run), sums into a hashed
// LDS table of ROWS wide rows (multiplicative hash, NA_DV_PROBES linear probes, a slot is never freed), flushes it once, and a row
// that finds no slot falls through to the caller's global accumulators.  A slot is 8 bytes per sum (the fixed-point mode's integers;
// the fp32 mode uses the low word), so ROWS shrinks with W to keep the table and its tags inside 64 KB -- two workgroups per CU of
// 160 KB LDS: 1024 rows for W <= 7, 512 for W <= 13, 256 up to W = 31 (62 KB).  The flush walks the table element by element, so the
// lanes of a wave add to consecutive floats of consecutive table rows (segments of 4 W bytes), not one lane per row.
// Deterministic mode: every contribution to 2^-40 fixed point on its own, as voxel_backward_kernel.
#pragma once
#include "voxel_cell.h"

namespace na {

#ifndef NA_DV_PROBES
#define NA_DV_PROBES 4
#endif
constexpr int DV_WG = 4096;  // workgroups at most: a workgroup's run is ceil(N / DV_WG) samples rounded up to whole rounds of 256
constexpr int dv_rows(int W) { return W <= 7 ? 1024 : W <= 13 ? 512 : 256; }
constexpr int dv_log2(int v) { return v <= 1 ? 0 : 1 + dv_log2(v / 2); }

// samples [lo, hi) of this workgroup: whole rounds of 256
__device__ __forceinline__ void dv_run(int64_t N, int64_t& lo, int64_t& hi) {
  const int64_t per = ((N + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  lo = blockIdx.x * per;
  hi = lo + per < N ? lo + per : N;
}

// the table of one workgroup (256 threads); `tags` [ROWS] and `vals` [ROWS * W] are the kernel's __shared__ arrays
template <int W>
struct DvTable {
  static constexpr int ROWS = dv_rows(W), SHIFT = 32 - dv_log2(ROWS);
  static_assert(ROWS * W * 8 + ROWS * 4 <= 65536, "the table and its tags stay inside 64 KB of LDS");
  uint32_t* tags;
  unsigned long long* vals;
  const long long* fix;  // non-null: the deterministic mode, 2^-40 fixed-point sums

  __device__ __forceinline__ void clear() const {
    for (int i = threadIdx.x; i < ROWS; i += 256) tags[i] = 0xffffffffu;
    for (int i = threadIdx.x; i < ROWS * W; i += 256) vals[i] = 0ull;
    __syncthreads();
  }

  // w * sv[0 .. W-1] for one grid row: the slot of the id (NA_DV_PROBES linear probes from its hash; a slot is never freed, so an id
  // finds the same slot every time, or none), else add_global(id, e, v)
  template <class AddGlobal>
  __device__ __forceinline__ void add_row(uint32_t id, float w, const float (&sv)[W], AddGlobal&& add_global) const {
    const uint32_t home = (id * 2654435761u) >> SHIFT;
#pragma unroll
    for (int p = 0; p < NA_DV_PROBES; ++p) {
      const uint32_t row = (home + p) & (ROWS - 1);
      const uint32_t old = atomicCAS(&tags[row], 0xffffffffu, id);
      if (old == 0xffffffffu || old == id) {
#pragma unroll
        for (int e = 0; e < W; ++e) {
          const float v = w * sv[e];
          if (fix == nullptr) atomicAdd((float*)&vals[row * W + e], v);
          else if (fabsf(v) < 1048576.0f) atomicAdd(&vals[row * W + e], (unsigned long long)__float2ll_rn(v * kFixScale));
          else add_global(id, e, v);  // (out of the fixed-point range, NaN: the fp32 path, as accumulate() does)
        }
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < W; ++e) add_global(id, e, w * sv[e]);
  }

  // after the workgroup's last add_row: out(id, e, slot) for every element of every occupied row
  template <class Out>
  __device__ __forceinline__ void flush(Out&& out) const {
    __syncthreads();
    for (int i = threadIdx.x; i < ROWS * W; i += 256) {
      const int row = i / W, e = i - row * W;
      const uint32_t id = tags[row];
      if (id == 0xffffffffu) continue;
      out(id, e, vals[i]);
    }
  }
};

static int dv_check(const char* who, int64_t N, int S, int n_ctrl, double grid_radius) {
  NA_REQUIRE(N >= 0, NA_EINVAL, "%s: bad shape N=%lld", who, (long long)N);
  NA_REQUIRE(n_ctrl >= 2 && n_ctrl <= 11, NA_EUNSUPPORTED, "%s: spline %d (2 .. 11 control points: 3 (n - 1) <= 32 channels per voxel)", who,
             n_ctrl);
  return vox_check_grid(who, S, 3, grid_radius);
}

#define NA_DV_DISPATCH(N_CTRL, LAUNCH) \
  switch (N_CTRL) {                    \
    case 2: LAUNCH(2); break;          \
    case 3: LAUNCH(3); break;          \
    case 4: LAUNCH(4); break;          \
    case 5: LAUNCH(5); break;          \
    case 6: LAUNCH(6); break;          \
    case 7: LAUNCH(7); break;          \
    case 8: LAUNCH(8); break;          \
    case 9: LAUNCH(9); break;          \
    case 10: LAUNCH(10); break;        \
    default: LAUNCH(11); break;        \
  }

}  // namespace na
