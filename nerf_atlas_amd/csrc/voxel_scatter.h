// The scatter-add machinery of every operator that adds rows of sums into the S^3 rows of a voxel grid: na_voxel_sample_backward and
// na_voxel_plv_sample_backward (voxel_plv.h), na_dyn_voxel_warp_backward (dyn_voxel.hip), na_dyn_voxel_spline_len_backward
// (spline_len.hip) and na_dyn_voxel_jac_quad_backward (dyn_voxel_div.hip), with the per-n dispatch and the shape check of the wide-row units.
//
// The scheme is hash_backward_kernel's (backward.hip): a workgroup of 256 threads takes a CONTIGUOUS run of samples (dv_run) --
// neighbouring rays at one step, which share cells -- sums into a hashed LDS table of ROWS grid rows, flushes it once, and a row that
// finds no slot falls through to the caller's global accumulators, so in exact arithmetic the result does not depend on the table.
// The table is keyed by a multiplicative hash of the row id with kVoxProbes linear probes (`id & (ROWS - 1)` would drop ix and most
// of iy: a workgroup's patch of cells collides with itself, and 84 % of the contributions of a `make voxel` crop reach memory, against
// 33 % with four probes; 32 % is the distinct-cell floor).  A slot is never freed, so an id finds the same slot every time, or none.
// Deterministic mode (na_set_deterministic): EVERY contribution is converted to 2^-40 fixed point on its own and only integers are
// added, in LDS and in memory alike, so the bits do not depend on the order of the samples.
// Probes, workgroups and "no wave merge in front of the table" were build-time switches once; DESIGN.md 3i and
// profiles/voxel/scatter_ab.json have the times of the other values.
#pragma once
#include "voxel_cell.h"

namespace na {

constexpr int kVoxProbes = 4;  // slots of the table an id may take
constexpr int DV_WG = 4096;    // workgroups at most: a workgroup's run is ceil(N / DV_WG) samples rounded up to whole rounds of 256
// rows of a table of W 8-byte sums: the table and its tags stay inside 64 KB, two workgroups per CU of 160 KB LDS (62 KB at W = 31)
constexpr int dv_rows(int W) { return W <= 7 ? 1024 : W <= 13 ? 512 : 256; }
constexpr int dv_log2(int v) { return v <= 1 ? 0 : 1 + dv_log2(v / 2); }

// samples [lo, hi) of this workgroup: whole rounds of 256
__device__ __forceinline__ void dv_run(int64_t N, int64_t& lo, int64_t& hi) {
  const int64_t per = ((N + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;
  lo = blockIdx.x * per;
  hi = lo + per < N ? lo + per : N;
}

// The table of one workgroup (256 threads): ROWS rows of SUMS entries; `tags` [ROWS] and `vals` [ROWS * SUMS] are the kernel's
// __shared__ arrays.  E = unsigned long long serves both modes (fixed-point integers, or an fp32 sum in the low word of a zeroed
// entry); E = float is an fp32-only table of half the bytes (fix is not looked at).
template <int SUMS, class E, int NROWS, bool DET = false>
struct VoxTable {
  using Entry = E;
  static constexpr int ROWS = NROWS, SHIFT = 32 - dv_log2(ROWS);
  static constexpr bool WIDE = sizeof(E) == 8;
  static_assert((WIDE || !DET) && (ROWS & (ROWS - 1)) == 0 && ROWS * (SUMS * (int)sizeof(E) + 4) <= 65536,
                "a power of two rows; the table and its tags stay inside 64 KB of LDS; fixed point needs 8-byte entries");
  uint32_t* tags;
  E* vals;
  const long long* fix;  // non-null: the deterministic mode, 2^-40 fixed-point sums (DET: the kernel knows it at compile time)
  __device__ __forceinline__ bool det() const { return DET || fix != nullptr; }

  __device__ __forceinline__ void clear() const {
    for (int i = threadIdx.x; i < ROWS; i += 256) tags[i] = 0xffffffffu;
    for (int i = threadIdx.x; i < ROWS * SUMS; i += 256) vals[i] = (E)0;
    __syncthreads();
  }

  // hit(slot) at the slot of grid row id and true, or false: kVoxProbes linear probes from the id's hash
  template <class Hit>
  __device__ __forceinline__ bool probe(uint32_t id, Hit&& hit) const {
    const uint32_t home = (id * 2654435761u) >> SHIFT;
#pragma unroll
    for (int p = 0; p < kVoxProbes; ++p) {
      const uint32_t slot = (home + p) & (ROWS - 1);
      const uint32_t old = atomicCAS(&tags[slot], 0xffffffffu, id);
      if (old == 0xffffffffu || old == id) {
        hit((int)slot);
        return true;
      }
    }
    return false;
  }

  // the slot of grid row id, or -1
  __device__ __forceinline__ int find_slot(uint32_t id) const {
    int slot = -1;
    probe(id, [&](int s) { slot = s; });
    return slot;
  }

  // sum e of a found slot += v.  The one place of the rule: out of the fixed-point range or NaN goes to add_global(id, e, v), the
  // fp32 path, as accumulate() sends it.
  template <class AddGlobal>
  __device__ __forceinline__ void add(uint32_t id, int slot, int e, float v, AddGlobal&& add_global) const {
    if constexpr (!WIDE) {
      atomicAdd(&vals[slot * SUMS + e], v);
    } else {
      if (!det()) atomicAdd((float*)&vals[slot * SUMS + e], v);
      else if (fabsf(v) < 1048576.0f) atomicAdd(&vals[slot * SUMS + e], (unsigned long long)__float2ll_rn(v * kFixScale));
      else add_global(id, e, v);
    }
  }

  // w * sv[0 .. SUMS-1] for one grid row: into its slot, else add_global(id, e, v)
  template <class AddGlobal>
  __device__ __forceinline__ void add_row(uint32_t id, float w, const float (&sv)[SUMS], AddGlobal&& add_global) const {
    const bool found = probe(id, [&](int slot) {
#pragma unroll
      for (int e = 0; e < SUMS; ++e) add(id, slot, e, w * sv[e], add_global);
    });
    if (found) return;
#pragma unroll
    for (int e = 0; e < SUMS; ++e) add_global(id, e, w * sv[e]);
  }

  // after the workgroup's last add: out(id, e, v) for every entry of every occupied row.  The walk is entry by entry, so the lanes of
  // a wave add to consecutive floats of consecutive table rows (segments of 4 SUMS bytes), not one lane per row.
  template <class Out>
  __device__ __forceinline__ void flush(Out&& out) const {
    __syncthreads();
    for (int i = threadIdx.x; i < ROWS * SUMS; i += 256) {
      const int slot = i / SUMS, e = i - slot * SUMS;
      const uint32_t id = tags[slot];
      if (id == 0xffffffffu) continue;
      out(id, e, vals[i]);
    }
  }

  // a flushed entry into memory: the fp32 sum to dst[at], or the integers to fix_dst[at]
  __device__ __forceinline__ void put(float* dst, long long* fix_dst, int64_t at, E v) const {
    if constexpr (!WIDE) {
      atomicAdd(dst + at, v);
    } else {
      if (!det()) atomicAdd(dst + at, __uint_as_float((uint32_t)v));
      else atomicAdd((unsigned long long*)(fix_dst + at), v);
    }
  }
};

// the table of the wide rows (W sums per grid row, 8-byte entries)
template <int W> using DvTable = VoxTable<W, unsigned long long, dv_rows(W)>;

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
