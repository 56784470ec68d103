// NeRFVoxel (src/nerf.py:401-524): a dense S^3 grid of density and colour parameters read by the reference's 8-neighbour lookup
// (grid_coords_trilin_weights, src/nerf.py:493-515).  Four operators: the gather (na_voxel_sample), its scatter-add backward
// (na_voxel_sample_backward), its gradient w.r.t. explicit positions (na_voxel_sample_backward_pts) and the eval route as one launch (na_voxel_render: positions -> gather -> activation -> compositing).
//
// The lookup is NOT a textbook trilinear interpolation and is reproduced, not improved:
//   neighbours  p -+ voxel_len / 2 per axis, clamped to +-grid_radius; corner u takes + on axis i when bit i of u is set
//   centres     (floor(n / voxel_len + 1e-10) + 0.5) * voxel_len, clamped to +-(grid_radius - voxel_len / 2)
//   xyz         (p - centre of corner 0) / voxel_len, unclamped: a point outside the grid is EXTRAPOLATED with weights that
//               alternate in sign, grow polynomially and still sum to 1
//   ids         floor(centre / voxel_len + 1e-10) + S / 2 -- always inside 0 .. S-1 because the centres were clamped
// The lower and the upper neighbour come from two independent floors, so on the planes p = (k + 0.5) voxel_len one ulp decides
// between the pairs (k, k+1), (k+1, k+2) and (k, k+2): cell membership is part of the operator's definition and every operation
// up to and including xyz is the reference's fp32 operation in the reference's order (this unit is built with -ffp-contract=off
// and hipcc's correctly rounded division; tests/voxel_ref.py restates the chain in fp32 torch and the g23 fixtures pin it).
#include "voxel_cell.h"

namespace na {

// ------------------------------------------------------------------------------------ gather
// one thread per sample, one 16-byte row store
__global__ __launch_bounds__(256) void voxel_sample_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                           const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                           const float* __restrict__ den, const float* __restrict__ rgb,
                                                           float* __restrict__ raw) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    float px, py, pz, v[4];
    vox_position(pts, rays, ts, R, n, px, py, pz);
    vox_gather(px, py, pz, g, den, rgb, v);
    *(float4*)(raw + n * 4) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

// ------------------------------------------------------------------------------------ gather: gradient w.r.t. the positions
// g_pts[n, a] = (1 / voxel_len) sum_u (dw_u / dxyz_a) (g_raw[n, 0] densities[row_u] + sum_c g_raw[n, 1 + c] rgb[row_u, c]).  In the
// reference only xyz = (p - centre of corner 0) / voxel_len depends on p -- the floors and both clamps carry no gradient -- so the
// derivative is the one of the polynomial this cell's weights are, inside the grid and in the extrapolated region alike:
// dw_u / dx = +-(wy wz), the sign + when corner u takes the upper cell on that axis.  A gather (no atomics), one thread per sample.
// A non-finite coordinate makes the whole row NaN (one NaN fraction alone would leave the other two axes' sums finite).
__global__ __launch_bounds__(256) void voxel_backward_pts_kernel(const float* __restrict__ pts, int64_t N, VoxGrid g,
                                                                 const float* __restrict__ den, const float* __restrict__ rgb,
                                                                 const float* __restrict__ g_raw, float* __restrict__ g_pts) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
    const VoxCell c = vox_cell(pts[n * 3], pts[n * 3 + 1], pts[n * 3 + 2], g);
    const float4 gv = *(const float4*)(g_raw + n * 4);
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int64_t row = vox_row(c, u, g.S);
      const float* q = rgb + row * 3;
      const float v = ((gv.x * den[row] + gv.y * q[0]) + gv.z * q[1]) + gv.w * q[2];
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
// g_densities[row] += w_u g_raw[n, 0], g_rgb[row, :] += w_u g_raw[n, 1:4] for the 8 corners of every sample.
// The pattern of hash_backward_kernel (backward.hip): a workgroup takes a CONTIGUOUS run of samples -- neighbouring rays at one
// step, which share cells -- and sums into a hashed table of VB_ROWS grid rows in LDS, flushed once at the end; a row
// taken by another cell falls through to the global accumulator.  Default mode: fp32 sums go to LDS and memory; with
// NA_VOXEL_MERGE_ROUNDS > 0 the lanes of a wave that share a cell are merged first, per corner (leader rounds, DPP wave total; then
// lane by lane), as hash_backward_kernel does -- on a `make voxel` crop 2 % of the lanes share lane 0's cell and the merge does not pay.
// Deterministic mode (na_set_deterministic): EVERY contribution w_u * g is converted to 2^-40 fixed point on its own and only
// integers are added -- in the wave merge's place each lane adds its own integers to the LDS row -- so the result is bitwise
// independent of the order of the samples, not only of the arrival order of the workgroups.
// Build-time constants, the defaults chosen by tools/voxel_bench.py on camera rays (DESIGN.md 3i has the times of the other values):
#ifndef NA_VOXEL_MERGE_ROUNDS
#define NA_VOXEL_MERGE_ROUNDS 0   // leader rounds of the wave merge (0: none -- it measured 1-2 % slower than none at every table setting)
#endif
#ifndef NA_VOXEL_MAX_WG
#define NA_VOXEL_MAX_WG 4096      // workgroups at most
#endif
#ifndef NA_VOXEL_PROBES
#define NA_VOXEL_PROBES 4         // slots of the LDS table an id may take (linear probing)
#endif
#ifndef NA_VOXEL_LDS_TABLE
#define NA_VOXEL_LDS_TABLE 1      // 0: no table, every (merged) contribution straight to the global accumulators
#endif
constexpr int VB_ROWS = 1024;  // (the hash below takes the top 10 bits)
constexpr int VB_WG = NA_VOXEL_MAX_WG;  // a workgroup's run is ceil(N / VB_WG) samples rounded up to whole rounds of 256
__global__ __launch_bounds__(256) void voxel_backward_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                             const float* __restrict__ ts, int64_t R, int64_t N, VoxGrid g,
                                                             const float* __restrict__ g_raw, float* __restrict__ g_den,
                                                             float* __restrict__ g_rgb, long long* __restrict__ fix) {
  const int64_t S3 = (int64_t)g.S * g.S * g.S;
  long long* fix_rgb = fix != nullptr ? fix + S3 : nullptr;
  auto add_global = [&](uint32_t id, int e, float v) {
    if (e == 0) accumulate(g_den, fix, (int64_t)id, v);
    else accumulate(g_rgb, fix_rgb, (int64_t)id * 3 + (e - 1), v);
  };
#if NA_VOXEL_LDS_TABLE
  __shared__ uint32_t tags[VB_ROWS];
  __shared__ unsigned long long vals[VB_ROWS * 4];  // fp32 sums (low word) or fixed-point sums: [density | 3 colour channels]
  for (int i = threadIdx.x; i < VB_ROWS; i += 256) tags[i] = 0xffffffffu;
  for (int i = threadIdx.x; i < VB_ROWS * 4; i += 256) vals[i] = 0ull;
  __syncthreads();
  // four sums for one grid row.  The table is keyed by a multiplicative hash of the row id with NA_VOXEL_PROBES linear probes (the
  // hash table's own `id & (rows - 1)` would drop ix and most of iy: a workgroup's patch of cells collides with itself, and 84 %
  // of the contributions of a `make voxel` crop reach memory, against 33 % with four probes; 32 % is the distinct-cell floor).  A slot
  // is never freed, so an id finds the same slot every time, or none.
  auto add_row = [&](uint32_t id, float s0, float s1, float s2, float s3) {
    const uint32_t home = (id * 2654435761u) >> 22;  // 10 bits: VB_ROWS
    const float sv[4] = {s0, s1, s2, s3};
    for (int p = 0; p < NA_VOXEL_PROBES; ++p) {
      const uint32_t row = (home + p) & (VB_ROWS - 1);
      const uint32_t old = atomicCAS(&tags[row], 0xffffffffu, id);
      if (old == 0xffffffffu || old == id) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (fix == nullptr) atomicAdd((float*)&vals[row * 4 + e], sv[e]);
          else if (fabsf(sv[e]) < 1048576.0f) atomicAdd(&vals[row * 4 + e], (unsigned long long)__float2ll_rn(sv[e] * kFixScale));
          else add_global(id, e, sv[e]);  // (out of the fixed-point range, NaN: the fp32 path, as accumulate() does)
        }
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) add_global(id, e, sv[e]);
  };
#else
  auto add_row = [&](uint32_t id, float s0, float s1, float s2, float s3) {
    add_global(id, 0, s0); add_global(id, 1, s1); add_global(id, 2, s2); add_global(id, 3, s3);
  };
#endif
  const int64_t per = ((N + gridDim.x - 1) / gridDim.x + 255) / 256 * 256;  // samples of this workgroup: whole rounds
  const int64_t n_lo = blockIdx.x * per, n_hi = n_lo + per < N ? n_lo + per : N;
  for (int64_t base = n_lo; base < n_hi; base += 256) {
    const int64_t n = base + threadIdx.x;
    const bool live = n < n_hi;
    VoxCell c;
    c.ix[0] = c.ix[1] = c.iy[0] = c.iy[1] = c.iz[0] = c.iz[1] = 0;
    c.x = c.y = c.z = 0.f;
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    if (live) {
      float px, py, pz;
      vox_position(pts, rays, ts, R, n, px, py, pz);
      c = vox_cell(px, py, pz, g);
      const float4 gv = *(const float4*)(g_raw + n * 4);
      g0 = gv.x; g1 = gv.y; g2 = gv.z; g3 = gv.w;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const uint32_t id = (uint32_t)vox_row(c, u, g.S);
      const float w = vox_weight(c, u);
      const float a0 = w * g0, a1 = w * g1, a2 = w * g2, a3 = w * g3;
      bool todo = live;
      if (fix == nullptr) {
        for (int round = 0; round < NA_VOXEL_MERGE_ROUNDS; ++round) {
          const uint64_t pending = __ballot(todo);
          if (pending == 0) break;
          const int leader = __ffsll((unsigned long long)pending) - 1;
          const uint32_t lid = __shfl(id, leader);
          const bool mine = todo && id == lid;
          const float s0 = wave_total_lane63(mine ? a0 : 0.f), s1 = wave_total_lane63(mine ? a1 : 0.f);
          const float s2 = wave_total_lane63(mine ? a2 : 0.f), s3 = wave_total_lane63(mine ? a3 : 0.f);
          if ((threadIdx.x & 63) == 63) add_row(lid, s0, s1, s2, s3);
          todo = todo && !mine;
        }
      }
      if (todo) add_row(id, a0, a1, a2, a3);
    }
  }
#if NA_VOXEL_LDS_TABLE
  __syncthreads();
  for (int row = threadIdx.x; row < VB_ROWS; row += 256) {
    const uint32_t id = tags[row];
    if (id == 0xffffffffu) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned long long v = vals[row * 4 + e];
      const int64_t at = e == 0 ? (int64_t)id : (int64_t)id * 3 + (e - 1);
      if (fix == nullptr) atomicAdd((e == 0 ? g_den : g_rgb) + at, __uint_as_float((uint32_t)v));
      else atomicAdd((unsigned long long*)((e == 0 ? fix : fix_rgb) + at), v);
    }
  }
#endif
}

// ------------------------------------------------------------------------------------ eval route, one launch
// One thread per ray walks T in order like composite_kernel (basic_ops.hip) with the same per-step arithmetic on the same
// device functions (common.h fast_softplus / fast_exp; the running product is the reference's cumprod association).  The rows of
// U steps are gathered first -- their addresses do not depend on the walk -- so 8 U independent loads are in flight before the
// U dependent updates run.
__global__ __launch_bounds__(64) void voxel_render_kernel(const float* __restrict__ rays, const float* __restrict__ pts,
                                                          const float* __restrict__ ts, int T, int64_t R, VoxGrid g,
                                                          const float* __restrict__ den, const float* __restrict__ rgb, int act_kind,
                                                          int bg_kind, float* __restrict__ alpha_out, float* __restrict__ weights_out,
                                                          float* __restrict__ out) {
  for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < R; r += (int64_t)gridDim.x * blockDim.x) {
    const float* ry = rays + r * 6 + 3;
    const float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
    float trans = 1.0f, acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, wsum_head = 0.f;
    constexpr int U = 4;
    for (int t0 = 0; t0 < T; t0 += U) {
      float raw[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;  // (clamped: the tail gathers the last step again and ignores it)
        float px, py, pz;
        vox_position(pts, rays, ts, R, (int64_t)t * R + r, px, py, pz);
        vox_gather(px, py, pz, g, den, rgb, raw[u]);
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
          acc0 = acc0 + w * apply_sigmoid_kind(raw[u][1], act_kind);
          acc1 = acc1 + w * apply_sigmoid_kind(raw[u][2], act_kind);
          acc2 = acc2 + w * apply_sigmoid_kind(raw[u][3], act_kind);
          if (t < T - 1) wsum_head = wsum_head + w;
        }
      }
    }
    const float sky = bg_kind == NA_BG_WHITE ? 1.0f - wsum_head : 0.f;
    out[r * 3] = acc0 + sky; out[r * 3 + 1] = acc1 + sky; out[r * 3 + 2] = acc2 + sky;
  }
}

}  // namespace na

using namespace na;

extern "C" {

int na_voxel_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, float* raw, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_sample: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_sample", S, C, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(densities && rgb && raw && (pts || (rays && ts)), NA_ENULL, "na_voxel_sample: null pointer");
  hipLaunchKernelGGL(voxel_sample_kernel, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts, R, N,
                     vox_grid(S, grid_radius), densities, rgb, raw);
  return check_launch("na_voxel_sample");
}

int na_voxel_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                             double grid_radius, float* g_densities, float* g_rgb, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_sample_backward: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_sample_backward", S, C, grid_radius)) return rc;
  const int64_t N = (int64_t)T * R;
  if (N == 0) return NA_OK;
  NA_REQUIRE(g_raw && g_densities && g_rgb && (pts || (rays && ts)), NA_ENULL, "na_voxel_sample_backward: null pointer");
  int rc;
  const size_t S3 = (size_t)S * S * S;
  long long* fix = det_begin(S3 * 4, (hipStream_t)stream, "na_voxel_sample_backward", &rc);
  if (rc != NA_OK) return rc;
  hipLaunchKernelGGL(voxel_backward_kernel, dim3(grid_for(N, 256, VB_WG)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts, R, N,
                     vox_grid(S, grid_radius), g_raw, g_densities, g_rgb, fix);
  if (fix != nullptr) {
    if (int rc2 = det_finish(fix, S3, g_densities, (hipStream_t)stream, "na_voxel_sample_backward")) return rc2;
    return det_finish(fix + S3, S3 * 3, g_rgb, (hipStream_t)stream, "na_voxel_sample_backward");
  }
  return check_launch("na_voxel_sample_backward");
}

int na_voxel_sample_backward_pts(const float* pts, int64_t N, const float* densities, const float* rgb, const float* g_raw, int S, int C,
                                 double grid_radius, float* g_pts, void* stream) {
  NA_REQUIRE(N >= 0, NA_EINVAL, "na_voxel_sample_backward_pts: bad shape N=%lld", (long long)N);
  if (int rc = vox_check_grid("na_voxel_sample_backward_pts", S, C, grid_radius)) return rc;
  if (N == 0) return NA_OK;
  NA_REQUIRE(pts && densities && rgb && g_raw && g_pts, NA_ENULL, "na_voxel_sample_backward_pts: null pointer");
  hipLaunchKernelGGL(voxel_backward_pts_kernel, dim3(grid_for(N, 256)), dim3(256), 0, (hipStream_t)stream, pts, N, vox_grid(S, grid_radius),
                     densities, rgb, g_raw, g_pts);
  return check_launch("na_voxel_sample_backward_pts");
}

int na_voxel_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                    void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_voxel_render: bad shape T=%d R=%lld", T, (long long)R);
  if (int rc = vox_check_grid("na_voxel_render", S, C, grid_radius)) return rc;
  NA_REQUIRE(act_kind >= NA_SIG_NORMAL && act_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "na_voxel_render: activation kind %d", act_kind);
  NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "na_voxel_render: bg kind %d", bg_kind);
  if (R == 0) return NA_OK;
  NA_REQUIRE(rays && ts && densities && rgb && out, NA_ENULL, "na_voxel_render: null pointer");
  hipLaunchKernelGGL(voxel_render_kernel, dim3(grid_for(R, 64)), dim3(64), 0, (hipStream_t)stream, rays, pts, ts, T, R,
                     vox_grid(S, grid_radius), densities, rgb, act_kind, bg_kind, alpha, weights, out);
  return check_launch("na_voxel_render");
}

}  // extern "C"
