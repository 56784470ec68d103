// NeRFVoxel.sparsify (`--voxel-sparsify`): a liveness table over the voxels and a renderer that skips empty space.
//   na_voxel_live_table     keep[v] = !(density[v] < d_thresh) (a NaN density is kept), live[x,y,z] = any keep in the 3 x 3 x 3 window
//                           x .. x+2 (clamped at S-1): vox_axis derives the lower and the upper id of an axis from two separately rounded
//                           floors, which differ by 0, 1 or 2, so the window covers every corner a sample with these LOWER ids can read.
//   na_voxel_live_samples   flags [M,R]: live[ix0, iy0, iz0] of vox_cell's cell, or 1 where a coordinate is not finite
//   na_voxel_mask_rows      out[n,:] = flags[n] ? x[n,:] : (fill0, 0, .., 0): the training route's mask behind the lookups
//   na_voxel_sparse_render  the three one-launch renderers over a shared row or per-ray rows, gathering and walking live steps only
// The table is compare and integer logic only (no transcendental on the device), the test of a sample is one byte read.  A dead sample
// has alpha = weight = 0 and leaves the walk untouched -- what VoxWalk computes for alpha 0: trans ((1 - 0) + 1e-10f) = trans in fp32,
// acc + 0 c = acc -- so with a table of ones every output is voxel_fine_kernel's bit for bit.
//
// Renderer: voxel_fine_kernel's decomposition (L lanes share a ray, one lane walks) with a compaction in front.  Per chunk of L steps:
//   A  lane j forms the position of step t0 + j and its three vox_axis, reads the table byte; a dead step's alpha / weight zeros are
//      stored right there.  One ballot of the (single) wave gives every ray's live bits; the live step indices go, in ascending order,
//      to the ray's FIFO in LDS (a ring of 2 L entries: at most L - 1 wait from the chunk before, at most L arrive).
//   B  once L indices wait (at the last chunk: whatever waits, in two rounds), L lanes take them, run the per-step code of the dense
//      kernel on the ORIGINAL row (vox_ray_point, vox_gather, vox_alpha, vox_colour) and park [alpha | 3 colours]; then one lane walks them.
// The trip counts of both loops depend on M alone, so every thread meets every barrier; LDS does not depend on M.
#include "voxel_plv.h"

namespace na {

constexpr int VSP_BLOCK = 64;  // threads of a workgroup: one wave (the ballot spans the workgroup, the barriers cost nothing)

__device__ __forceinline__ bool vsp_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// the definition of a live sample: the table byte of the cell's LOWER ids, or a non-finite coordinate (which keeps producing NaN)
__device__ __forceinline__ bool vsp_live(float px, float py, float pz, const VoxGrid& g, const uint8_t* __restrict__ live) {
  const VoxCell c = vox_cell(px, py, pz, g);
  const bool bad = !(vsp_finite(px) && vsp_finite(py) && vsp_finite(pz));
  return bad | (live[((int64_t)c.ix[0] * g.S + c.iy[0]) * g.S + c.iz[0]] != 0);
}

// ------------------------------------------------------------------------------------ table
__global__ __launch_bounds__(256) void live_table_kernel(const float* __restrict__ den, int S, float d_thresh, uint8_t* __restrict__ live,
                                                         unsigned long long* __restrict__ count) {
  const int64_t N = (int64_t)S * S * S;
  for (int64_t base = (int64_t)blockIdx.x * 256; base < N; base += (int64_t)gridDim.x * 256) {  // (uniform: the ballot sees whole waves)
    const int64_t n = base + threadIdx.x;
    bool any = false;
    if (n < N) {
      const int z = (int)(n % S), y = (int)((n / S) % S), x = (int)(n / ((int64_t)S * S));
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          for (int k = 0; k < 3; ++k) {
            const int xx = min(x + i, S - 1), yy = min(y + j, S - 1), zz = min(z + k, S - 1);
            any |= !(den[((int64_t)xx * S + yy) * S + zz] < d_thresh);
          }
      live[n] = any ? 1 : 0;
    }
    if (count != nullptr) {
      const unsigned long long m = __ballot(any);
      if ((threadIdx.x & 63) == 0 && m != 0) atomicAdd(count, (unsigned long long)__popcll(m));
    }
  }
}

// ------------------------------------------------------------------------------------ flags of samples
// sample n = t * R + r: explicit pts, or o + ts[r * stride + t] d (stride 0: one shared row) as vox_position forms it
__global__ __launch_bounds__(256) void live_samples_kernel(const float* __restrict__ pts, const float* __restrict__ rays,
                                                           const float* __restrict__ ts, int64_t stride, int64_t R, int64_t N, VoxGrid g,
                                                           const uint8_t* __restrict__ live, uint8_t* __restrict__ flags) {
  for (int64_t n = blockIdx.x * (int64_t)256 + threadIdx.x; n < N; n += (int64_t)gridDim.x * 256) {
    float px, py, pz;
    if (pts != nullptr || stride == 0) {
      vox_position(pts, rays, ts, R, n, px, py, pz);
    } else {
      const float3 p = vox_ray_point(rays + (n % R) * 6, ts[(n % R) * stride + n / R]);
      px = p.x; py = p.y; pz = p.z;
    }
    flags[n] = vsp_live(px, py, pz, g, live) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(256) void mask_rows_kernel(const float* __restrict__ x, const uint8_t* __restrict__ flags, int64_t N, int C,
                                                        float fill0, float* __restrict__ out) {
  const int64_t E = N * C;
  for (int64_t e = blockIdx.x * (int64_t)256 + threadIdx.x; e < E; e += (int64_t)gridDim.x * 256) {
    const int64_t n = e / C;
    out[e] = flags[n] != 0 ? x[e] : (e - n * C == 0 ? fill0 : 0.f);
  }
}

// ------------------------------------------------------------------------------------ renderer
template <int K, bool SH, int L>
__global__ __launch_bounds__(VSP_BLOCK) void voxel_sparse_kernel(const float* __restrict__ rays, const float* __restrict__ ts_ray, int64_t stride,
                                                                 int M, int64_t R, VoxGrid g, const float* __restrict__ den,
                                                                 const float* __restrict__ rgb, const uint8_t* __restrict__ table,
                                                                 int act_kind, int bg_kind, float* __restrict__ alpha_out,
                                                                 float* __restrict__ weights_out, float* __restrict__ out) {
  constexpr int RPB = VSP_BLOCK / L, Q = 2 * L;
  __shared__ float4 park[RPB][L];  // a step as the walk needs it: [alpha | 3 activated colours]
  __shared__ int fifo[RPB][Q];     // live step indices of a ray, ascending, ring of Q
  const int slot = threadIdx.x / L, j = threadIdx.x % L;
  const unsigned long long below = j == 0 ? 0ull : (~0ull >> (64 - j));  // the ray's lanes in front of this one
  const unsigned long long all = ~0ull >> (64 - L);
  for (int64_t base = (int64_t)blockIdx.x * RPB; base < R; base += (int64_t)gridDim.x * RPB) {  // (uniform: every thread meets the barriers)
    const int64_t r = base + slot;
    const bool ray = r < R;
    const int64_t rr = ray ? r : R - 1;  // (a slot past the end computes the last ray again and writes nothing)
    const float* ry = rays + rr * 6;
    const float* row = ts_ray + rr * stride;
    const float nrm = sqrtf((ry[3] * ry[3] + ry[4] * ry[4]) + ry[5] * ry[5]);
    float Y[SH_MAX_K];
    plv_ray_basis<K>(rays, rr, Y);
    VoxWalk walk;
    int head = 0, tail = 0;  // of the ray's FIFO, counted without wrap (the same in all L lanes of the ray)
    for (int t0 = 0; t0 < M; t0 += L) {
      // ---- A: test, store the dead steps' zeros, queue the live ones
      const int t = t0 + j;
      bool on = false;
      if (t < M) {
        const float3 p = vox_ray_point(ry, row[t]);
        on = vsp_live(p.x, p.y, p.z, g, table);
        if (!on && ray) {
          if (alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = 0.f;
          if (weights_out != nullptr) weights_out[(int64_t)t * R + r] = 0.f;
        }
      }
      const unsigned long long bits = (__ballot(on) >> (slot * L)) & all;
      if (on) fifo[slot][(tail + __popcll(bits & below)) % Q] = t;
      tail += __popcll(bits);
      __syncthreads();
      // ---- B: gather and walk L queued steps; the last chunk drains the queue (at most 2 L - 1 wait)
      const bool last = t0 + L >= M;
      for (int round = 0; round < (last ? 2 : 1); ++round) {
        const int waiting = tail - head;
        const int n = last ? (waiting < L ? waiting : L) : (waiting >= L ? L : 0);
        if (j < n) {
          const int tq = fifo[slot][(head + j) % Q];
          const float3 p = vox_ray_point(ry, row[tq]);
          float raw[5];
          vox_gather<K, SH>(p.x, p.y, p.z, g, den, rgb, Y, raw);
          const float a = vox_alpha(raw[0], row, tq, M, nrm);
          const float3 c = vox_colour<K, SH>(raw, act_kind);
          if (ray && alpha_out != nullptr) alpha_out[(int64_t)tq * R + r] = a;
          park[slot][j] = make_float4(a, c.x, c.y, c.z);
        }
        __syncthreads();
        if (j == 0 && ray) {
          for (int u = 0; u < n; ++u) {
            const int tu = fifo[slot][(head + u) % Q];
            const float4 p = park[slot][u];
            const float w = walk.weight(p.x);
            if (weights_out != nullptr) weights_out[(int64_t)tu * R + r] = w;
            walk.add(w, p.y, p.z, p.w, tu == M - 1);
          }
        }
        head += n;
        __syncthreads();  // (the next round overwrites the parked steps, the next chunk the queue)
      }
    }
    if (j == 0 && ray) walk.finish(bg_kind, out + r * 3);
  }
}

}  // namespace na

using namespace na;

extern "C" {

int na_voxel_live_table(const float* densities, int S, float d_thresh, uint8_t* live, int64_t* count, void* stream) {
  const char* who = "na_voxel_live_table";
  if (int rc = vox_check_grid(who, S, 3, 1.0)) return rc;
  NA_REQUIRE(!(d_thresh != d_thresh), NA_EINVAL, "%s: d_thresh is NaN", who);
  NA_REQUIRE(densities, NA_ENULL, "%s: densities is null", who);
  NA_REQUIRE(live, NA_ENULL, "%s: live is null", who);
  hipStream_t s = (hipStream_t)stream;
  if (count != nullptr) {  // (the kernel adds one ballot's population at a time)
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
    NA_REQUIRE(e == hipSuccess, NA_EHIP, "%s: %s", who, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(live_table_kernel, dim3(grid_for((int64_t)S * S * S, 256)), dim3(256), 0, s, densities, S, d_thresh, live,
                     (unsigned long long*)count);
  return check_launch(who);
}

int na_voxel_live_samples(const float* pts, const float* rays, const float* ts, int64_t stride, int M, int64_t R, int S, double grid_radius,
                          const uint8_t* live, uint8_t* flags, void* stream) {
  const char* who = "na_voxel_live_samples";
  NA_REQUIRE(M >= 1 && R >= 0 && stride >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld stride=%lld", who, M, (long long)R, (long long)stride);
  NA_REQUIRE(stride == 0 || stride >= M, NA_EINVAL, "%s: row stride %lld below M=%d", who, (long long)stride, M);
  if (int rc = vox_check_grid(who, S, 3, grid_radius)) return rc;
  if (R == 0) return NA_OK;
  NA_REQUIRE(pts != nullptr || (rays != nullptr && ts != nullptr), NA_ENULL, "%s: needs pts, or rays and ts", who);
  NA_REQUIRE(live, NA_ENULL, "%s: live is null", who);
  NA_REQUIRE(flags, NA_ENULL, "%s: flags is null", who);
  hipLaunchKernelGGL(live_samples_kernel, dim3(grid_for((int64_t)M * R, 256)), dim3(256), 0, (hipStream_t)stream, pts, rays, ts, stride, R,
                     (int64_t)M * R, vox_grid(S, grid_radius), live, flags);
  return check_launch(who);
}

int na_voxel_mask_rows(const float* x, const uint8_t* flags, int64_t N, int C, float fill0, float* out, void* stream) {
  const char* who = "na_voxel_mask_rows";
  NA_REQUIRE(N >= 0 && C >= 1, NA_EINVAL, "%s: bad shape N=%lld C=%d", who, (long long)N, C);
  if (N == 0) return NA_OK;
  NA_REQUIRE(x, NA_ENULL, "%s: x is null", who);
  NA_REQUIRE(flags, NA_ENULL, "%s: flags is null", who);
  NA_REQUIRE(out, NA_ENULL, "%s: out is null", who);
  hipLaunchKernelGGL(mask_rows_kernel, dim3(grid_for(N * C, 256)), dim3(256), 0, (hipStream_t)stream, x, flags, N, C, fill0, out);
  return check_launch(who);
}

int na_voxel_sparse_render(int head, int order, int lanes, int shared_row, const float* rays, int64_t R, const float* ts, int M,
                           const float* densities, const float* rgb, int S, double grid_radius, const uint8_t* live, int act_kind,
                           int bg_kind, float* alpha, float* weights, float* out, void* stream) {
  const char* who = "na_voxel_sparse_render";
  NA_REQUIRE(head >= NA_VOX_HEAD_RGB && head <= NA_VOX_HEAD_SH, NA_EINVAL, "%s: head %d (NA_VOX_HEAD_RGB, _PLV, _SH)", who, head);
  NA_REQUIRE(M >= 1 && R >= 0, NA_EINVAL, "%s: bad shape M=%d R=%lld", who, M, (long long)R);
  const VoxHead h{head, order};
  if (int rc = h.check(who, S, h.row_floats(), grid_radius)) return rc;
  NA_REQUIRE(vox_lanes_ok(lanes), NA_EINVAL, "%s: %d lanes per ray (4, 8, 16, 32, 64)", who, lanes);
  if (int rc = vox_check_kinds(who, act_kind, bg_kind)) return rc;
  NA_REQUIRE(live, NA_ENULL, "%s: live is null (a table of ones renders everything)", who);
  if (R == 0) return NA_OK;
  if (int rc = vox_check_render_ptrs(who, h, rays, ts, "ts", densities, rgb, out)) return rc;
  const VoxGrid g = vox_grid(S, grid_radius);
  const int64_t stride = shared_row ? 0 : M;
  vox_for_head(h, [&](auto k, auto tag) {
    vox_for_lanes(lanes, [&](auto l) {
      constexpr int L = decltype(l)::value;
      hipLaunchKernelGGL((voxel_sparse_kernel<decltype(k)::value, decltype(tag)::value, L>), dim3(grid_for(R, VSP_BLOCK / L)), dim3(VSP_BLOCK), 0,
                         (hipStream_t)stream, rays, ts, stride, M, R, g, densities, rgb, live, act_kind, bg_kind, alpha, weights, out);
    });
  });
  return check_launch(who);
}

}  // extern "C"
