// Alpha compositing over PER-RAY steps, forward and backward: the fine pass of coarse -> fine TRAINING (PlainNeRF.forward_coarse_fine
// with gradients wanted).  na_composite / na_composite_backward take one shared ts [T]; here every ray has its own
// increasing row ts_ray [R, T] -- what na_resample_ts writes and na_render_plain_view_ls_rayts reads.  The per-step arithmetic is
// composite_kernel's (csrc/basic_ops.hip) and composite_backward_kernel's / composite_backward_seg_kernel's (csrc/backward.hip)
// operation for operation, and the backward picks the same decomposition by T, so rows equal to shared steps give the same bits.
//
// Step reads.  density / feat / alpha / weights are step-major ([T, R]: a lane per ray reads a coalesced row per step), the steps are
// ray-major: a lane per ray reading ts_ray[r * T + t] touches 64 cache lines per step.  The rows are therefore read coalesced -- along
// T -- into an LDS tile [rays][steps] with an odd pitch and turned there: lane r then reads column t of row r, bank (r * pitch + t)
// mod 32, conflict-free within each 32-lane half.  A tile is private to its 64 (32) rays: a non-finite step stays in its ray.
//
// The interval floor is a select, not fmaxf: fmaxf(NaN, 1e-5f) = 1e-5f would turn a NaN step into a finite interval.  For every
// other difference (-Inf included) the select returns what fmaxf returns.
#include "common.h"

namespace na {

constexpr int RT_RAYS = 64;             // rays per workgroup of the one-thread-per-ray kernels
constexpr int RT_CH = 32;               // steps per LDS tile of those kernels
constexpr int RT_PITCH = RT_CH + 1;     // (odd: column reads are conflict-free)
constexpr int RT_SEG = 16;              // steps per segment of the segmented backward (CB_SEG of csrc/backward.hip)
constexpr int RT_SEG_MAX_T = 256;       // 16 segments: 64 rays x 8 (T <= 128) or 32 rays x 16 threads, a segment held in registers

__device__ __forceinline__ float floor_step(float d) { return d < 1e-5f ? 1e-5f : d; }

// columns c0 .. c0 + 31 of the rows r0 .. r0 + 63 -> tile[64][33].  64 threads: a half-wave per row, 128 contiguous bytes each.
// Rows beyond R and columns beyond T - 1 re-read the last valid one (their values are never used).
__device__ __forceinline__ void stage_chunk(const float* __restrict__ ts_ray, int T, int64_t R, int64_t r0, int c0, float* tile, int tid) {
  const int col = tid & (RT_CH - 1);
  const int c = c0 + col < T ? c0 + col : T - 1;
#pragma unroll 8
  for (int k = 0; k < RT_RAYS / 2; ++k) {
    const int row = 2 * k + (tid >> 5);
    const int64_t r = r0 + row < R ? r0 + row : R - 1;
    tile[row * RT_PITCH + col] = ts_ray[r * T + c];
  }
}

// ------------------------------------------------------------------------------------------------ positions
// pts[t, r, :] = r_o[r] + ts_ray[r, t] * r_d[r] in compute_pts_kernel's operation order.  A workgroup = 64 rays x 32 steps: the
// steps through the LDS tile, wave w writes the steps w, w + 4, .. of the tile (768 contiguous bytes per step).
__global__ __launch_bounds__(256) void compute_pts_rayts_kernel(const float* __restrict__ rays, int64_t R, const float* __restrict__ ts_ray,
                                                                int T, float* __restrict__ pts) {
  __shared__ float tile[RT_RAYS * RT_PITCH];
  const int tx = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * RT_RAYS;
  const int c0 = blockIdx.y * RT_CH;
  if (w == 0) stage_chunk(ts_ray, T, R, r0, c0, tile, tx);
  __syncthreads();
  const int64_t r = r0 + tx;
  if (r >= R) return;
  const float* ry = rays + r * 6;
  const float o0 = ry[0], o1 = ry[1], o2 = ry[2], d0 = ry[3], d1 = ry[4], d2 = ry[5];
  for (int u = w; u < RT_CH && c0 + u < T; u += 4) {
    const float tt = tile[tx * RT_PITCH + u];
    float* o = pts + ((int64_t)(c0 + u) * R + r) * 3;
    o[0] = o0 + tt * d0;
    o[1] = o1 + tt * d1;
    o[2] = o2 + tt * d2;
  }
}

// ------------------------------------------------------------------------------------------------ forward
// composite_kernel with per-ray steps: one thread per ray walks T in order, rows fetched U = 8 steps at a time; the steps of the
// workgroup's 64 rays come 32 at a time through the tile.  The tile holds the columns c0 + 1 .. c0 + 32 -- the UPPER end of every
// interval of the chunk -- and the lower end is carried in a register, so that no column is staged twice.
template <int C>
__global__ __launch_bounds__(RT_RAYS) void composite_rayts_kernel(const float* __restrict__ density, const float* __restrict__ feat,
                                                                  const float* __restrict__ ts_ray, const float* __restrict__ rays, int T,
                                                                  int64_t R, int density_kind, int bg_kind, float* __restrict__ alpha_out,
                                                                  float* __restrict__ weights_out, float* __restrict__ out, int Crt,
                                                                  const float* __restrict__ sky_rand) {
  __shared__ float tile[RT_RAYS * RT_PITCH];
  const int CC = C > 0 ? C : Crt;
  const int tx = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * RT_RAYS;
  const bool live = r0 + tx < R;
  const int64_t r = live ? r0 + tx : R - 1;
  const float* ry = rays + r * 6 + 3;
  float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
  float trans = 1.0f;
  float acc[C > 0 ? C : 8];
  for (int c = 0; c < CC; ++c) acc[c] = 0.f;
  float wsum_head = 0.f;
  float tcur = ts_ray[r * T];
  const float* trow = tile + tx * RT_PITCH;
  constexpr int U = 8;
  for (int c0 = 0; c0 < T; c0 += RT_CH) {
    __syncthreads();  // (the previous chunk has been consumed)
    stage_chunk(ts_ray, T, R, r0, c0 + 1, tile, tx);
    __syncthreads();
    const int c1 = c0 + RT_CH < T ? c0 + RT_CH : T;
    for (int t0 = c0; t0 < c1; t0 += U) {
      float dv[U], fv[U][C > 0 ? C : 8];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u < T ? t0 + u : T - 1;
        dv[u] = density[(int64_t)t * R + r];
        const float* f = feat + ((int64_t)t * R + r) * CC;
        for (int c = 0; c < CC; ++c) fv[u][c] = f[c];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t < T) {
          const float d = dv[u];
          float sigma = density_kind == NA_DENSITY_SOFTPLUS_M1 ? fast_softplus(d - 1.0f) : (d < 0.f ? 0.f : d);
          const float tn = trow[t - c0];  // ts_ray[r, t + 1] (t = T - 1: the clamped last column, unused)
          float dist = t < T - 1 ? floor_step(tn - tcur) : 1e10f;
          tcur = tn;
          dist = dist * nrm;
          float a = 1.0f - fast_exp(-sigma * dist);
          float w = a * trans;
          trans = trans * ((1.0f - a) + 1e-10f);
          if (live) {
            if (alpha_out != nullptr) alpha_out[(int64_t)t * R + r] = a;
            if (weights_out != nullptr) weights_out[(int64_t)t * R + r] = w;
          }
          for (int c = 0; c < CC; ++c) acc[c] = acc[c] + w * fv[u][c];
          if (t < T - 1) wsum_head = wsum_head + w;
        }
      }
    }
  }
  float sky = bg_kind == NA_BG_WHITE ? 1.0f - wsum_head : bg_kind == NA_BG_RANDOM ? sky_rand[r] * (1.0f - wsum_head) : 0.f;
  if (live)
    for (int c = 0; c < CC; ++c) out[r * CC + c] = acc[c] + sky;
}

// ------------------------------------------------------------------------------------------------ backward, sequential
// composite_backward_kernel with per-ray steps (the formulas: csrc/backward.hip).  The forward sweep stages the chunks upwards
// (upper interval ends, the lower end carried), the backward sweep stages them downwards (lower ends, the upper end carried).
template <int C>
__global__ __launch_bounds__(RT_RAYS) void composite_rayts_backward_kernel(const float* __restrict__ density, const float* __restrict__ feat,
                                                                           const float* __restrict__ ts_ray, const float* __restrict__ rays,
                                                                           int T, int64_t R, int density_kind, int bg_kind,
                                                                           const float* __restrict__ g_out, float* __restrict__ g_density,
                                                                           float* __restrict__ g_feat, const float* __restrict__ sky_rand) {
  __shared__ float tile[RT_RAYS * RT_PITCH];
  const int tx = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * RT_RAYS;
  const bool live = r0 + tx < R;
  const int64_t r = live ? r0 + tx : R - 1;
  const float* ry = rays + r * 6 + 3;
  const float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
  float g[C];
  float gsum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { g[c] = g_out[r * C + c]; gsum += g[c]; }
  const float gsky = bg_kind == NA_BG_WHITE ? gsum : bg_kind == NA_BG_RANDOM ? gsum * sky_rand[r] : 0.f;
  const float* trow = tile + tx * RT_PITCH;
  constexpr int U = 8;
  float trans = 1.0f;
  float tcur = ts_ray[r * T];
  for (int c0 = 0; c0 < T; c0 += RT_CH) {
    __syncthreads();
    stage_chunk(ts_ray, T, R, r0, c0 + 1, tile, tx);
    __syncthreads();
    const int c1 = c0 + RT_CH < T ? c0 + RT_CH : T;
    for (int t0 = c0; t0 < c1; t0 += U) {
      float dv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) dv[u] = density[(int64_t)(t0 + u < T ? t0 + u : T - 1) * R + r];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t < T) {
          const float d = dv[u];
          const float sigma = density_kind == NA_DENSITY_SOFTPLUS_M1 ? softplusf_(d - 1.0f) : (d < 0.f ? 0.f : d);
          const float tn = trow[t - c0];
          float dist = t < T - 1 ? floor_step(tn - tcur) : 1e10f;
          tcur = tn;
          dist *= nrm;
          const float a = 1.0f - expf(-sigma * dist);
          if (live) g_density[(int64_t)t * R + r] = trans;  // scratch: T_t (read back by this thread only)
          trans = trans * ((1.0f - a) + 1e-10f);
        }
      }
    }
  }
  float suffix = 0.f;
  float tnext = 0.f;  // ts_ray[r, t + 1] of the step in hand (t = T - 1 has the closing interval instead)
  for (int c0 = ((T - 1) / RT_CH) * RT_CH; c0 >= 0; c0 -= RT_CH) {
    __syncthreads();
    stage_chunk(ts_ray, T, R, r0, c0, tile, tx);
    __syncthreads();
    const int top = c0 + RT_CH - 1 < T - 1 ? c0 + RT_CH - 1 : T - 1;
    for (int t1 = top; t1 >= c0; t1 -= U) {
      float dv[U], tv[U], cv[U][C];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t1 - u >= c0 ? t1 - u : c0;
        dv[u] = density[(int64_t)t * R + r];
        tv[u] = live ? g_density[(int64_t)t * R + r] : 1.0f;
        const float* ct = feat + ((int64_t)t * R + r) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) cv[u][c] = ct[c];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t1 - u;
        if (t >= c0) {
          const float d = dv[u];
          const float sigma = density_kind == NA_DENSITY_SOFTPLUS_M1 ? softplusf_(d - 1.0f) : (d < 0.f ? 0.f : d);
          const float tt = trow[t - c0];
          float dist = t < T - 1 ? floor_step(tnext - tt) : 1e10f;
          tnext = tt;
          dist *= nrm;
          const float e = expf(-sigma * dist);
          const float a = 1.0f - e;
          const float f = (1.0f - a) + 1e-10f;
          const float Tt = tv[u];
          const float w = a * Tt;
          float G = 0.f;
#pragma unroll
          for (int c = 0; c < C; ++c) {
            G += g[c] * cv[u][c];
            if (live) g_feat[((int64_t)t * R + r) * C + c] = w * g[c];
          }
          if (t < T - 1) G -= gsky;
          const float dLda = G * Tt - suffix / f;
          suffix += G * w;
          const float dsig = density_kind == NA_DENSITY_SOFTPLUS_M1 ? sigmoidf_(d - 1.0f) : (d > 0.f ? 1.f : 0.f);
          if (live) g_density[(int64_t)t * R + r] = dLda * dist * e * dsig;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward, segmented
// composite_backward_seg_kernel with per-ray steps: one thread per (ray, 16-step segment), blockDim = (rays, S).  64 rays x S <= 8
// is the shared-step kernel's shape; 32 rays x S <= 16 (T <= 256) keeps the workgroup at 512 threads, i.e. the same register budget
// for a segment held in registers -- a wave then carries two segments of 32 rays, its loads are 128-byte half rows.  The workgroup's
// rows of ts_ray are ONE contiguous range of rays x T floats: staged flat, fully coalesced, into tile[rays][T | 1].
template <int C>
__global__ __launch_bounds__(512) void composite_rayts_backward_seg_kernel(const float* __restrict__ density, const float* __restrict__ feat,
                                                                           const float* __restrict__ ts_ray, const float* __restrict__ rays,
                                                                           int T, int64_t R, int density_kind, int bg_kind,
                                                                           const float* __restrict__ g_out, float* __restrict__ g_density,
                                                                           float* __restrict__ g_feat, const float* __restrict__ sky_rand) {
  extern __shared__ float rt_lds[];  // tile [NR][pitch] | P [S][NR] | Q [S][NR]
  const int tx = threadIdx.x, seg = threadIdx.y, NR = blockDim.x, S = blockDim.y;
  const int pitch = T | 1;
  float* tile = rt_lds;
  float* P = tile + NR * pitch;
  float* Q = P + S * NR;
  const int64_t r0 = (int64_t)blockIdx.x * NR;
  {
    const int64_t base = r0 * T, last = R * T - 1;
    const int n = NR * T;
    for (int e = seg * NR + tx; e < n; e += NR * S) {
      const int row = e / T, col = e - row * T;
      tile[row * pitch + col] = ts_ray[base + e < last ? base + e : last];
    }
  }
  const int64_t r = r0 + tx;
  const bool live = r < R;
  const int64_t rc = live ? r : R - 1;
  const int t_lo = seg * RT_SEG;
  const float* ry = rays + rc * 6 + 3;
  const float nrm = sqrtf((ry[0] * ry[0] + ry[1] * ry[1]) + ry[2] * ry[2]);
  float g[C];
  float gsum = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c) { g[c] = g_out[rc * C + c]; gsum += g[c]; }
  const float gsky = bg_kind == NA_BG_WHITE ? gsum : bg_kind == NA_BG_RANDOM ? gsum * sky_rand[rc] : 0.f;
  float dv[RT_SEG], cv[RT_SEG][C];
#pragma unroll
  for (int u = 0; u < RT_SEG; ++u) {
    const int t = t_lo + u < T ? t_lo + u : T - 1;
    dv[u] = density[(int64_t)t * R + rc];
    const float* ct = feat + ((int64_t)t * R + rc) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) cv[u][c] = ct[c];
  }
  __syncthreads();  // the tile
  const float* trow = tile + tx * pitch;
  float ev[RT_SEG], fv[RT_SEG], lp[RT_SEG], dist[RT_SEG];
  float run = 1.0f;
#pragma unroll
  for (int u = 0; u < RT_SEG; ++u) {
    const int t = t_lo + u;
    const float d = dv[u];
    const float sigma = density_kind == NA_DENSITY_SOFTPLUS_M1 ? softplusf_(d - 1.0f) : (d < 0.f ? 0.f : d);
    float di = t < T - 1 ? floor_step(trow[t + 1] - trow[t]) : 1e10f;
    di *= nrm;
    dist[u] = di;
    const float e = expf(-sigma * di);
    ev[u] = e;
    const float a = 1.0f - e;
    fv[u] = (1.0f - a) + 1e-10f;
    lp[u] = run;
    if (t < T) run = run * fv[u];
  }
  P[seg * NR + tx] = run;
  __syncthreads();
  float t_start = 1.0f;
  for (int s2 = 0; s2 < seg; ++s2) t_start = t_start * P[s2 * NR + tx];
  float Gv[RT_SEG], Tv[RT_SEG], sl[RT_SEG];
  float run2 = 0.f;
#pragma unroll
  for (int u = RT_SEG - 1; u >= 0; --u) {
    const int t = t_lo + u;
    const float Tt = t_start * lp[u];
    const float w = (1.0f - ev[u]) * Tt;
    float G = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      G += g[c] * cv[u][c];
      if (live && t < T) g_feat[((int64_t)t * R + r) * C + c] = w * g[c];
    }
    if (t < T - 1) G -= gsky;
    Gv[u] = G; Tv[u] = Tt; sl[u] = run2;
    if (t < T) run2 += G * w;
  }
  Q[seg * NR + tx] = run2;
  __syncthreads();
  float suffix0 = 0.f;
  for (int s2 = S - 1; s2 > seg; --s2) suffix0 += Q[s2 * NR + tx];
#pragma unroll
  for (int u = 0; u < RT_SEG; ++u) {
    const int t = t_lo + u;
    if (live && t < T) {
      const float d = dv[u];
      const float dLda = Gv[u] * Tv[u] - (suffix0 + sl[u]) / fv[u];
      const float dsig = density_kind == NA_DENSITY_SOFTPLUS_M1 ? sigmoidf_(d - 1.0f) : (d > 0.f ? 1.f : 0.f);
      g_density[(int64_t)t * R + r] = dLda * dist[u] * ev[u] * dsig;
    }
  }
}

// form: NA_RAYTS_BWD_AUTO picks by T like launch_composite_backward (csrc/backward.hip) up to 128 steps -- sequential for T <= 16,
// 64 rays x S segments for 17 .. 128 -- and goes on segmenting, 32 rays x S, up to 256 (measured at 64 + 128 = 192 steps: DESIGN.md
// 3h); beyond that the sequential kernel, which takes any T.
static bool rayts_seg_ok(int T) { return T > RT_SEG && T <= RT_SEG_MAX_T; }

template <int C>
static int launch_rayts_backward(const float* density, const float* feat, const float* ts_ray, const float* rays, int T, int64_t R,
                                 int density_kind, int bg_kind, const float* rand, const float* g_out, float* g_density, float* g_feat,
                                 int form, hipStream_t stream) {
  const int S = (T + RT_SEG - 1) / RT_SEG;
  if (form == NA_RAYTS_BWD_SEG || (form == NA_RAYTS_BWD_AUTO && rayts_seg_ok(T))) {
    const int NR = S <= 8 ? 64 : 32;
    const size_t lds = ((size_t)NR * (T | 1) + 2 * (size_t)S * NR) * sizeof(float);  // (<= 64 x 129 + 1024 or 32 x 257 + 1024 floats: 37 KiB)
    hipLaunchKernelGGL(composite_rayts_backward_seg_kernel<C>, dim3((unsigned)((R + NR - 1) / NR)), dim3(NR, S), lds, stream, density, feat,
                       ts_ray, rays, T, R, density_kind, bg_kind, g_out, g_density, g_feat, rand);
  } else {
    hipLaunchKernelGGL(composite_rayts_backward_kernel<C>, dim3((unsigned)((R + RT_RAYS - 1) / RT_RAYS)), dim3(RT_RAYS), 0, stream, density,
                       feat, ts_ray, rays, T, R, density_kind, bg_kind, g_out, g_density, g_feat, rand);
  }
  return check_launch("na_composite_rayts_backward");
}

// (the grids are one workgroup per 64 / 32 rays, unsigned: R < 2^36; r * T and t * R + r are 64-bit)
static int rayts_common(const char* who, int T, int64_t R, int density_kind, int bg_kind, const float* rand) {
  NA_REQUIRE(T >= 1 && R >= 0 && R < ((int64_t)1 << 36), NA_EINVAL, "%s: bad shape T=%d R=%lld", who, T, (long long)R);
  NA_REQUIRE(density_kind == 0 || density_kind == 1, NA_EUNSUPPORTED, "%s: density kind %d", who, density_kind);
  NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE || bg_kind == NA_BG_RANDOM, NA_EUNSUPPORTED, "%s: bg kind %d", who, bg_kind);
  NA_REQUIRE(bg_kind != NA_BG_RANDOM || rand != nullptr || R == 0, NA_ENULL, "%s: bg random needs the per-ray draw `rand`", who);
  return NA_OK;
}

}  // namespace na

using namespace na;

extern "C" int na_compute_pts_rayts(const float* rays, int64_t R, const float* ts_ray, int T, float* pts, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0 && R < ((int64_t)1 << 36) && (T + RT_CH - 1) / RT_CH <= 65535, NA_EINVAL,
             "na_compute_pts_rayts: bad shape T=%d R=%lld", T, (long long)R);
  if (R == 0) return NA_OK;
  NA_REQUIRE(rays && ts_ray && pts, NA_ENULL, "na_compute_pts_rayts: null pointer");
  hipLaunchKernelGGL(compute_pts_rayts_kernel, dim3((unsigned)((R + RT_RAYS - 1) / RT_RAYS), (unsigned)((T + RT_CH - 1) / RT_CH)), dim3(256),
                     0, (hipStream_t)stream, rays, R, ts_ray, T, pts);
  return check_launch("na_compute_pts_rayts");
}

extern "C" int na_composite_rayts(const float* density, const float* feat, const float* ts_ray, const float* rays, int T, int64_t R, int C,
                                  int density_kind, int bg_kind, const float* rand, float* out, float* alpha, float* weights, void* stream) {
  const int rc = rayts_common("na_composite_rayts", T, R, density_kind, bg_kind, rand);
  if (rc != NA_OK) return rc;
  NA_REQUIRE(C >= 1 && C <= 8, NA_EINVAL, "na_composite_rayts: bad shape C=%d (C<=8)", C);
  if (R == 0) return NA_OK;
  NA_REQUIRE(density && feat && ts_ray && rays && out, NA_ENULL, "na_composite_rayts: null pointer");
  const dim3 g((unsigned)((R + RT_RAYS - 1) / RT_RAYS)), b(RT_RAYS);
  if (C == 3)
    hipLaunchKernelGGL(composite_rayts_kernel<3>, g, b, 0, (hipStream_t)stream, density, feat, ts_ray, rays, T, R, density_kind, bg_kind,
                       alpha, weights, out, C, rand);
  else
    hipLaunchKernelGGL(composite_rayts_kernel<0>, g, b, 0, (hipStream_t)stream, density, feat, ts_ray, rays, T, R, density_kind, bg_kind,
                       alpha, weights, out, C, rand);
  return check_launch("na_composite_rayts");
}

extern "C" int na_composite_rayts_backward_form(const float* density, const float* feat, const float* ts_ray, const float* rays, int T,
                                                int64_t R, int C, int density_kind, int bg_kind, const float* rand, const float* g_out,
                                                float* g_density, float* g_feat, int form, void* stream) {
  const int rc = rayts_common("na_composite_rayts_backward", T, R, density_kind, bg_kind, rand);
  if (rc != NA_OK) return rc;
  NA_REQUIRE(C == 3 || C == 1, NA_EUNSUPPORTED, "na_composite_rayts_backward: C=%d (1 or 3)", C);
  NA_REQUIRE(form == NA_RAYTS_BWD_AUTO || form == NA_RAYTS_BWD_SEQ || form == NA_RAYTS_BWD_SEG, NA_EINVAL,
             "na_composite_rayts_backward: form %d", form);
  NA_REQUIRE(form != NA_RAYTS_BWD_SEG || rayts_seg_ok(T), NA_EUNSUPPORTED,
             "na_composite_rayts_backward: the segmented form holds 17 .. %d steps (2 .. 16 segments of 16 steps in registers), T=%d",
             RT_SEG_MAX_T, T);
  if (R == 0) return NA_OK;
  NA_REQUIRE(density && feat && ts_ray && rays && g_out && g_density && g_feat, NA_ENULL, "na_composite_rayts_backward: null pointer");
  if (C == 3)
    return launch_rayts_backward<3>(density, feat, ts_ray, rays, T, R, density_kind, bg_kind, rand, g_out, g_density, g_feat, form,
                                    (hipStream_t)stream);
  return launch_rayts_backward<1>(density, feat, ts_ray, rays, T, R, density_kind, bg_kind, rand, g_out, g_density, g_feat, form,
                                  (hipStream_t)stream);
}

extern "C" int na_composite_rayts_backward(const float* density, const float* feat, const float* ts_ray, const float* rays, int T, int64_t R,
                                           int C, int density_kind, int bg_kind, const float* rand, const float* g_out, float* g_density,
                                           float* g_feat, void* stream) {
  return na_composite_rayts_backward_form(density, feat, ts_ray, rays, T, R, C, density_kind, bg_kind, rand, g_out, g_density, g_feat,
                                          NA_RAYTS_BWD_AUTO, stream);
}
