// Training step, round 5: the forward of a 256-wide Linear with the WEIGHTS resident in registers.
//
//   y[N, 256] = act([x0 (256) | x1 (<= 80)]) . W^T + b                 (src/neural_blocks.py:288-296, training mode)
//
// lsnt::kernel<0> (train_gemm.hip) streams the packed W from L2 once per 64-sample tile -- 256 KiB per tile, four times the tile's
// HBM bytes, through the same vector memory path as the row fetches and the stores; it runs a 256 x 256 layer at 3.7 TB/s of its
// 537 MB, and a skip layer [256 | 38] as two passes.  Here the data flow of the input-gradient role of lsbw::kernel (train_bwd.hip):
// a workgroup owns a sample slice and ALL 256 output columns; wave t of its eight holds the fragments of W's rows 32 t .. 32 t + 31
// for ALL k for the whole launch (K = 256: 16 k steps x (hi | lo) = 128 registers; K = 336: 168), so the loop moves nothing
// but the rows: fetched as whole contiguous rows (x1's unaligned 38 / 69 columns as dwords) two stages ahead (one with a second
// source: registers), activated ONCE, split into bf16 hi | lo planes in LDS ([sample][k of the concatenation]: both sources in
// one image, so a skip layer is one pass), 48-63 MFMAs per wave and stage, the 32 x 256 result through an LDS tile out as whole
// rows (+ bias).  (The first version split the OUTPUT columns over two workgroups like lsbw does for dW's sake: each half
// converted all of x0, and the Cody-Waite sin twice per element made sin layers slower than lsnt -- 159 against 147 us.)
// The two waves of a SIMD run in antiphase (one converts / stores while the other multiplies).
// Same three bf16 products per k, fp32 accumulation, k ascending like lsnt: last-bit differences at most (the bias is added at the
// end here), pinned at 2e-6 of the largest value by tests/test_gpu_train_gemm.py like the other kernel pairs.
#include <atomic>
#include <type_traits>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "train_shared.h"

namespace na {
namespace lsfw {
constexpr int SS = 32;                  // samples per stage
constexpr int KMAX = 336;               // 256 + 80
constexpr int OP = 1040;                // row pitch of the output tile (256 floats + 4: 260 dwords = 4 mod 64)
constexpr int OT = SS * OP;
// MODE 0: a 256 wide source; 1: + a narrow second source (a skip layer); 2: a narrow source alone (an init Linear: 38 / 69 columns)
template <int MODE> struct Geo {
  static constexpr bool X0 = MODE != 2, X1 = MODE != 0;
  static constexpr int KOFF = X0 ? 256 : 0;            // column of the image where the narrow source starts
  static constexpr int KTOT = KOFF + (X1 ? KMAX - 256 : 0);
  static constexpr int P = KTOT * 2 + 16;              // row pitch of a plane: 132 / 172 / 44 dwords = 4 x odd mod 64: conflict-free b128 reads
  static constexpr int PLANE = SS * P;
  static constexpr int STAGE = 2 * PLANE;              // hi | lo
  static constexpr int LDS = 2 * STAGE + 2 * OT;       // two stage buffers + two output tiles: 131 / 151 KiB
  static constexpr int NK = KTOT / 16;                 // k steps (a wave holds them all): 16 / 21 / 5
};

struct Args {
  const float* x0;   // [N, 256]
  const float* x1;   // [N, in1] or null
  const char* wp;    // packed W [256, K] (layout of lsnt::pack_many_kernel)
  const float* bias; // [256] or null
  float* y;          // [N, 256]
  int in1, NCH, nks, nsl, xcd_map;
  int out;           // output columns: 256, or (NOUT instantiations: the out Linears, 256 -> 65 / 3) <= 128
  int64_t N;
};

// NOUT: a narrow output (<= 128 columns, unaligned rows): column tiles past it idle, the tile leaves as dwords
template <int ACT, int MODE, bool NOUT = false>
__global__ __launch_bounds__(512) void kernel(Args g) {
  using G = Geo<MODE>;
  constexpr bool X0 = G::X0, X1 = G::X1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slice = blockIdx.x;
  const int64_t nst_all = (g.N + SS - 1) / SS;
  const int64_t per = (nst_all + g.nsl - 1) / g.nsl;
  const int64_t st0 = slice * per;
  const int nst = (int)((st0 + per <= nst_all ? per : (nst_all > st0 ? nst_all - st0 : 0)));
  char* const otile = smem + 2 * G::STAGE;

  const int c4 = tid & 63, r0 = tid >> 6;    // x0: piece c4 (4 columns) of rows r0 + 8 j, j = 0..3
  const int xc = tid & 31, xr0 = tid >> 5;   // x1: piece xc of rows xr0 + 16 j, j = 0..1
  const uint32_t o0 = (uint32_t)((r0 * 256 + 4 * c4) * 4);
  uint32_t o1[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) o1[e] = (X1 && 4 * xc + e < g.in1) ? (uint32_t)((xr0 * g.in1 + 4 * xc + e) * 4) : lsnt::OOB;
  f32x4 a0[4], a1[X1 ? 1 : 4], b0[2], b1[X1 ? 1 : 2];  // (X1: one prefetch set -- 168 registers of W leave no room for two)
  auto stage_rsrc = [&](const float* base, int ld, int st) __attribute__((always_inline)) {
    const int64_t m0 = (st >= 0 && st < nst) ? (st0 + st) * SS : g.N;
    return lsnt::tile_rsrc(base, ld, m0, g.N, g.wp);
  };
  auto load = [&](f32x4 (&a)[4], f32x4 (&b)[2], int st) __attribute__((always_inline)) {  // (both sets have this shape when they exist)
    if constexpr (X0) {
      const __amdgpu_buffer_rsrc_t r0s = stage_rsrc(g.x0, 256, st);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r0s, o0, 8 * j * 256 * 4, 0));
    }
    if constexpr (X1) {
      const __amdgpu_buffer_rsrc_t r1s = stage_rsrc(g.x1, g.in1, st);
      // (one 16-byte load per piece whatever the row length -- 4-byte aligned raw-buffer loads are legal and range-checked per dword;
      // the elements of the next row a piece brings along are zeroed at conversion)
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r1s, o1[0], 16 * j * g.in1 * 4, 0));
    }
  };
  const int ro0 = r0 * G::P + c4 * 8, ro1 = xr0 * G::P + (G::KOFF + 4 * xc) * 2;
  auto convert = [&](const f32x4 (&a)[4], const f32x4 (&b)[2], char* buf) __attribute__((always_inline)) {
    if constexpr (X0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4 v = a[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = tact(v[e], ACT);
        bf16x4 hi, lo;
        split4(v, hi, lo);
        char* p = buf + ro0 + 8 * j * G::P;
        *(bf16x4*)p = hi;
        *(bf16x4*)(p + G::PLANE) = lo;
      }
    }
    if constexpr (X1) {
      if (4 * xc < KMAX - 256) {  // (columns 256 .. 335 of the image: 20 pieces per row)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          f32x4 v = b[j];
#pragma unroll
          for (int e = 1; e < 4; ++e) v[e] = o1[e] != lsnt::OOB ? v[e] : 0.f;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = tact(v[e], ACT);
          bf16x4 hi, lo;
          split4(v, hi, lo);
          char* p = buf + ro1 + 16 * j * G::P;
          *(bf16x4*)p = hi;
          *(bf16x4*)(p + G::PLANE) = lo;
        }
      }
    }
  };
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  const int ncol = tid & 127, nrow0 = tid >> 7;   // NOUT: element (row nrow0 + 4 j, column ncol)
  if (g.bias != nullptr) {
    if constexpr (NOUT) {}  // (added in the accumulators: below)
    else {
#pragma unroll
      for (int e = 0; e < 4; ++e) bias4[e] = g.bias[4 * c4 + e];
    }
  }
  // y of stage st: the tile + bias, as whole row pieces (the thread's pieces = the ones it fetches of x0: same offsets)
  auto finish = [&](int st) __attribute__((always_inline)) {
    const __amdgpu_buffer_rsrc_t ry = stage_rsrc(g.y, g.out, st);
    if constexpr (NOUT) {
      const char* ot = otile + (st & 1) * OT + nrow0 * OP + ncol * 4;
      const uint32_t oy = ncol < g.out ? (uint32_t)((nrow0 * g.out + ncol) * 4) : lsnt::OOB;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = *(const float*)(ot + 4 * j * OP);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), ry, oy, 4 * j * g.out * 4, 0);
      }
      return;
    }
    const char* ot = otile + (st & 1) * OT + r0 * OP + c4 * 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x4 v = *(const f32x4*)(ot + 8 * j * OP);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += bias4[e];
      // (row step in the vector offset, soffset 0: build.check_store_data_overwrite, tools/hw/store_soffset_hazard.hip)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ry, o0 + (uint32_t)(8 * j * 256 * 4), 0, 0);
    }
  };

  // this wave's fragments of W: rows 32 wave .. (column tile `wave` of the output), every k step
  constexpr int NK = G::NK;
  bf16x8 wh[NK], wl[NK];
  {
    const char* base = g.wp + (size_t)(wave >> 1) * g.NCH * (2 * lsnt::SEG) + lane * 16;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int ks = i < g.nks ? i : g.nks - 1;  // (slots past nks: a valid address, never used)
      const char* f = (NOUT && 64 * (wave >> 1) >= g.out ? g.wp + lane * 16 : base) + (size_t)(((ks >> 3) * 2 + (wave & 1)) * 8 + (ks & 7)) * 2048;  // (NOUT: column groups past the output do not exist in the stream)
      wh[i] = *(const bf16x8*)f;
      wl[i] = *(const bf16x8*)(f + 1024);
    }
  }
  const int n = lane & 31, hh = lane >> 5;
  const int fro = n * G::P + hh * 16;
  const int oto = n * OP + (32 * wave + 4 * hh) * 4;
  const bool tile_on = !NOUT || 32 * wave < g.out;  // (wave-uniform)
  // NOUT: the accumulators START at the bias, like nrw::kernel<0> which ran these layers before -- the same bits as that kernel
  // (the chaotic D-NeRF recipes of tests/test_gpu_train.py amplify a last-place difference in a forward into another end point)
  float bias_acc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int c = 32 * wave + 8 * (q >> 2) + 4 * hh + (q & 3);
    bias_acc[q] = (NOUT && g.bias != nullptr && c < g.out) ? g.bias[c] : 0.f;
  }
  auto mma = [&](const char* buf, char* ot) __attribute__((always_inline)) {
    if (!tile_on) return;
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = NOUT ? bias_acc[q] : 0.f;
    const char* fr = buf + fro;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      if ((X0 && i < 16) || i < g.nks) {  // (wave-uniform; K = 256: exactly 16)
        const bf16x8 xh = *(const bf16x8*)(fr + i * 32);
        const bf16x8 xl = *(const bf16x8*)(fr + G::PLANE + i * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl[i], xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[i], xl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh[i], xh, acc, 0, 0, 0);
      }
    }
    // register q = column 32 wave + 8 (q >> 2) + 4 hh + (q & 3) of sample n
#pragma unroll
    for (int k = 0; k < 4; ++k) *(f32x4*)(ot + oto + 32 * k) = f32x4{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
  };
  // (X1: every stage's conversion writes ALL 80 columns behind the first source -- zeros past in1 -- so the k steps up to 336 read finite zeros)
  // step s: [finish(s - 1) | convert(s + 1) | fetch] and mma(s), one barrier; waves 0-3 multiply first, waves 4-7 convert first
  // (the two waves of a SIMD in antiphase).  Without a second source the rows are fetched TWO stages ahead (two register sets).
  const bool mfirst = wave < 4;
  if constexpr (MODE == 0) {
    load(a0, b0, 0);
    load(a1, b1, 1);
    convert(a0, b0, smem);
    load(a0, b0, 2);
    __syncthreads();
    for (int s = 0; s < nst; s += 2) {
      if (mfirst) { mma(smem, otile); __builtin_amdgcn_sched_barrier(0); }
      finish(s - 1);
      convert(a1, b1, smem + G::STAGE);
      load(a1, b1, s + 3);
      __builtin_amdgcn_sched_barrier(0);  // (the scheduler sinks the fetches below the MFMAs otherwise)
      if (!mfirst) mma(smem, otile);
      __syncthreads();
      // (The condition gives the control-flow graph a path half A -> half A, and the compiler's waitcnt insertion, which must
      // hold on every path, waits for this half's fetches with vmcnt(7) instead of vmcnt(15): one stage after issue, not two.
      // An unconditional second half, which avoids that, measured the same: 148.8 against 149.6 us.)
      if (s + 1 < nst) {
        if (mfirst) { mma(smem + G::STAGE, otile + OT); __builtin_amdgcn_sched_barrier(0); }
        finish(s);
        convert(a0, b0, smem);
        load(a0, b0, s + 4);
        __builtin_amdgcn_sched_barrier(0);
        if (!mfirst) mma(smem + G::STAGE, otile + OT);
        __syncthreads();
      }
    }
  } else {
    load(a0, b0, 0);
    convert(a0, b0, smem);
    load(a0, b0, 1);
    __syncthreads();
    for (int s = 0; s < nst; s += 2) {
      if (mfirst) { mma(smem, otile); __builtin_amdgcn_sched_barrier(0); }
      finish(s - 1);
      convert(a0, b0, smem + G::STAGE);
      load(a0, b0, s + 2);
      __builtin_amdgcn_sched_barrier(0);
      if (!mfirst) mma(smem, otile);
      __syncthreads();
      if (s + 1 < nst) {
        if (mfirst) { mma(smem + G::STAGE, otile + OT); __builtin_amdgcn_sched_barrier(0); }
        finish(s);
        convert(a0, b0, smem);
        load(a0, b0, s + 3);
        __builtin_amdgcn_sched_barrier(0);
        if (!mfirst) mma(smem + G::STAGE, otile + OT);
        __syncthreads();
      }
    }
  }
  finish(nst - 1);
}

// NA_TRAIN_FUSED_FWD=0: never (the streaming kernel lsnt::kernel<0> for A/B runs).
static bool wanted(int64_t N, int out, int in0, int in1, int act) {
  static const bool off = [] { const char* e = getenv("NA_TRAIN_FUSED_FWD"); return e != nullptr && strcmp(e, "0") == 0; }();
  (void)act;
  const bool wide = in0 == 256 && in1 >= 0 && in1 <= KMAX - 256, narrow = in1 == 0 && in0 >= 1 && in0 <= KMAX - 256;
  const bool nout = out >= 1 && out <= 128 && in0 == 256 && in1 == 0;   // (the out Linears: 256 -> 65 / 3)
  return !off && ((out == 256 && (wide || narrow)) || nout) && N >= 8192;
}

template <int MODE, bool NOUT = false>
static auto pick_act(int act) -> void (*)(Args) {
  if (act == NA_ACT_LEAKY_RELU) return kernel<NA_ACT_LEAKY_RELU, MODE, NOUT>;
  if (act == NA_ACT_SIN) return kernel<NA_ACT_SIN, MODE, NOUT>;
  return kernel<NA_ACT_NONE, MODE, NOUT>;
}

static int launch(Args a, int act, hipStream_t st, const char* what) {
  const int mode = a.x0 == nullptr ? 2 : a.in1 > 0 ? 1 : 0;
  const int K = (mode == 2 ? 0 : 256) + a.in1;
  a.NCH = (K + lsnt::KC - 1) / lsnt::KC;
  if (a.NCH < 2) a.NCH = 2;
  a.nks = (K + 15) / 16;
  const int64_t nst = (a.N + SS - 1) / SS;
  const int cus = lsnt::cu_count();
  int nsl = cus;
  if (nst / 4 < nsl) nsl = (int)(nst / 4 > 0 ? nst / 4 : 1);
  a.nsl = nsl;
  a.xcd_map = 0;
  auto k = a.out != 256 ? pick_act<0, true>(act) : mode == 2 ? pick_act<2>(act) : mode == 1 ? pick_act<1>(act) : pick_act<0>(act);
  const int lds = mode == 2 ? Geo<2>::LDS : mode == 1 ? Geo<1>::LDS : Geo<0>::LDS;
  const int which = 3 * (a.out != 256 ? 3 : mode) + (act == NA_ACT_LEAKY_RELU ? 1 : act == NA_ACT_SIN ? 2 : 0);
  static std::atomic<uint64_t> done[12];
  int dev = 0;
  (void)hipGetDevice(&dev);
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done[which].load(std::memory_order_acquire) & bit)) {
    hipError_t e2 = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e2 != hipSuccess) { set_error("hipFuncSetAttribute: %s", hipGetErrorString(e2)); return NA_EHIP; }
    done[which].fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(k, dim3(nsl), dim3(512), lds, st, a);
  return check_launch(what);
}
}  // namespace lsfw

bool train_fwd_wanted(int64_t N, int out, int in0, int in1, int act) { return lsfw::wanted(N, out, in0, in1, act); }

int train_fwd_launch(const float* x0, int in0, const float* x1, int in1, int64_t N, const void* w_packed, const float* b, int out,
                     int pre_act, float* y, hipStream_t st, const char* what) {
  lsfw::Args a{};
  a.out = out;
  if (in0 == 256) { a.x0 = x0; a.x1 = in1 > 0 ? x1 : nullptr; a.in1 = in1; }
  else { a.x0 = nullptr; a.x1 = x0; a.in1 = in0; }  // a narrow source alone rides in the second source's slot
  a.wp = (const char*)w_packed; a.bias = b; a.y = y; a.N = N;
  return lsfw::launch(a, pre_act, st, what);
}
}  // namespace na
