// The optimiser step of runner.py:440-458 -- optim.SGD / RMSprop / Adam(weight_decay = --decay) / AdamW, as the reference builds them:
// no momentum, not centered, no amsgrad -- for every parameter tensor by ONE launch.
//
// torch's default (foreach) implementations are one multi-tensor launch per operation, each a read-modify-write of every parameter
// (torch/optim/{sgd,rmsprop,adam}.py::_multi_tensor_*).  Here one launch performs the SAME per-element operations in the same order,
// each rounded to fp32 like the corresponding ATen kernel rounds it; the ATen kernels are compiled with contraction on, this unit
// with -ffp-contract=off, and which multiply-adds ATen contracts is the `fma` mask (tools/optim_probe.py finds it on the GPU,
// tests/test_gpu_optim.py and tests/test_gpu_train.py pin it bit for bit against torch):
//
//   sgd       p = p + a g                                a = -lr                       (bit 3: _foreach_add_(alpha))
//   rmsprop   v = v alpha;  v = v + c (g g)              c = 1 - alpha                 (bit 1: addcmul, g g rounded first)
//             d = sqrt(v) + eps
//             p = p + a (g / d)                          a = -lr                       (bit 2: addcdiv, g / d rounded first)
//   adam      g' = g + wd p                              only with wd != 0             (bit 3: _foreach_add(alpha); g itself is not written)
//             m = m + w (g' - m)                         w = 1 - beta1 < 0.5           (bit 0: lerp)
//             v = v beta2;  v = v + c (g' g')            c = 1 - beta2                 (bit 1)
//             d = sqrt(v) / sqrt(1 - beta2^t) + eps
//             p = p + a (m / d)                          a = -lr / (1 - beta1^t)       (bit 2)
//   adamw     p = p k                                    k = 1 - lr wd, only with wd != 0
//             then adam's four lines on g
//
// The scalars arrive as the doubles torch's Python computes and are rounded to float like ATen's opmath conversion does.
//
// A streaming kernel: a block covers 1024 consecutive elements of one tensor, a thread four of them -- one 16-byte access per array
// where every pointer of the tensor is 16-byte aligned and the four elements exist, element by element otherwise (a ragged tail, a
// view that starts inside its storage).  Every index the kernel forms is below the tensor's numel: block b of tensor e covers
// (b - first[e]) * 1024 .. + 1023 and first[e + 1] - first[e] = ceil(numel[e] / 1024).
#include "common.h"
#include <math.h>

namespace na {

constexpr int kOptimMany = 48;   // tensors per launch: the table travels as the kernel's argument
struct OptimMany {
  float* p[kOptimMany];
  const float* g[kOptimMany];
  float* s0[kOptimMany];         // rmsprop: square_avg; adam / adamw: exp_avg
  float* s1[kOptimMany];         // adam / adamw: exp_avg_sq
  int first[kOptimMany + 1];     // first block of tensor e (a block = 1024 elements)
  int64_t numel[kOptimMany];
  int n, fma;
  float c[NA_OPTIM_MAX_SCALARS]; // the rule's scalars in the order of include/nerf_atlas_amd.h
};

constexpr int kStates[4] = {0, 1, 2, 2};   // state tensors per rule

// DECAY: the weight-decay line of adam (coupled) / adamw (decoupled) is performed (torch skips it for weight_decay == 0, and
// 0 * p is not nothing for a non-finite p)
template <int RULE, bool DECAY>
__device__ __forceinline__ void optim_one(const OptimMany& t, float& p, float g, float& s0, float& s1) {
  if constexpr (RULE == NA_OPTIM_SGD) {
    p = (t.fma & 8) ? fmaf(t.c[0], g, p) : p + t.c[0] * g;
  } else if constexpr (RULE == NA_OPTIM_RMSPROP) {
    float v = s0 * t.c[0];
    const float gg = g * g;
    v = (t.fma & 2) ? fmaf(t.c[1], gg, v) : v + t.c[1] * gg;
    const float d = sqrtf(v) + t.c[2];
    const float q = g / d;
    p = (t.fma & 4) ? fmaf(t.c[3], q, p) : p + t.c[3] * q;
    s0 = v;
  } else {
    if constexpr (DECAY && RULE == NA_OPTIM_ADAMW) p = p * t.c[6];
    if constexpr (DECAY && RULE == NA_OPTIM_ADAM) g = (t.fma & 8) ? fmaf(t.c[6], p, g) : g + t.c[6] * p;
    float m = s0, v = s1;
    const float diff = g - m;
    m = (t.fma & 1) ? fmaf(t.c[0], diff, m) : m + t.c[0] * diff;
    v = v * t.c[1];
    const float gg = g * g;
    v = (t.fma & 2) ? fmaf(t.c[2], gg, v) : v + t.c[2] * gg;
    const float d = sqrtf(v) / t.c[3] + t.c[4];
    const float q = m / d;
    p = (t.fma & 4) ? fmaf(t.c[5], q, p) : p + t.c[5] * q;
    s0 = m; s1 = v;
  }
}

template <int RULE, bool DECAY>
__global__ __launch_bounds__(256) void optim_many_kernel(OptimMany t) {
  constexpr int S = kStates[RULE];
  int e = 0;
  while (e + 1 < t.n && (int)blockIdx.x >= t.first[e + 1]) ++e;   // (<= 48 entries: a scalar walk)
  const int64_t i0 = ((int64_t)blockIdx.x - t.first[e]) * 1024 + threadIdx.x * 4;
  const int64_t n = t.numel[e];
  float* __restrict__ P = t.p[e];
  const float* __restrict__ G = t.g[e];
  float* __restrict__ S0 = S > 0 ? t.s0[e] : nullptr;
  float* __restrict__ S1 = S > 1 ? t.s1[e] : nullptr;
  const uintptr_t align = (uintptr_t)P | (uintptr_t)G | (uintptr_t)S0 | (uintptr_t)S1;   // (a null pointer is aligned)
  if (i0 + 4 <= n && (align & 15) == 0) {
    float4 p = *(const float4*)(P + i0), a = {}, b = {};
    const float4 g = *(const float4*)(G + i0);
    if constexpr (S > 0) a = *(const float4*)(S0 + i0);
    if constexpr (S > 1) b = *(const float4*)(S1 + i0);
    optim_one<RULE, DECAY>(t, p.x, g.x, a.x, b.x); optim_one<RULE, DECAY>(t, p.y, g.y, a.y, b.y);
    optim_one<RULE, DECAY>(t, p.z, g.z, a.z, b.z); optim_one<RULE, DECAY>(t, p.w, g.w, a.w, b.w);
    *(float4*)(P + i0) = p;
    if constexpr (S > 0) *(float4*)(S0 + i0) = a;
    if constexpr (S > 1) *(float4*)(S1 + i0) = b;
  } else {
    for (int64_t i = i0; i < i0 + 4 && i < n; ++i) {
      float p = P[i], a = 0.f, b = 0.f;
      if constexpr (S > 0) a = S0[i];
      if constexpr (S > 1) b = S1[i];
      optim_one<RULE, DECAY>(t, p, G[i], a, b);
      P[i] = p;
      if constexpr (S > 0) S0[i] = a;
      if constexpr (S > 1) S1[i] = b;
    }
  }
}

// The next chunk of the tensor list: up to 48 NON-EMPTY tensors from index `i` on.  Returns the index where it stopped -- the caller
// continues there, so a tensor is part of exactly one launch however many empty ones lie between (an empty tensor does not take a
// slot and is not counted).  The list has been validated by the caller.
static int optim_chunk(int states, int n, int i, float* const* params, const float* const* grads, float* const* state0,
                       float* const* state1, const int64_t* numel, OptimMany& t, int* blocks_out) {
  t.n = 0;
  int blocks = 0;
  for (; i < n && t.n < kOptimMany; ++i) {
    if (numel[i] == 0) continue;
    const int e = t.n++;
    t.p[e] = params[i]; t.g[e] = grads[i]; t.numel[e] = numel[i];
    t.s0[e] = states >= 1 ? state0[i] : nullptr;
    t.s1[e] = states >= 2 ? state1[i] : nullptr;
    t.first[e] = blocks;
    blocks += (int)((numel[i] + 1023) / 1024);
  }
  t.first[t.n] = blocks;
  *blocks_out = blocks;
  return i;
}

template <int RULE, bool DECAY>
static void optim_launch(const OptimMany& t, int blocks, hipStream_t stream) {
  hipLaunchKernelGGL((optim_many_kernel<RULE, DECAY>), dim3(blocks), dim3(256), 0, stream, t);
}

static int optim_step(const char* who, int rule, int n, float* const* params, const float* const* grads, float* const* state0,
                      float* const* state1, const int64_t* numel, const double* scalars, int n_scalars, int fma_mask, void* stream) {
  NA_REQUIRE(rule >= NA_OPTIM_SGD && rule <= NA_OPTIM_ADAMW, NA_EINVAL, "%s: update rule %d", who, rule);
  NA_REQUIRE(n >= 0, NA_EINVAL, "%s: n %d", who, n);
  static const int want[4] = {1, 4, 7, 7};
  NA_REQUIRE(n_scalars == want[rule], NA_EINVAL, "%s: rule %d takes %d scalars, got %d", who, rule, want[rule], n_scalars);
  if (n == 0) return NA_OK;
  const int states = kStates[rule];
  NA_REQUIRE(params && grads && numel && scalars && (states < 1 || state0) && (states < 2 || state1), NA_ENULL, "%s: null pointer", who);
  // validate the whole list before the first launch: a refused call has updated nothing
  int64_t all_blocks = 0;
  for (int i = 0; i < n; ++i) {
    NA_REQUIRE(numel[i] >= 0, NA_EINVAL, "%s: numel[%d] = %lld", who, i, (long long)numel[i]);
    NA_REQUIRE(numel[i] == 0 || (params[i] && grads[i] && (states < 1 || state0[i]) && (states < 2 || state1[i])), NA_ENULL,
               "%s: tensor %d has a null pointer", who, i);
    NA_REQUIRE(numel[i] < (1ll << 40), NA_EINVAL, "%s: too many elements", who);
    all_blocks += (numel[i] + 1023) / 1024;
    NA_REQUIRE(all_blocks < (1ll << 30), NA_EINVAL, "%s: too many elements", who);   // (a launch's grid stays below 2^30 blocks)
  }
  // (adam: scalar 6 is the coupled weight decay; adamw: 1 - lr wd, where 1 means none)
  const bool decay = (rule == NA_OPTIM_ADAM && scalars[6] != 0.0) || (rule == NA_OPTIM_ADAMW && scalars[6] != 1.0);
  for (int i = 0; i < n;) {
    OptimMany t{};
    int blocks = 0;
    i = optim_chunk(states, n, i, params, grads, state0, state1, numel, t, &blocks);
    if (t.n == 0) continue;   // (only empty tensors were left)
    t.fma = fma_mask;
    for (int k = 0; k < n_scalars; ++k) t.c[k] = (float)scalars[k];
    const hipStream_t s = (hipStream_t)stream;
    switch (rule) {
      case NA_OPTIM_SGD: optim_launch<NA_OPTIM_SGD, false>(t, blocks, s); break;
      case NA_OPTIM_RMSPROP: optim_launch<NA_OPTIM_RMSPROP, false>(t, blocks, s); break;
      case NA_OPTIM_ADAM: decay ? optim_launch<NA_OPTIM_ADAM, true>(t, blocks, s) : optim_launch<NA_OPTIM_ADAM, false>(t, blocks, s); break;
      default: decay ? optim_launch<NA_OPTIM_ADAMW, true>(t, blocks, s) : optim_launch<NA_OPTIM_ADAM, false>(t, blocks, s); break;
    }
  }
  return check_launch(who);
}

}  // namespace na

using namespace na;

extern "C" {

int na_optim_step(int rule, int n, float* const* params, const float* const* grads, float* const* state0, float* const* state1,
                  const int64_t* numel, const double* scalars, int n_scalars, int fma_mask, void* stream) {
  return optim_step("na_optim_step", rule, n, params, grads, state0, state1, numel, scalars, n_scalars, fma_mask, stream);
}

int na_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const int64_t* numel, double one_minus_beta1, double beta2, double one_minus_beta2, double bias_correction2_sqrt,
                 double eps, double neg_step_size, int fma_mask, void* stream) {
  const double scalars[7] = {one_minus_beta1, beta2, one_minus_beta2, bias_correction2_sqrt, eps, neg_step_size, 0.0};
  return optim_step("na_adam_step", NA_OPTIM_ADAM, n, params, grads, exp_avg, exp_avg_sq, numel, scalars, 7, fma_mask, stream);
}

}  // extern "C"
