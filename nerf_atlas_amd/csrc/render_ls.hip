// na_render_plain_view_ls: PlainNeRF.forward with the View head (src/nerf.py:326-361, src/refl.py:190-207) as ONE
// kernel on the LAYER-SYNCHRONOUS engine.  Same arithmetic and work items as render_fused.hip
// (a block = 32 consecutive steps of one ray, lane&31 = step, compositing = in-wave scan), different data flow:
//
//  * 8 waves = 4 row groups (64 output rows = two 32-row MFMA tiles) x 2 sample groups (NBLK blocks each).
//  * Activations live in LDS as ready-made MFMA B fragments, [group][block][chunk][lane] x 16 B: the lane that
//    produces 8 values of a chunk is the lane that consumes them, so ds_write_b128 / ds_read_b128 are lane-linear and
//    conflict-free; the implied k permutation is the engine's pi_perm, folded into the weight packing.
//  * A layer = an MFMA phase that is CHUNK-major: per 16-wide k chunk the wave streams its two A fragments straight
//    from global memory into registers (a 4-deep software-prefetched ring that runs across layer, MLP and pass
//    boundaries: no LDS-DMA, no weight ring in LDS) and feeds them to 2 x NBLK MFMAs whose B fragments come from LDS:
//    every LDS fragment read feeds TWO MFMAs (the one-read-per-MFMA structure of mlp_engine.h caps the matrix pipe
//    near 57 %).  All 2 x NBLK accumulator tiles stay in registers until the layer is complete; the activation
//    epilogue then overwrites the LDS fragments in place.
//  * The two sample groups run in ANTIPHASE, one workgroup barrier per phase: while one group streams MFMAs the
//    other runs its epilogue / encoder / compositing (VALU + LDS writes) on the same SIMDs, so VALU work never sits
//    between a wave's own MFMAs and each SIMD always has one MFMA-only wave.
//  * LDS: per group NBLK x (16 hidden + 4 init) chunks = 80 KiB, 160 KiB per workgroup (bf16: NBLK = 4; bf16x3 keeps
//    hi and lo planes: NBLK = 2).  The fifth init chunk of the View MLP (x, y, z, elev, azim) does not fit: every
//    consuming wave rebuilds its fragments in registers (scalar loads of the ray and of its per-ray elev/azim, which a
//    small pre-kernel writes once per ray; ~15 VALU per block) right before the two MFMAs that use them.
//  * `first.out` / `view.out` (65 and 3 rows) run block-per-wave (wave rg = block rg, all out tiles), which is also the
//    assignment of the hash-encoder prologue and of compositing, so density and colour never leave their wave.
//  * Sample group G = 2 * workgroup + g renders the rays G, G + nG, ... one after the other, block by block in step
//    order: the transmittance is carried across blocks (and passes) inside the group -- block partials meet in the
//    group's idle hidden region of LDS -- so there are no per-block partials in HBM and no finalize launch.
//
// Compiled once per precision (-DNA_PREC_INST=0|1|2|3).  Every unit holds its precision's kernels behind one
// render_ls_dispatch_<precision>; the NA_PREC_INST == 0 unit also holds the C entry points, which all go through ONE host
// path: ls_run (validate, fill ls::Args, launch) for the render / rows entries, ls_pack_begin + launch_pack for the pack entries.
#include <atomic>
#include "ls_pack.h"
#if NA_PREC_INST == 3
#include "ls_xsched.h"
#endif

namespace na {

static int no_ls_kernel(const char* what, int precision, int model) {
  set_error("%s: no layer-synchronous kernel for precision %d, model %d", what, precision, model);
  return NA_EUNSUPPORTED;
}

// The instantiations of render_ls_kernel<PREC, MODEL>: every (precision, model) pair that has a kernel is a case here, nothing else launches.
#if NA_PREC_INST == 3
int render_ls_dispatch_f16x(ls::Args& a, hipStream_t s, int model, const char* what) {
  switch (model) {
    case 0: return ls::launch<NA_PREC_F16X, 0>(a, s, what);
    case 1: return ls::launch<NA_PREC_F16X, 1>(a, s, what);
    case 2: return ls::launch<NA_PREC_F16X, 2>(a, s, what);
    case 3: return ls::launch<NA_PREC_F16X, 3>(a, s, what);
    case 4: return ls::launch<NA_PREC_F16X, 4>(a, s, what);
    case 5: return ls::launch<NA_PREC_F16X, 5>(a, s, what);
    case 6: return ls::launch<NA_PREC_F16X, 6>(a, s, what);
    case 7: return ls::launch<NA_PREC_F16X, 7>(a, s, what);
    case 8: return ls::launch<NA_PREC_F16X, 8>(a, s, what);
    default: return no_ls_kernel(what, NA_PREC_F16X, model);
  }
}
#elif NA_PREC_INST == 0
int render_ls_dispatch_bf16(ls::Args& a, hipStream_t s, int model, const char* what) {
  switch (model) {
    case 0: return ls::launch<NA_PREC_BF16, 0>(a, s, what);
    case 1: return ls::launch<NA_PREC_BF16, 1>(a, s, what);
    case 2: return ls::launch<NA_PREC_BF16, 2>(a, s, what);
    case 3: return ls::launch<NA_PREC_BF16, 3>(a, s, what);
    default: return no_ls_kernel(what, NA_PREC_BF16, model);
  }
}
#elif NA_PREC_INST == 1
int render_ls_dispatch_bf16x3(ls::Args& a, hipStream_t s, int model, const char* what) {
  switch (model) {
    case 0: return ls::launch<NA_PREC_BF16X3, 0>(a, s, what);
    case 1: return ls::launch<NA_PREC_BF16X3, 1>(a, s, what);
    case 2: return ls::launch<NA_PREC_BF16X3, 2>(a, s, what);
    case 3: return ls::launch<NA_PREC_BF16X3, 3>(a, s, what);
    case 4: return ls::launch<NA_PREC_BF16X3, 4>(a, s, what);
    case 9: return ls::launch<NA_PREC_BF16X3, 9>(a, s, what);
    default: return no_ls_kernel(what, NA_PREC_BF16X3, model);
  }
}
#elif NA_PREC_INST == 2
int render_ls_dispatch_f16(ls::Args& a, hipStream_t s, int model, const char* what) {
  switch (model) {
    case 0: return ls::launch<NA_PREC_F16, 0>(a, s, what);
    case 1: return ls::launch<NA_PREC_F16, 1>(a, s, what);
    case 2: return ls::launch<NA_PREC_F16, 2>(a, s, what);
    case 3: return ls::launch<NA_PREC_F16, 3>(a, s, what);
    default: return no_ls_kernel(what, NA_PREC_F16, model);
  }
}
#endif
int render_ls_dispatch_bf16(ls::Args& a, hipStream_t s, int model, const char* what);
int render_ls_dispatch_bf16x3(ls::Args& a, hipStream_t s, int model, const char* what);
int render_ls_dispatch_f16(ls::Args& a, hipStream_t s, int model, const char* what);
int render_ls_dispatch_f16x(ls::Args& a, hipStream_t s, int model, const char* what);

}  // namespace na

#if NA_PREC_INST == 0
using namespace na;

#define NA_TRY(expr) do { if (int rc_ = (expr)) return rc_; } while (0)

static int render_ls_dispatch(int precision, int model, ls::Args& a, hipStream_t s, const char* what) {
  switch (precision) {
    case NA_PREC_BF16: return render_ls_dispatch_bf16(a, s, model, what);
    case NA_PREC_BF16X3: return render_ls_dispatch_bf16x3(a, s, model, what);
    case NA_PREC_F16: return render_ls_dispatch_f16(a, s, model, what);
    case NA_PREC_F16X: return render_ls_dispatch_f16x(a, s, model, what);
    default: return no_ls_kernel(what, precision, model);
  }
}

// Which precisions an entry accepts: bit p = NA_PREC_p
constexpr unsigned kAnyPrec = 1u << NA_PREC_BF16 | 1u << NA_PREC_BF16X3 | 1u << NA_PREC_F16 | 1u << NA_PREC_F16X;
constexpr unsigned kF16x = 1u << NA_PREC_F16X, kBf16x3 = 1u << NA_PREC_BF16X3;
static bool accepts(unsigned precisions, int precision) { return precision >= 0 && precision < 32 && (precisions >> precision & 1u); }

// Bytes of the weight stream of schedule `model` (ls_engine.h MODEL 0..9) in `precision`
static size_t ls_stream_bytes(int precision, int model) {
  switch (model) {
    case 1: return ls::packed_bytes(precision, ls::kTinyPairs);
    case 2: return ls::packed_bytes(precision, ls::kViewPairs);
    case 3: return ls::packed_bytes(precision, ls::kSirenPairs);
    case 4: return precision == NA_PREC_F16X ? ls::packed_bytes_x(4) : ls::packed_bytes(precision, ls::kHashMlpPairs);
    case 5: case 6: case 7: case 8: return ls::packed_bytes_x(model);
    default: return ls::packed_bytes(precision);  // 0, and 9 (the training forward reads MODEL 0's stream)
  }
}

// ================================================================================================ render / rows entries
struct LsEntry {
  const char* what;            // the C entry point, for messages
  int model;
  unsigned precisions;
  const char* precision_note;  // behind "precision %d" when the check fails
  bool composites;             // takes sigmoid_kind / bg_kind and writes `out` (the rows entries do neither)
  bool needs_elaz;             // the View MLP's geometry chunk: ray_elaz_kernel fills the head of the workspace
  bool needs_workspace;        // (needs_elaz implies it; without elaz it is MODEL 7 / 8's park scratch: na_render_head_ls_workspace_bytes)
};
enum LsStage { kAfterPointers, kAfterPrecision, kAfterSigmoid, kAfterBg };  // where an entry's own checks sit among the common ones

// The one host path of the engine: validate (common checks in a fixed order, the entry's own through `own(stage)` at their places),
// fill the common fields of `a` (the entry has set what is particular to its MODEL), launch.
template <class Own>
static int ls_run(const LsEntry& e, ls::Args& a, const float* rays, const float* pts, int64_t R, const float* ts, int T, const void* tables,
                  const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                  void* workspace, size_t workspace_bytes, void* stream, bool own_pointers, Own own) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "%s: bad shape T=%d R=%lld", e.what, T, (long long)R);
  if (R == 0) return NA_OK;  // empty batch: a no-op before any pointer check (zero-size tensors carry null pointers)
  NA_REQUIRE(rays && ts && packed && own_pointers && (!e.composites || out) && (!e.needs_workspace || workspace), NA_ENULL,
             "%s: null pointer", e.what);
  NA_TRY(own(kAfterPointers));
  NA_REQUIRE(accepts(e.precisions, precision), NA_EUNSUPPORTED, "%s: precision %d%s", e.what, precision, e.precision_note);
  NA_TRY(own(kAfterPrecision));
  if (e.composites) {
    NA_REQUIRE(sigmoid_kind >= 0 && sigmoid_kind <= NA_SIG_IDENTITY, NA_EUNSUPPORTED, "%s: sigmoid %d", e.what, sigmoid_kind);
    NA_TRY(own(kAfterSigmoid));
    NA_REQUIRE(bg_kind == NA_BG_BLACK || bg_kind == NA_BG_WHITE, NA_EUNSUPPORTED, "%s: bg %d", e.what, bg_kind);
    NA_TRY(own(kAfterBg));
  }
  const size_t need = !e.needs_workspace ? 0 : e.needs_elaz ? na_render_ls_workspace_bytes(T, R) : na_render_head_ls_workspace_bytes(T, R);
  NA_REQUIRE(workspace_bytes >= need, NA_EWORKSPACE, "%s: workspace %zu < %zu bytes", e.what, workspace_bytes, need);
  a.rays = rays; a.ts = ts; a.pts = pts; a.tables = (const float4*)tables;
  a.packed = (const char*)packed; a.packed_size = (uint32_t)ls_stream_bytes(precision, e.model);
  a.alpha = alpha; a.weights = weights; a.out = out; a.bg_kind = bg_kind; a.sigmoid_kind = sigmoid_kind;
  a.R = R; a.T = T; a.nb = (T + 31) / 32;
  a.res = hash_resolutions();
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  if (e.needs_elaz) {
    float* elaz = (float*)ws;
    a.elaz = elaz;
    hipLaunchKernelGGL(ls::ray_elaz_kernel, dim3(grid_for(R, 256, 4096)), dim3(256), 0, (hipStream_t)stream, rays, R, elaz);
    if (NA_LS_TRACE) a.trace = (unsigned long long*)(((uintptr_t)(elaz + R * 2) + 255) & ~(uintptr_t)255);
  } else if (e.needs_workspace) {
    a.park = (float*)ws;
    if (NA_LS_TRACE) a.trace = (unsigned long long*)(ws + ls::kParkBytes);  // (tools/head_trace.py; the base size's per-ray scratch is unused here)
  }
  return render_ls_dispatch(precision, e.model, a, (hipStream_t)stream, e.what);
}
static int no_own_checks(LsStage) { return NA_OK; }

extern "C" size_t na_render_ls_workspace_bytes(int T, int64_t R) {
  if (T < 1 || R < 0) return 0;
  return (size_t)R * 2 * sizeof(float) + 256 + (NA_LS_TRACE ? 4096 + 256 : 0);
}

extern "C" size_t na_render_head_ls_workspace_bytes(int T, int64_t R) {
  if (T < 1 || R < 0) return 0;
  return na_render_ls_workspace_bytes(T, R) + 256 + ls::kParkBytes;
}

// ================================================================================================ pack entries
static int ls_pack_begin(const char* what, bool pointers, unsigned precisions, const char* note, int precision) {
  NA_REQUIRE(pointers, NA_ENULL, "%s: null pointer", what);
  NA_REQUIRE(accepts(precisions, precision), NA_EUNSUPPORTED, "%s: precision %d%s", what, precision, note);
  return NA_OK;
}

// The n Linears of one MLP: none may lack its weight (or, need_bias, its bias); copied to dst_w / dst_b for the pack kernels that take them by value
static int ls_linears(const char* what, const char* mlp, const float* const* w, const float* const* b, int n, bool need_bias,
                      const float** dst_w = nullptr, const float** dst_b = nullptr) {
  for (int i = 0; i < n; ++i) {
    NA_REQUIRE(w[i] && (!need_bias || b[i]), NA_ENULL, "%s: %s Linear %d is null", what, mlp, i);
    if (dst_w != nullptr) { dst_w[i] = w[i]; dst_b[i] = b[i]; }
  }
  return NA_OK;
}

// A bf16 / bf16x3 / f16 stream: the header, then one pack kernel of ls_pack.h over every fragment element and bias float
template <class Kernel, class PackArgs>
static int launch_pack(Kernel kernel, const PackArgs& w, int pairs, int precision, void* packed, void* stream, const char* what) {
  hipLaunchKernelGGL(ls::pack_ls_header_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ls::kMagic, (uint32_t)precision,
                     (uint32_t*)packed, (uint32_t)pairs);
  const int64_t total = 4 * 2 * (int64_t)pairs * 512 + 4 * ls::kNPhase * 256;
  hipLaunchKernelGGL(kernel, dim3(grid_for(total, 256, 4096)), dim3(256), 0, (hipStream_t)stream, w, precision == NA_PREC_BF16X3 ? 2 : 1,
                     precision == NA_PREC_F16 ? 1 : 0, (char*)packed);
  return check_launch(what);
}

// ---- PlainNeRF(view): MODEL 0, and MODEL 9 = its training forward
extern "C" size_t na_render_ls_packed_bytes(int precision) { return accepts(kAnyPrec, precision) ? ls_stream_bytes(precision, 0) : 0; }

extern "C" int na_render_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                 const float* const* w_view, const float* const* b_view, void* packed, void* stream) {
  const char* what = "na_render_ls_pack";
  ls::PackArgs w;
  NA_TRY(ls_pack_begin(what, w_first && b_first && w_view && b_view && packed, kAnyPrec, "", precision));
  NA_TRY(ls_linears(what, "first", w_first, b_first, 6, false, w.w_first, w.b_first));
  NA_TRY(ls_linears(what, "view", w_view, b_view, 6, false, w.w_view, w.b_view));
  if (precision == NA_PREC_F16X) return ls::render_lsx_pack(0, w_first, b_first, w_view, b_view, (char*)packed, (hipStream_t)stream);
  return launch_pack(ls::pack_ls_kernel, w, ls::kPairsPerPass, precision, packed, stream, what);
}

extern "C" int na_render_plain_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T,
                                       const float* hash_tables, const void* packed, int precision, int sigmoid_kind,
                                       int bg_kind, float* alpha, float* weights, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  ls::Args a{};
  return ls_run({"na_render_plain_view_ls", 0, kAnyPrec, "", true, true, true}, a, rays, pts, R, ts, T, hash_tables, packed, precision,
                sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, hash_tables != nullptr, no_own_checks);
}

// The same launch with PER-RAY steps ts_ray[R,T] (row r = the increasing sample distances of ray r): the fine pass of coarse ->
// fine rendering, whose steps come from na_resample_ts.  Positions are o + t d, interval lengths t[i + 1] - t[i] of the ray's own row.
extern "C" int na_render_plain_view_ls_rayts(const float* rays, int64_t R, const float* ts_ray, int T, const float* hash_tables,
                                             const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha,
                                             float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ls::Args a{};
  a.ts_stride = T;
  return ls_run({"na_render_plain_view_ls_rayts", 0, kAnyPrec, "", true, true, true}, a, rays, nullptr, R, ts_ray, T, hash_tables, packed,
                precision, sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, hash_tables != nullptr,
                no_own_checks);
}

// The training step's forward of PlainNeRF(view) as ONE launch (MODEL 9 = MODEL 0 in bf16x3 that also writes every Linear's output rows
// for the backward pass: ls_kernel.h train_store; what csrc/train_fwd.hip does layer by layer).  Replaces the twelve forward Linears of
// src/neural_blocks.py:279-296 (x 2) in a training iteration (runner.py:647-825).
extern "C" int na_train_plain_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                                      const void* packed, int sigmoid_kind, float* planes, float* view_rows, float* density,
                                      float* rgb_pre, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  NA_REQUIRE(T >= 1 && R >= 0, NA_EINVAL, "na_train_plain_view_ls: bad shape T=%d R=%lld", T, (long long)R);
  if (R == 0) return NA_OK;
  NA_REQUIRE(pts && planes && view_rows && density && rgb_pre, NA_ENULL, "na_train_plain_view_ls: null pointer");
  const int64_t N = (int64_t)T * R;
  NA_REQUIRE(N * 1024 < (1ll << 32), NA_EINVAL, "na_train_plain_view_ls: %lld samples (the row offsets are 32-bit: < 4 194 304)", (long long)N);
  ls::Args a{};
  a.y = planes; a.park = view_rows; a.rl = density; a.feat = rgb_pre;  // (ls_engine.h Args: MODEL 9's outputs ride in fields MODEL 0 leaves alone)
  return ls_run({"na_train_plain_view_ls", 9, kBf16x3, "", true, true, true}, a, rays, pts, R, ts, T, hash_tables, packed, NA_PREC_BF16X3,
                sigmoid_kind, NA_BG_BLACK, nullptr, nullptr, out, workspace, workspace_bytes, stream, hash_tables != nullptr, no_own_checks);
}

// ---- PlainNeRF(view) + mip (config 3; src/nerf.py:256-261, 326-361, src/utils.py:23-140) as ONE launch, NA_PREC_F16X only:
// the 96 IPE features of every sample are generated in the kernel (MODEL 6) for the init and skip Linears of both MLPs
extern "C" size_t na_render_plain_mip_ls_packed_bytes(int precision) { return accepts(kF16x, precision) ? ls_stream_bytes(precision, 6) : 0; }

extern "C" int na_render_plain_mip_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                           const float* const* w_view, const float* const* b_view, void* packed, void* stream) {
  const char* what = "na_render_plain_mip_ls_pack";
  NA_TRY(ls_pack_begin(what, w_first && b_first && w_view && b_view && packed, kF16x, " (f16x only)", precision));
  NA_TRY(ls_linears(what, "first", w_first, b_first, 6, true));
  NA_TRY(ls_linears(what, "view", w_view, b_view, 6, true));
  return ls::render_lsx_pack(6, w_first, b_first, w_view, b_view, (char*)packed, (hipStream_t)stream);
}

extern "C" int na_render_plain_mip_ls(const float* rays, int B, int H, int W, const float* ts, int T, const float* hash_tables,
                                      const void* packed, int precision, int mip_kind, int min_deg, int max_deg, float t_end,
                                      int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  const char* what = "na_render_plain_mip_ls";
  NA_REQUIRE(T >= 1 && B >= 0 && H >= 0 && W >= 0, NA_EINVAL, "%s: bad shape T=%d B=%d H=%d W=%d", what, T, B, H, W);
  ls::Args a{};
  a.mip_H = H; a.mip_W = W; a.mip_kind = mip_kind; a.mip_min_deg = min_deg; a.mip_nd = max_deg - min_deg; a.mip_t_end = t_end;
  return ls_run({what, 6, kF16x, " (f16x only)", true, true, true}, a, rays, nullptr, (int64_t)B * H * W, ts, T, hash_tables, packed,
                precision, sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, hash_tables != nullptr,
                [&](LsStage stage) -> int {
                  if (stage != kAfterPrecision) return NA_OK;
                  NA_REQUIRE(mip_kind == 0 || mip_kind == 1, NA_EUNSUPPORTED, "%s: mip kind %d", what, mip_kind);
                  NA_REQUIRE(max_deg - min_deg == 16, NA_EUNSUPPORTED, "%s: %d IPE degrees (the schedule is built for 16)", what, max_deg - min_deg);
                  NA_REQUIRE(H >= 2, NA_EINVAL, "%s: pixel radii need H >= 2 rows per crop (H=%d)", what, H);
                  return NA_OK;
                });
}

// ---- PlainNeRF with the Positional head (`make original`: src/nerf.py:340-361 + src/refl.py:230-245) and with PosLinearView
// (`make dnerf`: src/refl.py:248-290, optional refl_latent rows of src/nerf.py:1272-1278) as ONE launch each (MODEL 7 / 8), NA_PREC_F16X only
extern "C" size_t na_render_plain_pos_ls_packed_bytes(int precision) { return accepts(kF16x, precision) ? ls_stream_bytes(precision, 7) : 0; }
extern "C" size_t na_render_plain_plv_ls_packed_bytes(int precision) { return accepts(kF16x, precision) ? ls_stream_bytes(precision, 8) : 0; }

extern "C" int na_render_plain_pos_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                           const float* const* w_pos, const float* const* b_pos, void* packed, void* stream) {
  const char* what = "na_render_plain_pos_ls_pack";
  NA_TRY(ls_pack_begin(what, w_first && b_first && w_pos && b_pos && packed, kF16x, " (f16x only)", precision));
  NA_TRY(ls_linears(what, "first", w_first, b_first, 6, true));
  NA_TRY(ls_linears(what, "pos", w_pos, b_pos, 7, true));
  return ls::render_lsx_pack(7, w_first, b_first, w_pos, b_pos, (char*)packed, (hipStream_t)stream, 0);
}

extern "C" int na_render_plain_plv_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                           const float* const* w_head, const float* const* b_head, int n_rl, void* packed, void* stream) {
  const char* what = "na_render_plain_plv_ls_pack";
  NA_TRY(ls_pack_begin(what, w_first && b_first && w_head && b_head && packed, kF16x, " (f16x only)", precision));
  NA_REQUIRE(n_rl >= 0 && n_rl <= 3, NA_EUNSUPPORTED, "%s: %d refl_latent columns (0..3)", what, n_rl);
  NA_TRY(ls_linears(what, "first", w_first, b_first, 6, true));
  NA_TRY(ls_linears(what, "head", w_head, b_head, 8, true));
  return ls::render_lsx_pack(8, w_first, b_first, w_head, b_head, (char*)packed, (hipStream_t)stream, n_rl);
}

static int render_plain_head_ls(const char* what, int model, const float* rays, const float* pts, int64_t R, const float* ts, int T,
                                const float* hash_tables, const float* hash_tables_refl, const float* refl_latent, int64_t rl_ld, int n_rl,
                                const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                                void* workspace, size_t workspace_bytes, void* stream) {
  ls::Args a{};
  a.elaz = rays;  // (MODEL 8's group-wide ray table also fetches two floats per ray from here: any readable 8 R bytes)
  a.tables2 = (const float4*)hash_tables_refl;
  a.rl = n_rl > 0 ? refl_latent : nullptr; a.rl_ld = (int)rl_ld; a.n_rl = n_rl;
  return ls_run({what, model, kF16x, " (f16x only)", true, false, true}, a, rays, pts, R, ts, T, hash_tables, packed, precision, sigmoid_kind,
                bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, hash_tables && hash_tables_refl, [&](LsStage stage) -> int {
                  // (MODEL 8 applies the activation to 67 rows per sample inside the kernel: the four sigmoid-shaped kinds only)
                  if (stage == kAfterSigmoid)
                    NA_REQUIRE(model != 8 || sigmoid_kind == NA_SIG_NORMAL || sigmoid_kind == NA_SIG_THIN || sigmoid_kind == NA_SIG_FAT ||
                                   sigmoid_kind == NA_SIG_UPSHIFTED,
                               NA_EUNSUPPORTED, "%s: sigmoid kind %d (normal | thin | fat | upshifted)", what, sigmoid_kind);
                  if (stage == kAfterBg)
                    NA_REQUIRE(n_rl >= 0 && n_rl <= 3 && (n_rl == 0 || (refl_latent && rl_ld >= n_rl && rl_ld < (1 << 20))), NA_EINVAL,
                               "%s: refl_latent n=%d ld=%lld", what, n_rl, (long long)rl_ld);
                  return NA_OK;
                });
}

extern "C" int na_render_plain_pos_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                                      const float* hash_tables_refl, const void* packed, int precision, int sigmoid_kind, int bg_kind,
                                      float* alpha, float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  return render_plain_head_ls("na_render_plain_pos_ls", 7, rays, pts, R, ts, T, hash_tables, hash_tables_refl, nullptr, 0, 0, packed,
                              precision, sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream);
}

extern "C" int na_render_plain_plv_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                                      const float* hash_tables_refl, const float* refl_latent, int64_t rl_ld, int n_rl, const void* packed,
                                      int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return render_plain_head_ls("na_render_plain_plv_ls", 8, rays, pts, R, ts, T, hash_tables, hash_tables_refl, refl_latent, rl_ld, n_rl,
                              packed, precision, sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream);
}

// ---- TinyNeRF on the same engine (src/nerf.py:278-305)
extern "C" size_t na_render_tiny_ls_packed_bytes(int precision) { return accepts(kAnyPrec, precision) ? ls_stream_bytes(precision, 1) : 0; }

extern "C" int na_render_tiny_ls_pack(int precision, const float* const* w, const float* const* b, void* packed, void* stream) {
  const char* what = "na_render_tiny_ls_pack";
  ls::TinyPackArgs pa;
  NA_TRY(ls_pack_begin(what, w && b && packed, kAnyPrec, "", precision));
  NA_TRY(ls_linears(what, "estim", w, b, 8, false, pa.w, pa.b));
  if (precision == NA_PREC_F16X) return ls::render_lsx_pack(1, w, b, nullptr, nullptr, (char*)packed, (hipStream_t)stream);
  return launch_pack(ls::pack_ls_tiny_kernel, pa, ls::kTinyPairs, precision, packed, stream, what);
}

extern "C" int na_render_tiny_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const void* packed,
                                 int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                                 void* stream) {
  ls::Args a{};
  return ls_run({"na_render_tiny_ls", 1, kAnyPrec, "", true, false, false}, a, rays, pts, R, ts, T, nullptr, packed, precision, sigmoid_kind,
                bg_kind, alpha, weights, out, nullptr, 0, stream, true, no_own_checks);
}

// ---- View head + compositing on per-sample (density source, latent) rows: VolSDF's second half (src/nerf.py:981-1013)
extern "C" size_t na_render_view_ls_packed_bytes(int precision) { return accepts(kAnyPrec, precision) ? ls_stream_bytes(precision, 2) : 0; }

extern "C" int na_render_view_ls_pack(int precision, const float* const* w, const float* const* b, void* packed, void* stream) {
  const char* what = "na_render_view_ls_pack";
  ls::ViewPackArgs pa;
  NA_TRY(ls_pack_begin(what, w && b && packed, kAnyPrec, "", precision));
  NA_TRY(ls_linears(what, "view", w, b, 6, false, pa.w, pa.b));
  if (precision == NA_PREC_F16X) return ls::render_lsx_pack(2, w, b, nullptr, nullptr, (char*)packed, (hipStream_t)stream);
  return launch_pack(ls::pack_ls_view_kernel, pa, ls::kViewPairs, precision, packed, stream, what);
}

extern "C" int na_render_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* feat,
                                 int feat_ld, const float* beta, const void* packed, int precision, int sigmoid_kind,
                                 int bg_kind, float* alpha, float* weights, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  ls::Args a{};
  a.feat = feat; a.feat_ld = feat_ld; a.beta = beta;  // (beta NULL: column 0 is a density logit)
  return ls_run({"na_render_view_ls", 2, kAnyPrec, "", true, true, true}, a, rays, pts, R, ts, T, nullptr, packed, precision, sigmoid_kind,
                bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, feat != nullptr, [&](LsStage stage) -> int {
                  if (stage == kAfterPointers)
                    NA_REQUIRE(feat_ld >= 65, NA_EINVAL, "na_render_view_ls: feat_ld %d < 65 (signed distance + 64 latent columns)", feat_ld);
                  return NA_OK;
                });
}

// ---- VolSDF with the SIREN SDF network as one kernel (src/sdf.py:278-287 + src/nerf.py:981-1013)
extern "C" size_t na_render_volsdf_siren_ls_packed_bytes(int precision) {
  return accepts(kAnyPrec, precision) ? ls_stream_bytes(precision, 3) : 0;
}

extern "C" int na_render_volsdf_siren_ls_pack(int precision, const float* const* w_sdf, const float* const* b_sdf,
                                              const float* const* w_view, const float* const* b_view, void* packed, void* stream) {
  const char* what = "na_render_volsdf_siren_ls_pack";
  ls::SirenPackArgs pa;
  NA_TRY(ls_pack_begin(what, w_sdf && b_sdf && w_view && b_view && packed, kAnyPrec, "", precision));
  NA_TRY(ls_linears(what, "sdf", w_sdf, b_sdf, 7, false, pa.ws, pa.bs));
  NA_TRY(ls_linears(what, "view", w_view, b_view, 6, false, pa.wv, pa.bv));
  if (precision == NA_PREC_F16X) return ls::render_lsx_pack(3, w_sdf, b_sdf, w_view, b_view, (char*)packed, (hipStream_t)stream);
  return launch_pack(ls::pack_ls_siren_kernel, pa, ls::kSirenPairs, precision, packed, stream, what);
}

extern "C" int na_render_volsdf_siren_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* beta,
                                         const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha,
                                         float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  ls::Args a{};
  a.beta = beta;
  return ls_run({"na_render_volsdf_siren_ls", 3, kAnyPrec, "", true, true, true}, a, rays, pts, R, ts, T, nullptr, packed, precision,
                sigmoid_kind, bg_kind, alpha, weights, out, workspace, workspace_bytes, stream, beta != nullptr, no_own_checks);
}

// ---- a hash-encoded SkipConnMLP on the layer-synchronous engine, rows to HBM (D-NeRF's deformation network, src/nerf.py:1250-1257,
// 1267-1270): NA_PREC_F16X (one output tile: up to 32 rows) or NA_PREC_BF16X3 (round 6: the three-product stream, two tiles: up to 64)
extern "C" size_t na_mlp_hash_ls_packed_bytes(int precision) { return accepts(kF16x | kBf16x3, precision) ? ls_stream_bytes(precision, 4) : 0; }

extern "C" int na_mlp_hash_ls_pack(int precision, const float* const* w, const float* const* b, int n_out, void* packed, void* stream) {
  const char* what = "na_mlp_hash_ls_pack";
  ls::HashMlpPackArgs pw;
  NA_TRY(ls_pack_begin(what, w && b && packed, kF16x | kBf16x3, " (f16x | bf16x3)", precision));
  NA_TRY(ls_linears(what, "mlp", w, b, 7, false, pw.w, pw.b));
  const int max_out = precision == NA_PREC_BF16X3 ? 64 : 32;
  NA_REQUIRE(n_out >= 1 && n_out <= max_out, NA_EUNSUPPORTED, "%s: n_out %d (f16x: 1..32, one output tile; bf16x3: 1..64, two)", what, n_out);
  if (precision == NA_PREC_F16X) return ls::render_lsx_pack(4, w, b, nullptr, nullptr, (char*)packed, (hipStream_t)stream, n_out);
  pw.n_out = n_out;
  return launch_pack(ls::pack_ls_hashmlp_kernel, pw, ls::kHashMlpPairs, precision, packed, stream, what);
}

extern "C" int na_mlp_hash_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                              const void* packed, int precision, int n_out, float* y, int64_t y_ld, void* stream) {
  ls::Args a{};
  a.y = y; a.y_ld = (int)y_ld; a.n_out = n_out;
  return ls_run({"na_mlp_hash_ls", 4, kF16x | kBf16x3, " (f16x | bf16x3)", false, false, false}, a, rays, pts, R, ts, T, hash_tables, packed,
                precision, 0, NA_BG_BLACK, nullptr, nullptr, nullptr, nullptr, 0, stream, hash_tables && y, [&](LsStage stage) -> int {
                  if (stage == kAfterPrecision)
                    NA_REQUIRE(n_out >= 1 && n_out <= (precision == NA_PREC_BF16X3 ? 64 : 32) && y_ld >= n_out && y_ld < (1 << 20), NA_EINVAL,
                               "na_mlp_hash_ls: n_out %d, y_ld %lld", n_out, (long long)y_ld);
                  return NA_OK;
                });
}

// ---- a Fourier-encoded SkipConnMLP on the layer-synchronous engine, rows to HBM (VolSDF's MLP SDF network, src/sdf.py:250-258):
// NA_PREC_F16X only
extern "C" size_t na_mlp_fourier_ls_packed_bytes(int precision) { return accepts(kF16x, precision) ? ls_stream_bytes(precision, 5) : 0; }

extern "C" int na_mlp_fourier_ls_pack(int precision, const float* const* w, const float* const* b, void* packed, void* stream) {
  const char* what = "na_mlp_fourier_ls_pack";
  NA_TRY(ls_pack_begin(what, w && b && packed, kF16x, " (f16x only)", precision));
  NA_TRY(ls_linears(what, "mlp", w, b, 8, false));
  return ls::render_lsx_pack(5, w, b, nullptr, nullptr, (char*)packed, (hipStream_t)stream);
}

extern "C" int na_mlp_fourier_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* basis,
                                 const void* packed, int precision, float* y, int64_t y_ld, void* stream) {
  ls::Args a{};
  a.elaz = rays;  // (the group-wide ray table also fetches two floats per ray from here: any readable 8 R bytes)
  a.y = y; a.y_ld = (int)y_ld; a.n_out = 65;
  return ls_run({"na_mlp_fourier_ls", 5, kF16x, " (f16x only)", false, false, false}, a, rays, pts, R, ts, T, basis, packed, precision, 0,
                NA_BG_BLACK, nullptr, nullptr, nullptr, nullptr, 0, stream, basis && y, [&](LsStage stage) -> int {
                  if (stage != kAfterPrecision) return NA_OK;
                  NA_REQUIRE(y_ld >= 65 && y_ld < (1 << 20), NA_EINVAL, "na_mlp_fourier_ls: y_ld %lld < 65", (long long)y_ld);
                  NA_REQUIRE(((uintptr_t)basis & 15) == 0, NA_EINVAL, "na_mlp_fourier_ls: basis must be 16-byte aligned");
                  return NA_OK;
                });
}
#endif
