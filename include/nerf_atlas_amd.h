/*
 * nerf_atlas_amd.h -- C ABI of the MI355X (gfx950) NeRF volume-rendering hot path.
 *
 * The reference (JulianKnodt/nerf_atlas) has no FFI: its "operator API" is the Python
 * protocol of src/cameras.py, src/nerf.py, src/neural_blocks.py.  Each
 * entry point below replaces one reference operator (file:line cited per function) and is
 * what a reference-side ctypes stub would bind.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes.  Every pointer is a DEVICE pointer owned by the
 *    caller (PyTorch allocates); the library never allocates or frees caller memory.
 *  - Every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream).  No hidden synchronisation.
 *  - Return 0 on success, a negative NA_E* code otherwise; na_last_error() gives a
 *    thread-local message.
 *  - Layouts follow the reference: sample tensors are T-major ([T, R, ...], R = B*H*W rays).
 */
#ifndef NERF_ATLAS_AMD_H
#define NERF_ATLAS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NA_VERSION 100 /* 0.1.0 */

enum {
  NA_OK = 0,
  NA_EINVAL = -1,      /* bad shape / argument */
  NA_ENULL = -2,       /* required pointer is NULL */
  NA_EUNSUPPORTED = -3,/* shape or kind has no kernel */
  NA_EHIP = -4,        /* HIP runtime error (launch failed) */
  NA_EWORKSPACE = -5   /* workspace too small */
};

/* activation applied to the INPUT of every hidden Linear and of `out` (src/neural_blocks.py:290-296) */
enum { NA_ACT_NONE = 0, NA_ACT_LEAKY_RELU = 1, NA_ACT_SIN = 2 };
/* encoder fused in front of a SkipConnMLP */
enum { NA_ENC_NONE = 0, NA_ENC_HASH = 1, NA_ENC_FOURIER = 2 };
/* MLP arithmetic */
enum {
  NA_PREC_BF16 = 0,   /* bf16 operands, fp32 accumulate (1 MFMA product)            */
  NA_PREC_BF16X3 = 1, /* 2-way split bf16, 3 MFMA products, fp32-class accuracy     */
  NA_PREC_F16 = 2,    /* f16 operands, fp32 accumulate (1 MFMA product, 11-bit operands): the layer-synchronous
                         renderers (na_render_*_ls) and na_mlp_pack / na_mlp_forward; not na_render_plain_view */
  NA_PREC_F16X = 3    /* f16 main product + two MX-fp6 (e2m3, E8M0 scale per 32 k) correction products
                         fp6(W - f16 W) x fp6(x) + fp6(W) x fp6(x - f16 x) on v_mfma_scale_f32_32x32x64_f8f6f4: 1.5 MFMA
                         products per k, ~15-bit operands (init / geometry chunks: f16 hi + lo, 3 products).
                         The layer-synchronous renderers only (na_render_*_ls_pack / na_render_*_ls) */
};
/* weight-stream layouts */
enum { NA_LAYOUT_GENERIC = 0, NA_LAYOUT_PLAIN_FIRST = 1, NA_LAYOUT_PLAIN_VIEW = 2 };
/* density -> sigma (src/nerf.py:64-65) */
enum { NA_DENSITY_SOFTPLUS_M1 = 0, NA_DENSITY_RELU = 1 };
/* background (src/nerf.py:96-109) */
enum { NA_BG_BLACK = 0, NA_BG_WHITE = 1, NA_BG_RANDOM = 2 /* only through the *_random_bg entry points: needs the draw */ };
/* colour-head activations, src/utils.py:484-518 sigmoid_kinds */
enum {
  NA_SIG_NORMAL = 0, NA_SIG_THIN = 1, NA_SIG_FAT = 2, NA_SIG_TANH = 3, NA_SIG_UPSHIFTED = 4,
  NA_SIG_RELU = 5, NA_SIG_SIN = 6, NA_SIG_LEAKY_RELU = 7, NA_SIG_UPSHIFTED_SOFTPLUS = 8,
  NA_SIG_UPSHIFTED_RELU = 9, NA_SIG_CYCLIC = 10, NA_SIG_IDENTITY = 11
};

int na_version(void);
const char* na_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * A1+A2  pixel grid + NeRFCamera.sample_positions   (runner.py:490-503, src/cameras.py:45-66)
 * rays[b, r, c, :] for the crop rows crop_t..crop_t+crop_h, cols crop_l..crop_l+crop_w of a
 * size x size image (the crop is clipped to the image like the reference's slicing, so the
 * caller passes the clipped h,w).  noise: NULL, or [h,w,2] uniform[0,1) draws (u then v)
 * used as (noise-0.5)*with_noise  (replaces the reference's global-RNG rand_like).
 * rays: [B, h, w, 6] = origin | un-normalised direction.                                      */
int na_raygen(const float* c2w /*[B,3,4]*/, int B, float focal, int size,
              int crop_t, int crop_l, int crop_h, int crop_w,
              const float* noise, float with_noise, float* rays, void* stream);

/* A2' DTUCamera.sample_positions + lift  (src/cameras.py:159-223); rays [B, h, w, 6] with
 * normalised directions; pose/intrinsic [B,4,4].                                              */
int na_raygen_dtu(const float* pose, const float* intrinsic, int B, int size,
                  int crop_t, int crop_l, int crop_h, int crop_w, float* rays, void* stream);

/* A3 compute_ts (src/nerf.py:29-47).  rand: NULL or device [T] uniform draws (perturb>0).
 * ts: [T]; mids: NULL or [T-1].                                                               */
int na_compute_ts(float near, float far, int T, int lindisp, float perturb, const float* rand,
                  float* ts, float* mids, void* stream);

/* A3 compute_pts_ts (src/nerf.py:50-55): pts[t, r, :] = r_o[r] + ts[t] * r_d[r].
 * rays [R,6]; pts [T,R,3].                                                                    */
int na_compute_pts(const float* rays, const float* ts, int T, int64_t R, float* pts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A5 HashEncoder.forward (src/neural_blocks.py:139-193).  x [N,3]; tables [8,65536,4] fp32;
 * out [N, 32 + 3*include_input]; idx_out: NULL or int64 [8 levels, 8 corners, N] table rows
 * (bit-exact int64 hashing).                                                                  
 * `out` must be 16-byte aligned (the rows are written with 16-byte stores; NA_EINVAL otherwise). */
int na_hash_encode(const float* x, int64_t N, const float* tables, int include_input,
                   float* out, int64_t* idx_out, void* stream);

/* A5' FourierEncoder.forward / fourier (src/neural_blocks.py:52, src/utils.py:14-17).
 * basis [D,F] (already multiplied by extra_scale by the caller or pass scale); out [N,2F].    */
int na_fourier_encode(const float* x, int64_t N, int D, const float* basis, int F, float scale,
                      float* out, void* stream);

/* PositionalEncoder.forward (src/neural_blocks.py:30-34): out [N, 2*D*NB].                     */
int na_positional_encode(const float* x, int64_t N, int D, const float* bands, int NB,
                         float* out, void* stream);

/* A7 dir_to_elev_azim (src/utils.py:247-254): dirs [N,3] -> out [N,2].                         */
int na_view_elaz(const float* dirs, int64_t N, float* out, void* stream);
/* rows [x, y, z, elev, azim] [N, 5] of the View reflectance's input: pts [N = T x R, 3] with the per-RAY directions dirs [R, 3]
 * broadcast along the samples (n = t R + r) -- src/refl.py:190-207's cat([x, dir_to_elev_azim(view)]) in one launch. */
int na_view_rows(const float* pts, const float* dirs, int64_t N, int64_t R, float* out, void* stream);
/* training step, the torch glue around the two networks of PlainNeRF(view) as kernels (round 6):
 * na_hash_encode_rows   out [N, 32 + 3 (include_input + lead)] = [x (lead = 1) | x (include_input) | features]: with lead = 1 the
 *                       init rows cat([p, enc(p)]) of a hash-encoded SkipConnMLP (src/neural_blocks.py:139-193, 283-287) written by
 *                       the encoder itself.
 * na_plain_head_rows    PlainNeRF.from_pts between its networks (src/nerf.py:338-357, src/refl.py:190-207): first_out [N, 1 + C] ->
 *                       density [N] = first_out[:, 0] and the View MLP's init rows [N, 5 + C] = [x, y, z, elev, azim | first_out[:, 1:]]
 *                       (pts [N = T x R, 3], per-RAY directions dirs [R, 3], n = t R + r).                                            */
int na_hash_encode_rows(const float* x, int64_t N, const float* tables, int include_input, int lead, float* out, void* stream);
int na_plain_head_rows(const float* first_out, const float* pts, const float* dirs, int64_t N, int64_t R, int C, float* density,
                       float* rows, void* stream);

/* sigmoid_kinds (src/utils.py:484-518) elementwise, in place allowed.                          */
int na_sigmoid(const float* x, int64_t N, int kind, float* out, void* stream);

/* A6 mip integrated positional encoding, intended layout: rays [B*H*W,6] of an
 * H x W crop (radii_x differences rows), ts [T]; kind 0 = cylinder, 1 = cone; t_end = upper
 * bound of the last interval (NaN: the kernel uses 2 ts[T-1] - ts[T-2], the intended closing, so
 * the host need not read ts back); out [T, B*H*W, 6*(max_deg-min_deg)].                      */
int na_mip_encode(const float* rays, int B, int H, int W, const float* ts, int T, int kind,
                  float t_end, int min_deg, int max_deg, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A8 alpha_from_density + volumetric_integrate + sky (src/nerf.py:22-27,60-80,96-109).
 * density [T,R]; feat [T,R,C]; ts [T]; rays [R,6] (direction norm scales the intervals, Q1);
 * alpha/weights: NULL or [T,R]; out [R,C].                                                    */
int na_composite(const float* density, const float* feat, const float* ts, const float* rays,
                 int T, int64_t R, int C, int density_kind, int bg_kind,
                 float* alpha, float* weights, float* out, void* stream);

/* The same with `--bg random` (src/nerf.py:99-103 random_color): out += rand[r] * (1 - sum(weights[:-1])), ONE uniform draw
 * per ray broadcast over the channels.  The draw is an explicit input rand [R] (the reference calls torch.rand_like inside).
 * na_sky_random adds that term to the out [R,C] of a renderer that composited against black and kept weights [T,R]
 * (the fused one-kernel renderers).                                                              */
int na_composite_random_bg(const float* density, const float* feat, const float* ts, const float* rays,
                           int T, int64_t R, int C, int density_kind, const float* rand,
                           float* alpha, float* weights, float* out, void* stream);
int na_sky_random(const float* weights, const float* rand, int T, int64_t R, int C, float* out, void* stream);

/* volumetric_integrate(weights, other) alone (src/nerf.py:79-80; depth/flow maps,
 * runner.py:894-920): weights [T,R], other [T,R,C] -> out [R,C].                              */
int na_integrate(const float* weights, const float* other, int T, int64_t R, int C, float* out,
                 void* stream);

/* PosLinearView pieces (src/refl.py:248-290): unit view directions (F.normalize, eps 1e-12), and the final
 * out[N,C] = (sigmoid(lin[N]) / 2 + 0.5) * pos[N rows of pitch pos_ld, first C columns].                            */
int na_normalize3(const float* v, int64_t N, float* out, void* stream);
int na_pos_linear_combine(const float* lin, const float* pos, int64_t pos_ld, int64_t N, int C, float* out,
                          void* stream);

/* A12 VolSDF density = 1/beta * laplace_cdf(-sdf, beta) (src/utils.py:50-58, src/nerf.py:1000-1003);
 * beta is a device scalar (learned parameter).                                                */
int na_laplace_density(const float* sdf, int64_t N, const float* beta, float* density, void* stream);

/* A11 spline warp (src/nerf.py:1173-1178,1201-1206,1267-1278): est [N, 1+3n] = rigidity | n
 * control points; t [N] (or per-view broadcast via t_stride 0... caller expands); pts [N,3].
 * out_pts = pts + bezier(t) * sigmoid(rigidity/2); optional dp, rigidity_out [N,3],[N].       */
int na_bezier_warp(const float* est, int est_stride, const float* pts, const float* t, int64_t N,
                   int n_ctrl, float* out_pts, float* dp, float* rigidity_out, void* stream);
/* the same with DynamicNeRF's reflectance latent (--dyn-refl-latent n_rl > 0; src/nerf.py:1246-1248, 1272-1278):
 * est [N, >= 2 + (3 + n_rl) n] = rigidity | n control points | enc_rigidity | n latent control rows of n_rl;
 * refl_latent [N, n_rl] = bezier(latent control rows, t) * sigmoid(enc_rigidity) -- what from_pts receives as
 * `refl_latent` (src/nerf.py:1303).  n_rl 1..16.                                                               */
int na_bezier_warp_latent(const float* est, int est_stride, const float* pts, const float* t, int64_t N,
                          int n_ctrl, int n_rl, float* out_pts, float* dp, float* rigidity_out,
                          float* refl_latent, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A4 SkipConnMLP (src/neural_blocks.py:204-296).
 *
 * Exact-fp32 Linear used for any layer shape: y[N,out] = W[out,in] . act(x[N,in]) + b
 * (f32 MFMA, v_mfma_f32_32x32x2_f32 -- bitwise an fp32 fma chain).  x may be the concatenation
 * of two buffers (skip connection): x = [x0 (in0 cols) | x1 (in1 cols)].                      */
int na_linear_f32(const float* x0, int in0, const float* x1, int in1, int64_t N,
                  const float* W, const float* b, int out, int pre_act, float* y, void* stream);
/* na_linear_f32 for rows that live inside wider buffers and for a per-RAY bias (the hoisted spherical-harmonic head below:
 * src/neural_blocks.py:279-296 with the ray-constant columns of `init` folded into the bias).  x0 / x1 are read with the row
 * pitches ld0 >= in0 / ld1 >= in1 (floats), so a column slice such as `first_out[..., 1:]` goes in without a copy.  Bias: `b` [out]
 * broadcast, or `b_rows` [R, out] added as b_rows[n % R] (rows sample-major, n = t R + r, N a multiple of R), or neither; passing
 * both is NA_EINVAL.  Same kernel template and the same arithmetic as na_linear_f32.                                            */
int na_linear_f32_rows(const float* x0, int in0, int64_t ld0, const float* x1, int in1, int64_t ld1, int64_t N,
                       const float* W, const float* b, const float* b_rows, int64_t R, int out, int pre_act, float* y,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spherical-harmonic colour head, refl kind "sph-har" (src/refl.py:696-731; csrc/sh_head.hip).  Rows sample-major: the ray of
 * row n is n % R.  All arithmetic fp32.
 *
 * na_sh_shade           eval_sh + F.normalize + the head's activation (src/spherical_harmonics.py:55-106, src/refl.py:726-731):
 *                       rgb[n, c] = sigmoid_kind( sum_k coeffs[n, c K + k] Y_k(dirs[n % R] / max(|dirs[n % R]|, 1e-12)) ),
 *                       K = (order + 1)^2, order 0..4 (NA_EINVAL otherwise), the 3 K coefficients channel-major like the
 *                       reference's reshape(..., 3, K).  coeffs [N, 3 K] with row pitch ld; dirs [R, 3] un-normalised (R = N for
 *                       one direction per sample); pre: NULL or [N, 3], the sums in front of the activation (for the backward).
 *                       The basis is evaluated in registers; kind: every NA_SIG_*, anything else NA_EUNSUPPORTED.
 * na_sh_shade_backward  g_coeffs[n, c K + k] = g_rgb[n, c] * sigmoid_kind'(pre[n, c]) * Y_k (contiguous [N, 3 K]).  The
 *                       directions receive no gradient.
 * na_sh_view_terms      the ray-only part of the head's SkipConnMLP (src/neural_blocks.py:279-296 with
 *                       init = [v | enc(v) | latent], v = dir_to_elev_azim(view) of src/utils.py:247-254 and enc the FourierEncoder
 *                       of src/neural_blocks.py:36-55): with f = [elev, azim | sin(v B) | cos(v B)] (2 + 2 F values, bit-identical
 *                       to na_view_elaz + na_fourier_encode) of every ray,
 *                           terms[0, r, :] = w_init . f + b_init;   terms[1, r, :] = w_a . leaky_relu(f) + b_a;   terms[2] likewise (w_b),
 *                       w_init [hidden, 2 + 2 F] with row pitch ld_init = the view columns of `init.weight`; w_a / w_b with row
 *                       pitch ld_skip = the view columns of the two skip Linears (`layers.0`, `layers.3`); basis [2, F], scale =
 *                       the encoder's extra_scale; terms [3, R, hidden].  F <= 128 and hidden in {32, 64, 96, 128}, else
 *                       NA_EUNSUPPORTED.  The terms are the `b_rows` of na_linear_f32_rows over the remaining (latent) columns. */
int na_sh_shade(const float* coeffs, int64_t ld, const float* dirs, int64_t N, int64_t R, int order, int kind,
                float* rgb, float* pre, void* stream);
int na_sh_shade_backward(const float* g_rgb, const float* pre, const float* dirs, int64_t N, int64_t R, int order,
                         int kind, float* g_coeffs, void* stream);
int na_sh_view_terms(const float* dirs, int64_t R, const float* basis, int F, float scale, const float* w_init,
                     int64_t ld_init, const float* b_init, const float* w_a, const float* b_a, const float* w_b,
                     const float* b_b, int64_t ld_skip, int hidden, float* terms, void* stream);

typedef struct NaMlpDesc {
  int32_t in_size;     /* raw input width (p)                                         */
  int32_t enc_kind;    /* NA_ENC_*                                                    */
  int32_t enc_dims;    /* encoder output width (35 hash, 2F fourier, 0 none)          */
  int32_t latent_size; /* extra per-sample latent columns                             */
  int32_t num_layers;  /* hidden Linear count L (src/neural_blocks.py:240-244)        */
  int32_t hidden;      /* hidden width; the MFMA path requires 256                    */
  int32_t out_size;
  int32_t skip;        /* 3                                                           */
  int32_t activation;  /* NA_ACT_LEAKY_RELU | NA_ACT_SIN                              */
  int32_t layout;      /* NA_LAYOUT_*: GENERIC for na_mlp_forward; the PLAIN_* values
                          re-order rows/columns for na_render_plain_view               */
} NaMlpDesc;

/* Fused MFMA SkipConnMLP: weights are re-laid out once into the MFMA A-fragment stream
 * (bf16 hi [+ lo]) that the kernel DMA-streams through LDS.
 *   na_mlp_packed_bytes : size of that stream for (desc, precision); 0 if unsupported.
 *   na_mlp_pack         : device-side pack.  weights/biases: HOST arrays of L+2 DEVICE pointers
 *                         in the order init, layers[0..L-1], out  (nn.Linear layout [out,in]).
 *   na_mlp_forward      : p [N,in_size]; latent [N,latent_size] or NULL; enc_params: hash tables
 *                         [8,65536,4] or Fourier basis [D,F] or NULL; y [N,out_size].          */
size_t na_mlp_packed_bytes(const NaMlpDesc* desc, int precision);
int na_mlp_pack(const NaMlpDesc* desc, int precision, const float* const* weights,
                const float* const* biases, void* packed, void* stream);
int na_mlp_forward(const NaMlpDesc* desc, int precision, const void* packed,
                   const float* p, const float* latent, const float* enc_params, int64_t N,
                   float* y, void* stream);
/* Same with explicit row pitches (in floats) for p and latent: the inputs may be column slices of wider buffers, e.g.
 * latent = first_out + 1 with pitch 65 (src/nerf.py:349-352 `intermediate = first_out[..., 1:]`) -- no copy.          */
int na_mlp_forward_ld(const NaMlpDesc* desc, int precision, const void* packed,
                      const float* p, int64_t p_ld, const float* latent, int64_t latent_ld,
                      const float* enc_params, int64_t N, float* y, void* stream);
/* IPE latent generated in the MLP prologue (config 3: src/utils.py:83-140 cylinder / conic Gaussians, hook
 * src/nerf.py:256-261).  `mip` describes the crop the N = T*B*H*W samples come from (sample n = t*B*H*W + ray); the
 * leading 6*(max_deg-min_deg) latent columns are computed from it inside the kernel (same arithmetic as na_mip_encode,
 * intended layout), the remaining latent_size - 6 nd columns are read from `latent` (pitch latent_ld) as usual.
 * mip == NULL is na_mlp_forward_ld.                                                                               */
typedef struct NaMipDesc {
  const float* rays;   /* [B,H,W,6] rays of ONE crop (pixel radii difference neighbouring rows)   */
  const float* ts;     /* [T]                                                                     */
  int32_t B, H, W, T;
  int32_t kind;        /* 0 cylinder, 1 cone                                                      */
  int32_t min_deg, max_deg;
  float t_end;         /* closes the last interval (see na_mip_encode); NaN = 2 ts[T-1] - ts[T-2] */
} NaMipDesc;
int na_mlp_forward_mip(const NaMlpDesc* desc, int precision, const void* packed, const float* p, int64_t p_ld,
                       const float* latent, int64_t latent_ld, const float* enc_params, const NaMipDesc* mip, int64_t N,
                       float* y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A10 PlainNeRF.forward with the View head (src/nerf.py:326-361, src/refl.py:190-207), fully
 * fused: sample -> hash encode -> first MLP -> elaz -> View MLP -> sigmoid -> composite.
 *   rays [R,6]; ts [T]; hash tables [8,65536,4]; packed_first / packed_view from na_mlp_pack
 *   (descs: first = {3,HASH,35,0,4,256,1+64,3,LEAKY,PLAIN_FIRST}, view = {5,NONE,0,64,4,256,3,3,SIN,PLAIN_VIEW}).
 *   workspace: na_render_workspace_bytes(T,R) bytes of device scratch (per-(ray,block) partials).
 *   alpha/weights: NULL or [T,R].  out [R,3].                                                 */
size_t na_render_workspace_bytes(int T, int64_t R);
int na_render_plain_view(const float* rays, int64_t R, const float* ts, int T,
                         const float* hash_tables, const void* packed_first, const void* packed_view,
                         int precision, int sigmoid_kind, int bg_kind,
                         float* alpha, float* weights, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* Same kernel with explicit sample positions pts[T,R,3] (PlainNeRF.from_pts, src/nerf.py:340-361, as called by
 * DynamicNeRF with the spline-warped canonical points, src/nerf.py:1301-1303); directions and interval lengths still
 * come from rays / ts.                                                                                              */
int na_render_plain_view_pts(const float* rays, const float* pts, int64_t R, const float* ts, int T,
                             const float* hash_tables, const void* packed_first, const void* packed_view,
                             int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backward operators (training step, runner.py:609-850: loss.backward() differentiates exactly these).
 * fp32; every gradient buffer that is ACCUMULATED into (dW, db, tables_grad) must be zero-initialised
 * (or hold the running .grad) by the caller.
 *
 * na_act_backward      g_x = g_act * act'(x) for the pre-activation input x of a Linear
 *                      (src/neural_blocks.py:293).
 * na_sigmoid_backward  g_x = g_y * d/dx sigmoid_kind(x) (src/utils.py:484-518).
 * na_pos_linear_combine_backward  gradient of na_pos_linear_combine (src/refl.py:288-290) w.r.t. lin [N] (g_lin,
 *                      nullable) and pos (g_pos [N, gpos_ld], nullable: columns < C receive g * (sigmoid/2 + 0.5),
 *                      columns C..gpos_ld-1 are zeroed) given g [N, C].
 * na_linear_wgrad      dW[out,in] += dY^T . act([x0|x1]);  db[out] += sum_n dY (db may be NULL), exact fp32
 *                      (the exact input gradient is na_linear_f32 with W^T followed by na_act_backward).
 * Fast training precision: the three GEMMs of a layer on the bf16 matrix core with a 2-way operand split
 * (hi = bf16(x), lo = bf16(x - hi); lo*hi + hi*lo + hi*hi accumulated in fp32: relative error ~2^-16):
 * na_linear_bf16x3        same contract as na_linear_f32 (y = W . act([x0|x1]) + b).
 * na_linear_dgrad_bf16x3  g_x0[N,in0] | g_x1[N,in1] = (dY[N,out] . W) * act'([x0|x1]); Wt = W^T as
 *                         [in0+in1, out] row-major; either output may be NULL; x0/x1 = the forward inputs.
 * na_linear_wgrad_bf16x3  same contract as na_linear_wgrad.
 * na_linear_wgrad_bf16x3_ow  the same gradient WRITTEN to dW / db instead of accumulated (no zero fill by the caller).
 * Round 5 -- one pack launch per training step instead of one per GEMM (the reference's loop, runner.py:647-825, re-reads
 * nn.Linear.weight in every F.linear; here the bf16 hi / lo MFMA fragments of every Linear are built once per step):
 * na_train_packed_bytes   bytes of the packed form of an [M, K] B operand (0: no packed form, M > 1024).
 * na_train_pack_many      n operands in ONE launch: operand i is the M[i] x K[i] matrix B[m,k] = W[i][m * ld[i] + k], or with
 *                         transposed[i] B[m,k] = W[i][k * ld[i] + m] (the input gradient's W^T read straight from
 *                         nn.Linear.weight: no transposing copy); dst[i]: na_train_packed_bytes(M[i], K[i]) bytes, 16-byte aligned.
 * na_train_gemm_packed_ok 1 if a batch of N rows with M output columns runs the kernels that take packed operands
 *                         (N >= 2048, M <= 1024, NA_TRAIN_GEMM != tiled), else 0: call the unpacked entry points.
 * na_linear_bf16x3_pk / na_linear_dgrad_bf16x3_pk   na_linear_bf16x3 / na_linear_dgrad_bf16x3 with the packed W [out, in0+in1] /
 *                         packed W^T [in0+in1, out] in place of the matrix (NA_EUNSUPPORTED where ..._packed_ok says 0).
 * na_hash_encode_backward  tables_grad[8,65536,4] += trilinear weights x g_out[N, 32(+3)]
 *                      (src/neural_blocks.py:166-190).
 * na_hash_encode_backward_input  g_x[N,3] = d(features)/d(position) . g_out (+ g_out[:, :3] with
 *                      include_input); floor() carries no gradient, as in torch.autograd of the same lines.
 * na_laplace_density_backward    g_sdf[N] and (optional, ACCUMULATED into one float the caller zeroed) g_beta of
 *                      na_laplace_density (src/utils.py:50-58, src/nerf.py:985-990).
 * na_bezier_warp_backward        g_est[N, est_stride] of na_bezier_warp given any of g_out_pts [N,3], g_dp [N,3],
 *                      g_rigidity [N] (null = zero) (src/nerf.py:1173-1178,1201-1206,1267-1278).
 * na_composite_backward    gradient of na_composite w.r.t. density [T,R] and feat [T,R,C] (C = 1 or 3)
 *                      given g_out [R,C] (src/nerf.py:60-80,96-98).                              */
 /* Deterministic accumulation.  The gradients summed across workgroups (dW/db of the two na_linear_wgrad* kernels,
 * the hash-table scatter, d/dbeta of the Laplace density) use fp32 atomics by default: fast, but the rounding depends
 * on the arrival order, so two runs differ in the last bits (and a chaotic training trajectory such as D-NeRF's
 * diverges from there).  After na_set_deterministic(ws, bytes) -- a caller-owned device buffer of at least
 * 8 * (largest accumulated output) bytes = 16 MiB for the hash tables -- those operators accumulate in 64-bit fixed
 * point (2^-40 resolution): integer addition is associative, so results are bitwise reproducible.  The setting is
 * process-wide (autograd engines call the backward operators from their own threads); the workspace is used by one
 * operator at a time, in stream order, so all deterministic work must share one stream.  NULL switches it off.       */
int na_set_deterministic(void* workspace, size_t bytes);

/* Forward-mode tangents for SDF normals and the eikonal regulariser (src/sdf.py:43,108, runner.py:685-692,
 * src/utils.py:31): d sdf / d x is propagated forward through the MLP as three tangent rows per sample,
 * t_{l+1} = W_l . (act'(z_l) * t_l), so the loss on the normals is a first-order graph of the operators below plus
 * na_linear_*; no double backward is needed.
 * na_act_deriv          out = act'(x) (order 1) or act''(x) (order 2) for NA_ACT_* (leaky: 0.01|1, 0; sin: cos, -sin).
 * na_mul_bcast          out[j,i] = a[i] * b[j,i], a [n], b/out [J,n]: one multiplier row shared by J tangent rows.
 * na_mul_reduce         out[i] = sum_j g[j,i] * b[j,i] (gradient of na_mul_bcast w.r.t. a).
 * na_eikonal_loss       loss[0] += mean_n (|normals[:,n]| - 1)^2, normals [3,N] tangent-major; loss zeroed by caller.
 *                       N == 0: loss[0] = NaN, the mean of nothing (torch's); the backward writes nothing.
 * na_eikonal_loss_backward  g_normals [3,N] = g[0] * d loss / d normals.                                          */
int na_act_deriv(const float* x, int64_t n, int act, int order, float* out, void* stream);
int na_mul_bcast(const float* a, const float* b, int64_t n, int J, float* out, void* stream);
int na_mul_reduce(const float* g, const float* b, int64_t n, int J, float* out, void* stream);
int na_eikonal_loss(const float* normals, int64_t N, float* loss, void* stream);
int na_eikonal_loss_backward(const float* normals, int64_t N, const float* g, float* g_normals, void* stream);
int na_act_backward(const float* x, const float* g, int64_t n, int act, float* out, void* stream);
int na_sigmoid_backward(const float* x, const float* g, int64_t n, int kind, float* out, void* stream);
int na_pos_linear_combine_backward(const float* lin, const float* pos, int64_t pos_ld, const float* g, int64_t N, int C,
                                   float* g_lin, float* g_pos, int64_t gpos_ld, void* stream);
int na_linear_bf16x3(const float* x0, int in0, const float* x1, int in1, int64_t N, const float* W, const float* b,
                     int out, int pre_act, float* y, void* stream);
int na_linear_dgrad_bf16x3(const float* dY, int out, int64_t N, const float* Wt, const float* x0, int in0,
                           const float* x1, int in1, int pre_act, float* g_x0, float* g_x1, void* stream);
int na_linear_wgrad_bf16x3(const float* x0, int in0, const float* x1, int in1, int64_t N, const float* dY, int out,
                           int pre_act, float* dW, float* db, void* stream);
int na_linear_wgrad_bf16x3_ow(const float* x0, int in0, const float* x1, int in1, int64_t N, const float* dY, int out,
                              int pre_act, float* dW, float* db, void* stream);
size_t na_train_packed_bytes(int M, int K);
int na_train_gemm_packed_ok(int64_t N, int M);
/* Which kernel family a shape runs -- what the entry points themselves dispatch on, for callers and tests that must know:
 * K-staged tiles (small batches, widths > 1024; the _pk entry points return NA_EUNSUPPORTED there), the layer-synchronous
 * streaming kernels, the row-stream kernel of a narrow output (K = 256, M <= 128), the row-stream kernel on the narrow second
 * source of a skip layer with the streaming kernel on its first, W resident in registers (train_fwd.hip).  `in` of the
 * unpacked input gradient is in0 + in1. */
#define NA_TRAIN_PATH_KSTAGED 0
#define NA_TRAIN_PATH_LS 1
#define NA_TRAIN_PATH_NARROW 2
#define NA_TRAIN_PATH_NARROW_X1 3
#define NA_TRAIN_PATH_RESIDENT 4
int na_linear_bf16x3_path(int64_t N, int out);
int na_linear_dgrad_bf16x3_path(int64_t N, int in);
int na_linear_wgrad_bf16x3_path(int64_t N, int out, int in0, int in1);
int na_linear_bf16x3_pk_path(int64_t N, int out, int in0, int in1, int pre_act);
int na_linear_dgrad_bf16x3_pk_path(int64_t N, int out, int in0, int in1);
int na_train_pack_many(int n, const float* const* W, const int* M, const int* K, const int* ld, const int* transposed,
                       void* const* dst, void* stream);
int na_linear_bf16x3_pk(const float* x0, int in0, const float* x1, int in1, int64_t N, const void* w_packed, const float* b,
                        int out, int pre_act, float* y, void* stream);
int na_linear_dgrad_bf16x3_pk(const float* dY, int out, int64_t N, const void* wt_packed, const float* x0, int in0,
                              const float* x1, int in1, int pre_act, float* g_x0, float* g_x1, void* stream);
/* Round 5: input gradient AND weight gradient of one Linear in ONE pass over dY and the forward input (they read the same two
 * [N, .] tensors; src/neural_blocks.py:288-296 differentiated, runner.py:647-825's loss.backward()):
 *   g_x0[N,in0] = (dY . W[:, c0:c0+in0]) * act'(x0);  dW[out, 0:in0] (leading dimension ldw >= in0) and db[out] (if given) WRITTEN.
 * in0 = 256 (a wide source) or in0 <= 128 (a narrow one: an init Linear's 38 / 69 columns, the second source of a skip layer);
 * out <= 256; wt_packed = W^T [in, out] as na_train_pack_many packs it, at the column group of the source's first row c0 (a
 * multiple of 64): na_train_packed_row_offset(c0, out) bytes into the packed stream.  The sources of a concatenated input are
 * separate calls (dW + c0 with the full leading dimension).  na_linear_bwd_fused_ok: 1 if (N, out, in0) runs this kernel
 * (N >= 8192, NA_TRAIN_FUSED_BWD != 0), else the entry point returns NA_EUNSUPPORTED. */
size_t na_train_packed_row_offset(int row0, int K);
int na_linear_bwd_fused_ok(int64_t N, int out, int in0);
/* na_linear_wgrad_bf16x3_cols: the weight gradient of ONE source of a concatenated input: dW[:, 0:in) at leading dimension ldw and
 * (if given) db WRITTEN -- the narrow source [N, 38 / 69] of a skip layer whose wide source went through na_linear_bwd_bf16x3_pk. */
int na_linear_wgrad_bf16x3_cols(const float* x, int in, int64_t N, const float* dY, int out, int pre_act, float* dW, int ldw,
                                float* db, void* stream);
/* workspace: na_linear_bwd_workspace_bytes(N, in0) bytes of device memory for the partial gradients (16-byte aligned; the caller's
 * allocator -- torch's is stream-ordered and costs microseconds), or NULL: the call then takes them from the library's grow-only
 * scratch of this (device, stream) -- no driver call once it exists; it grows geometrically and a replaced buffer is freed when
 * the work queued before its replacement has finished. */
size_t na_linear_bwd_workspace_bytes(int64_t N, int in0);
int na_linear_bwd_partial_count(int64_t N, int in0);   /* partial gradients in that workspace (the nwg_i of na_train_reduce_many) */
/* The pass without its reduction (the whole-network backward of a SkipConnMLP: every Linear's partial gradients stay in a
 * workspace of its own -- na_linear_bwd_workspace_bytes(N, in0) bytes = slices x 67 584 floats -- and ONE na_train_reduce_many
 * sums them all: dW_i[out_i, 0:in_i) at leading dimension ldw_i and db_i (nullable) WRITTEN from nwg_i = slices partials).
 * g_add (nullable, [N, in0]; narrow sources, in0 <= 128, only): added to the input gradient before it is stored. */
int na_linear_bwd_partials_bf16x3_pk(const float* dY, int out, int64_t N, const void* wt_packed, const float* x0, int in0, int pre_act,
                                     float* g_x0, const float* g_add, int want_db, void* workspace, void* stream);
int na_train_reduce_many(int n, const float* const* part, const int* nwg, const int* out, const int* in, const int* ldw, float* const* dW,
                         float* const* db, void* stream);
int na_linear_bwd_bf16x3_pk(const float* dY, int out, int64_t N, const void* wt_packed, const float* x0, int in0, int pre_act,
                            float* g_x0, float* dW, int ldw, float* db, void* workspace, void* stream);
int na_linear_wgrad(const float* x0, int in0, const float* x1, int in1, int64_t N, const float* dY, int out,
                    int pre_act, float* dW, float* db, void* stream);
int na_hash_encode_backward(const float* x, int64_t N, const float* g_out, int include_input,
                            float* tables_grad, void* stream);
int na_hash_encode_backward_input(const float* x, int64_t N, const float* tables, const float* g_out,
                                  int include_input, float* g_x, void* stream);
/* the same two on a gradient read IN PLACE from wider rows (the gradient of a network's init rows [x | x | features | ...] of pitch
 * g_ld: no slice copy): _backward_rows takes the 32 feature columns at g_col0; _backward_input_rows takes rows
 * [x (lead) | x (include_input) | features] and adds the leading copy's gradient.
 * na_plain_head_rows_backward: g_first_out [N, 1 + C] = [g_density (nullable: 0) | g_rows[:, 5:]], g_pts [N, 3] = g_rows[:, :3] (nullable). */
int na_hash_encode_backward_rows(const float* x, int64_t N, const float* g_rows, int g_ld, int g_col0, float* tables_grad,
                                 void* stream);
int na_hash_encode_backward_input_rows(const float* x, int64_t N, const float* tables, const float* g_rows, int g_ld,
                                       int include_input, int lead, float* g_x, void* stream);
int na_plain_head_rows_backward(const float* g_density, const float* g_rows, int64_t N, int C, float* g_first_out, float* g_pts,
                                void* stream);
/* The Fourier encoder as a training node (csrc/fourier_grad.hip; src/utils.py:14-17 under autograd).  1 <= D <= 8, basis [D, F], `scale`
 * as na_fourier_encode takes it.
 * na_fourier_rows       rows [N, D + 2F + L] = [x | sin(x B) | cos(x B) | latent]: the init rows cat([p, enc(p), latent]) of a Fourier-encoded
 *                       SkipConnMLP (src/neural_blocks.py:283-287) by one launch, bit-identical to na_fourier_encode's features.  latent
 *                       [N, L] at row pitch lat_ld (NULL with L = 0).
 * na_fourier_encode_backward_input   g_x [N, D] = (lead ? g[:, 0:D] : 0) + sum_f be[:, f] (cos(m_f) g_sin[:, f] - sin(m_f) g_cos[:, f]),
 *                       be = scale * basis, m = x be: the 2F feature-gradient columns [g_sin | g_cos] are read in place at column col0 of rows of pitch g_ld (the standalone
 *                       encoder: g_ld = 2F, col0 = 0, lead = 0; init rows: g_ld = D + 2F + L, col0 = D, lead = 1 adds the raw columns'
 *                       gradient).  No atomics: bitwise reproducible, and the same bits for every pitch and column offset (F a multiple
 *                       of 4: 16-byte loads at 4-byte alignment; any other F a lane-strided form).
 * na_fourier_encode_backward_input_saved   the same with sin / cos read back from the forward's rows (`saved`, pitch s_ld, the sine
 *                       columns at s_col0) instead of recomputed: the alternative tools/fourier_grad_bench.py times against it. */
int na_fourier_rows(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* latent, int L, int64_t lat_ld,
                    float* rows, void* stream);
int na_fourier_encode_backward_input(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* g, int g_ld,
                                     int col0, int lead, float* g_x, void* stream);
int na_fourier_encode_backward_input_saved(const float* x, int64_t N, int D, const float* basis, int F, float scale, const float* g,
                                           int g_ld, int col0, int lead, const float* saved, int s_ld, int s_col0, float* g_x,
                                           void* stream);
/* The optimiser step of runner.py:448-458 (optim.Adam(params, lr, eps = 1e-7); amsgrad / maximize / weight decay off) for n tensors
 * by ONE launch: per element the operations of torch's foreach Adam in its order and rounding (fma_mask: which of its three
 * multiply-adds ATen contracts -- bit 0 lerp, bit 1 addcmul, bit 2 addcdiv; nerf_atlas_amd/train.py holds the value pinned against
 * torch bit for bit).  params / grads / exp_avg / exp_avg_sq: HOST arrays of n device pointers, numel[n]; the scalars as torch's
 * Python computes them in double: 1 - beta1, beta2, 1 - beta2, sqrt(1 - beta2^t), eps, -lr / (1 - beta1^t). */
int na_adam_step(int n, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                 const int64_t* numel, double one_minus_beta1, double beta2, double one_minus_beta2, double bias_correction2_sqrt,
                 double eps, double neg_step_size, int fma_mask, void* stream);
/* The optimiser table of runner.py:440-458 (optim.SGD / RMSprop / Adam with --decay / AdamW as the reference builds them: no momentum,
 * not centered, no amsgrad) the same way: n tensors by ONE launch per 48 non-empty tensors, per element torch's foreach operations in
 * torch's order, each rounded like the ATen kernel rounds it (nerf_atlas_amd/csrc/optim.hip lists them).  params / grads / state0 /
 * state1: HOST arrays of n device pointers (state0: square_avg or exp_avg, state1: exp_avg_sq; NULL where the rule has no such
 * state), numel[n]; an empty tensor is skipped.  The gradients are never written.  scalars[n_scalars], doubles as torch's Python
 * computes them, rounded to float here:
 *   NA_OPTIM_SGD      1: -lr
 *   NA_OPTIM_RMSPROP  4: alpha, 1 - alpha, eps, -lr
 *   NA_OPTIM_ADAM     7: 1 - beta1, beta2, 1 - beta2, sqrt(1 - beta2^t), eps, -lr / (1 - beta1^t), weight_decay (0: none)
 *   NA_OPTIM_ADAMW    7: the same six, then 1 - lr * weight_decay (1: none)
 * fma_mask: which multiply-adds ATen contracts -- bit 0 lerp, bit 1 addcmul, bit 2 addcdiv, bit 3 add(alpha) (SGD's update, Adam's
 * coupled decay); nerf_atlas_amd/train.py holds the values pinned against torch bit for bit.  The whole list is validated before
 * the first launch. */
enum { NA_OPTIM_SGD = 0, NA_OPTIM_RMSPROP = 1, NA_OPTIM_ADAM = 2, NA_OPTIM_ADAMW = 3 };
enum { NA_OPTIM_MAX_SCALARS = 7 };
int na_optim_step(int rule, int n, float* const* params, const float* const* grads, float* const* state0, float* const* state1,
                  const int64_t* numel, const double* scalars, int n_scalars, int fma_mask, void* stream);
/* Forward-mode derivative of the hash features along a per-point direction e (the deformation network's input
 * Jacobian-vector product that the FFJORD divergence estimate needs: runner.py:697-700, src/utils.py:467-478;
 * src/neural_blocks.py:166-190 is what is differentiated).
 * na_hash_encode_jvp           t_out[N, 32 (+3)] = d hash_encode(x)/dx . e   (rows [e | per-level features])
 * na_hash_encode_jvp_backward  tables_grad += d <g_t, J(x).e> / d tables (the adjoint of the above in the tables)
 * na_ffjord_div                div[N] = <e, d(rigid_dp)/dx . e> from the deformation MLP's outputs est[N, stride] =
 *                              [rigidity | n_ctrl control points | ...] and their directional derivatives est_tangent:
 *                              rigid_dp = bezier(P, t) * sigmoid(est0 / 2)  (src/nerf.py:1267-1278).               */
int na_hash_encode_jvp(const float* x, int64_t N, const float* tables, const float* tangent, int include_input,
                       float* t_out, void* stream);
int na_hash_encode_jvp_backward(const float* x, const float* tangent, int64_t N, const float* g_t, int include_input,
                                float* tables_grad, void* stream);
int na_ffjord_div(const float* est, const float* est_tangent, int est_stride, const float* t, const float* e, int64_t N,
                  int n_ctrl, float* div, void* stream);
int na_laplace_density_backward(const float* sdf, int64_t N, const float* beta, const float* g, float* g_sdf,
                                float* g_beta, void* stream);
int na_bezier_warp_backward(const float* est, int est_stride, const float* t, int64_t N, int n_ctrl,
                            const float* g_out_pts, const float* g_dp, const float* g_rigidity, float* g_est,
                            void* stream);
/* gradient of na_bezier_warp_latent: + g_refl_latent [N, n_rl] (nullable) into the enc_rigidity / latent control columns */
int na_bezier_warp_latent_backward(const float* est, int est_stride, const float* t, int64_t N, int n_ctrl, int n_rl,
                                   const float* g_out_pts, const float* g_dp, const float* g_rigidity,
                                   const float* g_refl_latent, float* g_est, void* stream);
int na_composite_backward(const float* density, const float* feat, const float* ts, const float* rays,
                          int T, int64_t R, int C, int density_kind, int bg_kind, const float* g_out,
                          float* g_density, float* g_feat, void* stream);
/* the same for na_composite_random_bg (src/nerf.py:99-103): d sky / d w_t = -rand[r] for t < T-1; rand carries no gradient */
int na_composite_random_bg_backward(const float* density, const float* feat, const float* ts, const float* rays,
                                    int T, int64_t R, int C, int density_kind, const float* rand, const float* g_out,
                                    float* g_density, float* g_feat, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Layer-synchronous fused renderer (csrc/render_ls.hip): the same operator as na_render_plain_view
 * (PlainNeRF.forward with the View head, src/nerf.py:326-361, src/refl.py:190-207) on the engine that keeps
 * activations in LDS and streams weights straight into registers.  Both MLPs are packed into ONE stream:
 *   w_first / b_first = {init, layers.0..3, out} of PlainNeRF.first  (hash encoder, 4x256, out 65; src/nerf.py:320-324)
 *   w_view  / b_view  = {init, layers.0..3, out} of View.mlp         (5 + 64 latent -> 4x256 -> 3; src/refl.py:201-204)
 * in nn.Linear layout (fp32, device pointers; biases may be NULL).  `pts` ([T,R,3], nullable) replaces o + t d by
 * explicit sample positions (PlainNeRF.from_pts with deformed points, src/nerf.py:337-361).  A ray's 32-step blocks
 * pass through one sample group in step order, so the transmittance product of src/nerf.py:22-27 is carried inside the
 * kernel: `out`, `alpha`, `weights` are final when it returns (no second launch).  Workspace: 8 B per ray (elev / azim
 * of the ray, written by a pre-kernel and read with scalar loads).  The stream's header names its precision and
 * schedule; a kernel handed a stream packed for anything else writes NaN colours instead of consuming it.          */
size_t na_render_ls_packed_bytes(int precision);
int na_render_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                      const float* const* w_view, const float* const* b_view, void* packed, void* stream);
size_t na_render_ls_workspace_bytes(int T, int64_t R);
int na_render_plain_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T,
                            const float* hash_tables, const void* packed, int precision, int sigmoid_kind, int bg_kind,
                            float* alpha, float* weights, float* out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* TinyNeRF (/root/reference/src/nerf.py:278-305 with the intended density = estim[..., 0]) on the same
 * layer-synchronous engine, one kernel per call: sample -> SkipConnMLP(3 -> 6 x 256 -> 4, skip 3, LeakyReLU; src/
 * neural_blocks.py:279-296) -> density | sigmoid_kind(colour) -> alpha compositing (src/nerf.py:22-27,60-80,96-98).
 * na_render_tiny_ls_pack takes the 8 Linears {init, layers.0..5, out} (nn.Linear layout, fp32 device pointers, biases may
 * be NULL).  Same ray / sample indexing, `pts`, alpha / weights outputs and precisions as na_render_plain_view_ls; no
 * workspace.                                                                                                         */
size_t na_render_tiny_ls_packed_bytes(int precision);
int na_render_tiny_ls_pack(int precision, const float* const* w, const float* const* b, void* packed, void* stream);
int na_render_tiny_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const void* packed,
                      int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                      void* stream);

/* The View head + alpha compositing alone on the same engine: VolSDF's second half (/root/reference/
 * src/nerf.py:981-1013 with src/refl.py:190-207 and src/utils.py:50-58).  `feat` holds one row per sample (sample n =
 * t * R + ray, row pitch feat_ld >= 65 floats): column 0 the signed distance, columns 1..64 the latent the SDF network
 * produced; the kernel turns the distance into the Laplace density with scale beta[0] (device pointer), evaluates
 * refl.View (x, elev / azim of the ray, latent -> sigmoid_kind(rgb)) and composites with the density used as it is (no
 * softplus).  beta == NULL: column 0 is a density LOGIT instead, sigma = softplus(column 0 - 1) as PlainNeRF's
 * alpha_from_density (src/nerf.py:60-73) -- NeRFAE's rows from na_ae_front; bg_kind black / white as na_render_plain_view_ls.
 * na_render_view_ls_pack takes View.mlp's 6 Linears {init, layers.0..3, out}.  Workspace and `pts` as for
 * na_render_plain_view_ls.                                                                                          */
size_t na_render_view_ls_packed_bytes(int precision);
int na_render_view_ls_pack(int precision, const float* const* w, const float* const* b, void* packed, void* stream);
int na_render_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* feat, int feat_ld,
                      const float* beta, const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha,
                      float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* VolSDF with the SIREN SDF network (/root/reference/src/sdf.py:278-287: SkipConnMLP 3 -> 5 x 256 -> 1 + 64, sin, skip 3)
 * as ONE kernel: sample -> SIREN -> Laplace density | latent -> refl.View -> compositing (src/nerf.py:981-1013).  The pack
 * call takes the SIREN's 7 Linears {init, layers.0..4, out} and View.mlp's 6; `beta` is the Laplace scale on the device.
 * Workspace, `pts`, precisions and outputs as for na_render_plain_view_ls.                                          */
size_t na_render_volsdf_siren_ls_packed_bytes(int precision);
int na_render_volsdf_siren_ls_pack(int precision, const float* const* w_sdf, const float* const* b_sdf,
                                   const float* const* w_view, const float* const* b_view, void* packed, void* stream);
int na_render_volsdf_siren_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* beta,
                              const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights,
                              float* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SDF ray marching (src/march.py).  Per-ray state lives in caller-owned device arrays; the SDF network
 * is evaluated for ALL rays by na_mlp_forward between the updates (no mask compaction, no host sync) and the updates
 * touch only the rays the reference's boolean-mask code would have touched.  `sdf` is column 0 of an [R, stride] MLP
 * output.  hits/rem/todo are 0/1 bytes.
 *
 * Compacted iterations (src/march.py:37-45, 164-179: the reference evaluates the SDF only for the rays its boolean masks keep):
 * na_compact_rays         idx[0..count) = the rays with live[r] != 0, ASCENDING (deterministic); *count = their number (device
 *                         int32).  idx has room for R + 256 entries (the tail is scratch).
 * na_ray_points_indexed / na_sphere_march_update_indexed / na_bisection_update_indexed: the kernels below on n compacted
 *                         rows -- row i of pts / sdf belongs to ray idx[i]; per-ray state arrays stay full size.
 * na_ray_points           pts[R,3] = r_o + r_d * t, t per ray (t_ray[R]) or t_scalar when t_ray is NULL.
 * na_sphere_march_update  one iteration of sphere_march (src/march.py:39-45): for rem rays  hits |= (sdf < eps) &
 *                         (dist <= far);  dist += sdf;  rem &= !(hits | dist > far).
 * na_sign_change_update   one uniform step `step` of throughput_with_sign_change (src/march.py:96-103): running
 *                         minimum + its step index, first sign change (last_pos / first_neg step indices, -1 = none).
 * na_bisection_update     bisection (src/march.py:159-179): sdf_mid NULL initialises todo and z = (low+high)/2 from
 *                         low/high/sdf_low/sdf_high; otherwise one iteration with the SDF at z.                        */
int na_compact_rays(const uint8_t* live, int64_t R, int32_t* idx, int32_t* count, void* stream);
int na_ray_points_indexed(const float* r_o, const float* r_d, const float* t_ray, const int32_t* idx, int64_t n, float* pts,
                          void* stream);
int na_sphere_march_update_indexed(const float* sdf, int stride, const int32_t* idx, int64_t n, float eps, float far,
                                   float* dist, uint8_t* hits, uint8_t* rem, void* stream);
int na_bisection_update_indexed(const float* sdf_mid, int stride, const int32_t* idx, int64_t n, float eps, float* low,
                                float* high, float* sdf_low, float* sdf_high, float* z, uint8_t* todo, void* stream);
int na_ray_points(const float* r_o, const float* r_d, const float* t_ray, float t_scalar, int64_t R, float* pts,
                  void* stream);
int na_sphere_march_update(const float* sdf, int stride, int64_t R, float eps, float far, float* dist, uint8_t* hits,
                           uint8_t* rem, void* stream);
int na_sign_change_update(const float* sdf, int stride, int64_t R, int step, float* curr_min, int32_t* idxs,
                          int32_t* last_pos, int32_t* first_neg, void* stream);
int na_bisection_update(const float* sdf_mid, int stride, int64_t R, float eps, float* low, float* high, float* sdf_low,
                        float* sdf_high, float* z, uint8_t* todo, void* stream);

/* ---- N4: lights and occlusion (src/lights.py:69-132 Point; src/renderers.py:29-163 occlusion kinds) ----------------
 * na_point_light      Point.forward for N points: dir[N,3] = normalize(center - x) (eps 1e-6), dist[N] = |center - x|,
 *                     spectrum[N,3] = intensity / (4 pi dist^2) (or intensity when distance_decay == 0).  center and
 *                     intensity are one vector (stride 0) or one per point (stride 3: `loc.expand(mask.shape)[mask]`).
 * na_occlusion_apply  out = spectrum * a * v:  att_mode 0 a = 1; 1 a = sigmoid(raw_att) on hidden points only
 *                     (LearnedLighting :65-67); 2 a = sigmoid(raw_att) + 1e-2 (AllLearnedOcc :111-121);  v = 1 where
 *                     visible (or visible == NULL), hidden_value elsewhere (0: LightingWIsect :40-45; sigmoid(alpha):
 *                     LearnedConstantSoftLighting :82-83, JointLearnedConstOcc :143-146).                           */
int na_point_light(const float* x, const float* center, int center_stride, const float* intensity, int intensity_stride,
                   int distance_decay, int64_t N, float* dir, float* dist, float* spectrum, void* stream);
int na_occlusion_apply(const float* spectrum, const uint8_t* visible, const float* raw_att, int att_mode,
                       float hidden_value, int64_t N, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * A hash-encoded SkipConnMLP alone on the layer-synchronous engine (round 4): D-NeRF's deformation network
 * (src/nerf.py:1250-1257 delta_estim = SkipConnMLP(in 3, HashEncoder, 5 x 256, skip 3, out 3 n + 1), evaluated at
 * :1267-1270) at the samples of rays x ts (or explicit pts [T,R,3]); rows y[(t * R + ray) * y_ld + 0..n_out).
 * weights / biases: init, layers.0..4, out (nn.Linear layout).  NA_PREC_F16X (n_out <= 32; the output turns NaN as a whole if an
 * activation saturates the half range, see na_render_plain_view_ls) or, round 6, NA_PREC_BF16X3 -- the three-product bf16 split, the
 * accuracy class of na_mlp_forward's rows, n_out <= 64 (with `--dyn-refl-latent`, src/nerf.py:1246-1248: 3 n + 1 + n rl + 1 rows).
 * The other precisions use na_mlp_forward. */
size_t na_mlp_hash_ls_packed_bytes(int precision);
int na_mlp_hash_ls_pack(int precision, const float* const* weights, const float* const* biases, int n_out, void* packed,
                        void* stream);
int na_mlp_hash_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                   const void* packed, int precision, int n_out, float* y, int64_t y_ld, void* stream);

/* The same for a Fourier-encoded SkipConnMLP: VolSDF's MLP SDF network (src/sdf.py:250-258: SkipConnMLP(in 3, FourierEncoder
 * with 128 frequencies, 6 x 256, skip 3, out 1 + 64), evaluated at src/sdf.py:109-112).  weights / biases: init, layers.0..5,
 * out; basis [3,128] fp32, 16-byte aligned, any extra_scale already multiplied in; rows y[(t * R + ray) * y_ld + 0..65) =
 * (signed distance | 64 latent columns), the layout na_render_view_ls takes as `feat`.  The 256 Fourier features are generated
 * inside the kernel wherever a Linear consumes them; they never exist in HBM.  NA_PREC_F16X only.                         */
size_t na_mlp_fourier_ls_packed_bytes(int precision);
int na_mlp_fourier_ls_pack(int precision, const float* const* weights, const float* const* biases, void* packed, void* stream);
int na_mlp_fourier_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* basis,
                      const void* packed, int precision, float* y, int64_t y_ld, void* stream);

/* Coarse -> fine rendering (BASELINE config 2 "64 + 128"; the reference's sample_pdf, src/nerf.py:1745-1779 with its call site
 * :572-578, is dead code -- INTENDED reading, pinned against an fp64 restatement only: see csrc/basic_ops.hip).
 * na_resample_ts: ts [T] shared coarse steps, weights [T,R] of the coarse pass (rows 0..T-2 are used: weights[:-1]),
 * u NULL (linspace(0,1,N), the reference's `uniform`) or [N,R] draws in [0,1); fine [R,N] (nullable) = the N inverse-cdf
 * positions per ray; merged [R,T+N] (nullable) = coarse and new positions of a ray in increasing order (stable).
 * na_render_plain_view_ls_rayts: na_render_plain_view_ls with per-ray steps ts_ray [R,T] (e.g. `merged`).              */
size_t na_resample_ts_lds_bytes(int T, int N, int with_u);
int na_resample_ts(const float* ts, const float* weights, int64_t R, int T, const float* u, int N, float* fine, float* merged,
                   void* stream);
int na_render_plain_view_ls_rayts(const float* rays, int64_t R, const float* ts_ray, int T, const float* hash_tables,
                                  const void* packed, int precision, int sigmoid_kind, int bg_kind, float* alpha,
                                  float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* Compositing over PER-RAY steps with a backward: the fine pass of coarse -> fine TRAINING (csrc/composite_rayts.hip).
 * ts_ray [R,T]: one increasing row per ray (`merged` of na_resample_ts); density / alpha / weights [T,R], feat [T,R,C] step-major.
 * na_compute_pts_rayts          pts[t, r, :] = r_o[r] + ts_ray[r, t] * r_d[r], na_compute_pts's operation order; pts [T,R,3].
 * na_composite_rayts            na_composite with interval lengths max(ts_ray[r,t+1] - ts_ray[r,t], 1e-5) |d| (the closing one
 *                      1e10 |d|); C = 1..8; bg_kind black / white / random, `rand` [R] the per-ray draw of NA_BG_RANDOM (NULL
 *                      otherwise); alpha / weights NULL or [T,R].  Rows equal to shared steps give na_composite's bits.
 * na_composite_rayts_backward   g_density [T,R], g_feat [T,R,C] (C = 1 or 3) given g_out [R,C]; `rand` as above, it carries no
 *                      gradient, nor do the steps.  No atomics: bitwise reproducible.  The decomposition follows T like
 *                      na_composite_backward's up to 128 steps (rows equal to shared steps: the same bits), 16-step segments go on
 *                      to 256 steps, any longer row takes the one-thread-per-ray chain.
 * na_composite_rayts_backward_form  the same with the decomposition named (measurements, tests): NA_RAYTS_BWD_SEG outside
 *                      17 .. 256 steps is NA_EUNSUPPORTED.
 * A non-finite step or density poisons its own ray only, as far as the reference's arithmetic makes it non-finite.               */
enum { NA_RAYTS_BWD_AUTO = 0, NA_RAYTS_BWD_SEQ = 1, NA_RAYTS_BWD_SEG = 2 };
int na_compute_pts_rayts(const float* rays, int64_t R, const float* ts_ray, int T, float* pts, void* stream);
int na_composite_rayts(const float* density, const float* feat, const float* ts_ray, const float* rays, int T, int64_t R, int C,
                       int density_kind, int bg_kind, const float* rand, float* out, float* alpha, float* weights, void* stream);
int na_composite_rayts_backward(const float* density, const float* feat, const float* ts_ray, const float* rays, int T, int64_t R,
                                int C, int density_kind, int bg_kind, const float* rand, const float* g_out, float* g_density,
                                float* g_feat, void* stream);
int na_composite_rayts_backward_form(const float* density, const float* feat, const float* ts_ray, const float* rays, int T,
                                     int64_t R, int C, int density_kind, int bg_kind, const float* rand, const float* g_out,
                                     float* g_density, float* g_feat, int form, void* stream);

/* The training iteration's FORWARD of PlainNeRF(view) as ONE launch (round 6; runner.py:647-825 drives src/nerf.py:326-361, whose two
 * SkipConnMLPs are src/neural_blocks.py:279-296): na_render_plain_view_ls's kernel in NA_PREC_BF16X3 -- the three-product bf16 split
 * of the training GEMMs -- with explicit sample positions pts [T,R,3], which also leaves in HBM what the backward pass reads: the output
 * rows (bias added, BEFORE the next layer's activation: what na_linear_bwd_partials takes as the next Linear's forward input) of the ten
 * 256-wide Linears, planes[(p * T * R + t * R + ray) * 256 + c], p = 0..4 `first`.init, layers.0..3; 5..9 the View MLP's;
 * view_rows [T*R, 69] = the View MLP's init rows [x, y, z, elev, azim | intermediate] (src/nerf.py:338-357, src/refl.py:190-207: what
 * na_plain_head_rows builds from `first`'s output, which is not materialised), density [T*R] (first.out's column 0) and rgb_pre [T*R, 3]
 * (before the sigmoid).  The layer-by-layer forward (na_linear_bf16x3_pk per Linear) writes every one of those rows AND reads it back as
 * the next layer's input; here the activations stay in LDS and the rows leave as whole 128-byte lines, non-temporal.  packed: na_render_ls_pack(NA_PREC_BF16X3) of the CURRENT weights; out [R,3] receives the kernel's own
 * composited colour (black background; callers that composite with noise or a random background ignore it); workspace:
 * na_render_ls_workspace_bytes.  T * R < 4 194 304 (32-bit row offsets). */
int na_train_plain_view_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                           const void* packed, int sigmoid_kind, float* planes, float* view_rows, float* density, float* rgb_pre,
                           float* out, void* workspace, size_t workspace_bytes, void* stream);

/* PlainNeRF(view) with mip's integrated positional encoding (config 3: src/nerf.py:256-261 hook, :326-361 forward,
 * src/utils.py:23-27, 60-140 cylinder / conic Gaussians) as ONE launch of the layer-synchronous engine, NA_PREC_F16X only.
 * rays [B,H,W,6] of whole crops (pixel radii difference neighbouring rows: H >= 2); ts [T]; weights of `first`
 * ([256,134], [256,390], 3 x [256,256], [65,256]) and of the View MLP ([256,165], [256,421], 3 x [256,256], [3,256]) in the
 * reference's column order [p | enc(p) | IPE 96 | ...]; max_deg - min_deg must be 16.  The 96 IPE features of a sample are
 * generated in the kernel for each of the four Linears that consume them (same arithmetic as na_mip_encode, intended
 * layout; t_end as there).  Outputs, workspace (na_render_ls_workspace_bytes) and the range guard as na_render_plain_view_ls. */
size_t na_render_plain_mip_ls_packed_bytes(int precision);
int na_render_plain_mip_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                const float* const* w_view, const float* const* b_view, void* packed, void* stream);
int na_render_plain_mip_ls(const float* rays, int B, int H, int W, const float* ts, int T, const float* hash_tables,
                           const void* packed, int precision, int mip_kind, int min_deg, int max_deg, float t_end,
                           int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out, void* workspace,
                           size_t workspace_bytes, void* stream);

/* PlainNeRF with the reference's OTHER two colour heads, each as ONE launch of the layer-synchronous engine (NA_PREC_F16X only):
 *   na_render_plain_pos_ls   `--refl-kind pos` (`make original`, makefile:8-13): PlainNeRF.from_pts (src/nerf.py:340-361) with
 *                            refl.Positional (src/refl.py:230-245) -- a second hash-encoded SkipConnMLP (5 x 256, skip 3, its OWN
 *                            HashEncoder tables, latent = the 64 intermediate rows of `first`) -> 3, act, compositing.
 *                            w_pos / b_pos: {init [256,102], layers.0 [256,358], layers.1, layers.2 [256,256], layers.3 [256,358],
 *                            layers.4 [256,256], out [3,256]}, reference column order [p 3 | x 3 + hash 32 | latent 64].
 *   na_render_plain_plv_ls   `--refl-kind pos-linear-view` (`make dnerf`, makefile:106-114): refl.PosLinearView (src/refl.py:248-290):
 *                            pos = SkipConnMLP(hash, 2 x 256) -> act -> [colour 3 | intermediate 64]; view = SkipConnMLP(in
 *                            [x | normalize(r_d)], latent [latent | intermediate], 2 x 128, sin) -> 1; colour * (sigmoid(view) / 2 + 0.5).
 *                            w_head / b_head: {pos.init [256,102+n], pos.layers.0 [256,358+n], pos.layers.1 [256,256], pos.out [67,256],
 *                            view.init [128,134+n], view.layers.0 [128,262+n], view.layers.1 [128,128], view.out [1,128]}.
 *                            n = n_rl in 0..3: DynamicNeRF's refl_latent columns (src/nerf.py:1245-1248, 1272-1278, 1303:
 *                            `--dyn-refl-latent`), rows refl_latent[T * R, rl_ld] (sample t * R + ray), appended to the latent of
 *                            both MLPs as the reference does (src/nerf.py:352-358).  sigmoid_kind: normal | thin | fat | upshifted
 *                            (the activation covers all 67 rows of `pos` inside the kernel: NA_EUNSUPPORTED for the other kinds,
 *                            which the host layer renders through the unfused operators).
 * rays / pts / ts / hash_tables (of `first`) / outputs / range guard as na_render_plain_view_ls; hash_tables_refl [8,65536,4] = the
 * head's own encoder.  workspace: na_render_head_ls_workspace_bytes(T, R) bytes (per-ray scratch + an 8-MiB L2-resident park
 * where a workgroup keeps the raw latent rows of its blocks between the Linears that consume them).                            */
size_t na_render_plain_pos_ls_packed_bytes(int precision);
size_t na_render_plain_plv_ls_packed_bytes(int precision);
size_t na_render_head_ls_workspace_bytes(int T, int64_t R);
int na_render_plain_pos_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                const float* const* w_pos, const float* const* b_pos, void* packed, void* stream);
int na_render_plain_plv_ls_pack(int precision, const float* const* w_first, const float* const* b_first,
                                const float* const* w_head, const float* const* b_head, int n_rl, void* packed, void* stream);
int na_render_plain_pos_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                           const float* hash_tables_refl, const void* packed, int precision, int sigmoid_kind, int bg_kind,
                           float* alpha, float* weights, float* out, void* workspace, size_t workspace_bytes, void* stream);
int na_render_plain_plv_ls(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* hash_tables,
                           const float* hash_tables_refl, const float* refl_latent, int64_t rl_ld, int n_rl, const void* packed,
                           int precision, int sigmoid_kind, int bg_kind, float* alpha, float* weights, float* out,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NeRFAE, `--model ae` (the reference's src/nerf.py:766-840; csrc/ae_front.hip).  The model's FRONT as one launch: per sample
 *     encoded   = encode(p)            SkipConnMLP(in 3, FourierEncoder 128 frequencies, 5 x 128, skip 3, out E)   (src/nerf.py:784-788,822)
 *     encoded   = F.normalize(encoded) when `normalize` != 0 (divide by max(|encoded|, 1e-12))                     (src/nerf.py:824)
 *     first_out = density_tform(encoded)  SkipConnMLP(in E, 5 x 64, skip 3, out 1 + I)                             (src/nerf.py:790-793,826)
 * with the 256 Fourier features generated in the kernel wherever a Linear consumes them and every hidden activation of both
 * networks in registers: only the finished row of a sample reaches memory,
 *     y[(t * R + ray) * y_ld + 0] = first_out[0] (the density logit) | + 1 .. 1 + E = encoded | + 1 + E .. 1 + E + I = first_out[1:],
 * which for E + I = 64 is the `feat` row of na_render_view_ls (column 0 | the 64 latent columns in the order refl.View receives
 * them, src/nerf.py:832-836).  Positions: rays [R,6] x ts [T], or explicit pts [T,R,3] (rays may then be NULL).  basis [3,128] fp32
 * with any extra_scale multiplied in.  na_ae_front_pack takes the 7 Linears {init, layers.0..4, out} of each network (nn.Linear
 * layout, reference column order [hidden | p 3 | sin 128 | cos 128] in the skip layers; biases may be NULL).
 * Arithmetic: the three-product bf16 split (hi * hi + hi * lo + lo * hi, fp32 accumulation) under every `precision` NA_PREC_BF16 /
 * NA_PREC_BF16X3 / NA_PREC_F16X -- operands with fp32's range, so there is no range guard.  E in {16, 32, 64}, I in {32, 64},
 * y_ld >= 1 + E + I; everything else NA_EUNSUPPORTED (the host then runs the per-layer path).
 *
 * The two row operators of the model's differentiable path (widths 1..64, row pitches in floats):
 * na_row_normalize            y = F.normalize(x, dim=-1)  (src/nerf.py:824);  _backward: g_x = (g_y - y <y, g_y>) / max(|x|, 1e-12)
 * na_row_sqnorm_mean          out[0] += mean_n |x_n|^2  (torch.linalg.norm(encoded, dim=-1).square().mean(), src/nerf.py:811); `out`
 *                             zeroed by the caller; reduced through the fixed-point accumulator under na_set_deterministic;
 *                             _backward: g_x = g[0] * 2 x / N.                                                          */
size_t na_ae_front_packed_bytes(int precision, int E, int I);
int na_ae_front_pack(int precision, int E, int I, const float* const* w_enc, const float* const* b_enc,
                     const float* const* w_den, const float* const* b_den, void* packed, void* stream);
int na_ae_front(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* basis, const void* packed,
                int precision, int E, int I, int normalize, float* y, int64_t y_ld, void* stream);
int na_row_normalize(const float* x, int64_t x_ld, int64_t N, int W, float* y, int64_t y_ld, void* stream);
int na_row_normalize_backward(const float* x, int64_t x_ld, const float* g_y, int64_t g_ld, int64_t N, int W, float* g_x,
                              int64_t gx_ld, void* stream);
int na_row_sqnorm_mean(const float* x, int64_t x_ld, int64_t N, int W, float* out, void* stream);
int na_row_sqnorm_mean_backward(const float* x, int64_t x_ld, const float* g, int64_t N, int W, float* g_x, int64_t gx_ld,
                                void* stream);

/* ---------------------------------------------------------------------------------------------
 * NeRFVoxel (src/nerf.py:401-524): a dense S^3 grid, densities [S,S,S,1] and rgb [S,S,S,C] (C = 3; another C returns
 * NA_EUNSUPPORTED), read by the reference's 8-neighbour lookup (grid_coords_trilin_weights, src/nerf.py:493-515): neighbours
 * p -+ voxel_len / 2 clamped to +-grid_radius, centres (floor(n / voxel_len + 1e-10) + 0.5) voxel_len clamped to
 * +-(grid_radius - voxel_len / 2), xyz = (p - centre of corner 0) / voxel_len UNclamped (points outside the grid are extrapolated
 * with sign-alternating weights that sum to 1), ids floor(centre / voxel_len + 1e-10) + S / 2.  Cell membership and xyz are fixed in
 * fp32: every operation of that chain is the reference's fp32 operation in its order (no fma contraction, correctly rounded
 * division), with voxel_len etc. the fp32 images of the Python doubles formed from `grid_radius` (a double for that reason).
 * S even, 2 .. 1024.  Positions: explicit pts [T*R,3] (rays / ts may then be NULL), or rays [R,6] x ts [T] formed in the kernel as
 * na_compute_pts forms them, sample n = t * R + r.  Every grid read and every accumulate goes through an id clamped to 0 .. S-1 as an
 * integer: a NaN or Inf coordinate gives NaN in that sample's outputs (and in the <= 8 grid rows its gradient lands in) and
 * touches no other address.
 * raw and g_raw rows are read and written as one 16-byte access: both pointers must be 16-byte aligned.
 * na_voxel_sample           raw [T*R, 1 + C] = [density | C colour parameters], before any activation.
 * na_voxel_sample_backward  g_densities [S^3] += , g_rgb [S^3, C] += the 8 weights x g_raw [T*R, 1 + C] (outputs zeroed by the
 *                           caller; no gradient w.r.t. the positions).  fp32 atomics by default; under na_set_deterministic the
 *                           2^-40 fixed-point path with EVERY contribution converted on its own, so the result is bitwise
 *                           independent of the order of the samples as well (workspace >= 8 * 4 S^3 bytes = 8 MiB at S = 64,
 *                           else NA_EWORKSPACE).
 * na_voxel_render           the eval route as one launch: positions -> lookup -> NA_SIG_* act_kind on the colour parameters ->
 *                           na_composite's arithmetic (softplus(density - 1) form) against NA_BG_BLACK / NA_BG_WHITE; alpha / weights
 *                           NULL or [T,R]; out [R,C].  bg random: composite against black, then na_sky_random.              */
int na_voxel_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, float* raw, void* stream);
int na_voxel_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                             double grid_radius, float* g_densities, float* g_rgb, void* stream);
int na_voxel_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                    int S, int C, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                    void* stream);
/* na_voxel_sample_backward_pts  g_pts [N,3] = the gradient of na_voxel_sample w.r.t. explicit positions pts [N,3] given g_raw [N, 1 + C]
 *                           (16-byte aligned).  In the reference only xyz depends on p -- the floors and both clamps carry no gradient --
 *                           so g_pts[n,a] = (1 / voxel_len) sum_u (dw_u / dxyz_a) (g_raw[n,0] densities[row_u] + sum_c g_raw[n,1+c]
 *                           rgb[row_u,c]) with dw_u / dx = +-(wy wz): the derivative of the cell's (inside the grid: trilinear; outside:
 *                           extrapolating) polynomial.  A gather, no atomics; a non-finite coordinate gives a NaN row.             */
int na_voxel_sample_backward_pts(const float* pts, int64_t N, const float* densities, const float* rgb, const float* g_raw, int S, int C,
                                 double grid_radius, float* g_pts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * NeRFVoxel with the per-voxel pos-linear-view head (PosLinearView.to_voxel, src/refl.py:265-280; csrc/voxel.hip): rgb is
 * [S,S,S,C] with C = 3 + (order+1)^2, a row [raw rgb (3) | (order+1)^2 coefficients of one real spherical-harmonic channel], order 0..4
 * (else NA_EINVAL; 4 is the reference's).  Per sample s = sum_k Y_k(d / max(|d|, 1e-12)) c_k with c_k the interpolated coefficient
 * and d = rays[n % R, 3:6] (un-normalised; rays is required in both position forms), and the colour is
 * act(raw rgb) * (sigmoid(s) / 2 + 0.5).  The lookup, its positions (explicit pts [T*R,3], or rays x ts) and its memory-safety rule are
 * those of na_voxel_sample above; every corner's coefficients are contracted with the ray's basis as the row arrives (d_u = sum_k in
 * k order by fma, then s = sum_u w_u d_u in corner order), so no [N, (order+1)^2] array exists in either direction.  With C % 4 == 0
 * (order 0, 2, 4) rows are read with 16-byte loads and rgb must be 16-byte aligned (else NA_EINVAL); raw and g_raw always.
 * na_voxel_plv_sample               raw [T*R,4] = [density | 3 colour parameters] (na_voxel_sample's layout and arithmetic) and
 *                                   sh [T*R] = s, before any activation.
 * na_voxel_plv_sample_backward      g_densities [S^3] += , g_rgb [S^3,C] += (zeroed by the caller): corner u of sample n receives
 *                                   w_u [g_raw[n,0] | g_raw[n,1..3] | g_sh[n] Y_k].  fp32 atomics by default; under
 *                                   na_set_deterministic every contribution goes to 2^-40 fixed point on its own (bitwise
 *                                   independent of the order of the samples; workspace >= 8 (1 + C) S^3 bytes = 60.8 MB at S = 64,
 *                                   C = 28, else NA_EWORKSPACE before anything is written).  ..._variant runs scatter variant 1
 *                                   (whole rows in the LDS table) or 2 (the four leading sums in the table, the coefficient block
 *                                   straight to memory) for measurements; the plain entry point runs the shipped one.
 * na_voxel_plv_sample_backward_pts  g_pts [N,3] for explicit pts [N,3] (N a multiple of R): na_voxel_sample_backward_pts with the
 *                                   per-corner value g_raw[n,0] densities[row] + sum_c g_raw[n,1+c] rgb[row,c] + g_sh[n] sum_k Y_k
 *                                   rgb[row,3+k].  A gather, no atomics; a non-finite coordinate gives a NaN row.
 * na_voxel_plv_render               the eval route as one launch: the basis once per ray, then per step the lookup, NA_SIG_* act_kind
 *                                   on the colour parameters, the linear scale and na_composite's arithmetic against NA_BG_BLACK /
 *                                   NA_BG_WHITE; alpha / weights NULL or [T,R]; out [R,3].  bg random: black, then na_sky_random. */
int na_voxel_plv_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, float* raw, float* sh, void* stream);
int na_voxel_plv_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                 const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb, void* stream);
int na_voxel_plv_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw,
                                         const float* g_sh, int S, int order, double grid_radius, float* g_densities, float* g_rgb,
                                         int variant, void* stream);
int na_voxel_plv_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                     const float* g_raw, const float* g_sh, int S, int order, double grid_radius, float* g_pts,
                                     void* stream);
int na_voxel_plv_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        int S, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                        void* stream);

/* ---------------------------------------------------------------------------------------------
 * NeRFVoxel with the per-voxel spherical-harmonic colour head (SphericalHarmonic.to_voxel, src/refl.py:715-722; csrc/voxel.hip): rgb is
 * [S,S,S,C] with C = 3 (order+1)^2, channel-major -- coefficient k of colour channel c at c (order+1)^2 + k -- order 0..4.  C does not
 * identify the head (3 is the RGB head's count, 12 the pos-linear-view head's at order 2), so every entry point takes both and returns
 * NA_EINVAL unless C == 3 (order+1)^2.  Per sample s_c = sum_u w_u sum_k Y_k(d / max(|d|, 1e-12)) rgb[row_u, c (order+1)^2 + k] with
 * d = rays[n % R, 3:6]; the colour is act(s_c).  Positions, lookup and memory-safety rule are na_voxel_sample's; each channel block of a
 * corner's row is contracted with the ray's basis as it arrives (d_uc = Y_0 v, then fma in k order; s_c = s_c + w_u d_uc in corner
 * order), so no [N, (order+1)^2] or [N, 3, (order+1)^2] array exists in either direction.  With C % 4 == 0 (orders 1 and 3) rows are read
 * 16 bytes at a time: rgb must then be 16-byte aligned (else NA_EINVAL); raw and g_raw always.
 * na_voxel_sh_sample               raw [T*R,4] = [density | s_r s_g s_b], before any activation: the RGB head's layout.
 * na_voxel_sh_sample_backward      g_densities [S^3] += , g_rgb [S^3,C] += (zeroed by the caller): corner u of sample n receives
 *                                  w_u [g_raw[n,0] | (w_u g_raw[n,1+c]) Y_k], 1 + C sums per row.  fp32 atomics by default; under
 *                                  na_set_deterministic every contribution goes to 2^-40 fixed point on its own (bitwise independent of
 *                                  the order of the samples; workspace >= 8 (1 + C) S^3 bytes = 159 MB at S = 64, C = 75, else
 *                                  NA_EWORKSPACE before anything is written).  ..._variant runs scatter variant 1 (whole rows in the
 *                                  LDS table) or 2 (a pass per colour channel, [density | one channel block] in the table) for
 *                                  measurements; the plain entry point runs the shipped one of the mode.
 * na_voxel_sh_sample_backward_pts  g_pts [N,3] for explicit pts [N,3] (N a multiple of R): na_voxel_sample_backward_pts with the
 *                                  per-corner value g_raw[n,0] densities[row] + sum_c g_raw[n,1+c] d_uc.  A gather, no atomics; a
 *                                  non-finite coordinate gives a NaN row.
 * na_voxel_sh_render               the eval route as one launch: the basis once per ray, then per step the lookup, NA_SIG_* act_kind on
 *                                  s_c and na_composite's arithmetic against NA_BG_BLACK / NA_BG_WHITE; alpha / weights NULL or [T,R];
 *                                  out [R,3].  Bit for bit the three operators in a row.  bg random: black, then na_sky_random. */
int na_voxel_sh_sample(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, float* raw, void* stream);
int na_voxel_sh_sample_backward(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S, int C,
                                int order, double grid_radius, float* g_densities, float* g_rgb, void* stream);
int na_voxel_sh_sample_backward_variant(const float* pts, const float* rays, int64_t R, const float* ts, int T, const float* g_raw, int S,
                                        int C, int order, double grid_radius, float* g_densities, float* g_rgb, int variant, void* stream);
int na_voxel_sh_sample_backward_pts(const float* pts, const float* rays, int64_t R, int64_t N, const float* densities, const float* rgb,
                                    const float* g_raw, int S, int C, int order, double grid_radius, float* g_pts, void* stream);
int na_voxel_sh_render(const float* rays, const float* pts, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                       int S, int C, int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                       void* stream);

/* NeRFVoxel coarse -> fine (`--voxel-steps-fine`, this build's flag; csrc/voxel_fine.hip): a proposal pass over the density
 * grid alone, na_resample_ts, and a fine pass over every ray's own merged row.
 * na_voxel_proposal          one launch: alpha (NULL or [T,R]) and weights [T,R] of rays [R,6] over the shared steps ts [T], from densities
 *                            [S,S,S,1] only -- bit for bit the alpha / weights of na_voxel_render / na_voxel_plv_render /
 *                            na_voxel_sh_render on the same rays, steps and density grid (softplus density, black background).
 * na_voxel_render_rayts      na_voxel_render / na_voxel_plv_render / na_voxel_sh_render over PER-RAY steps ts_ray [R,M] (one increasing row
 * na_voxel_plv_render_rayts  per ray: `merged` of na_resample_ts) in the place of ts [T]; positions are o + t d (there are no explicit
 * na_voxel_sh_render_rayts   pts).  Step lengths are max(ts_ray[r,t+1] - ts_ray[r,t], 1e-5) |d|, the closing one 1e10 |d|.  out [R,3]
 *                            is required, alpha / weights are NULL or [M,R]; bg black or white.  Rows that all equal one shared row
 *                            give the shared-step renderer's three outputs bit for bit.
 * na_voxel_fine_lanes        any of the four with the number of lanes that share a ray named (4, 8, 16, 32, 64; measurements):
 *                            head NA_VOX_HEAD_*, shared_row != 0 reads ts_ray as one [M] row for every ray.
 * Codes as the shared-step renderers': NA_EINVAL shapes / resolution / order / grid_radius / C of the SH head / alignment, NA_ENULL,
 * NA_EUNSUPPORTED activation / bg / C != 3 of the RGB head; R == 0 is NA_OK.                                                          */
enum { NA_VOX_HEAD_RGB = 0, NA_VOX_HEAD_PLV = 1, NA_VOX_HEAD_SH = 2, NA_VOX_HEAD_DENSITY = 3 };
int na_voxel_proposal(const float* rays, int64_t R, const float* ts, int T, const float* densities, int S, double grid_radius, float* alpha,
                      float* weights, void* stream);
int na_voxel_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                          double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out, void* stream);
int na_voxel_plv_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S,
                              int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                              void* stream);
int na_voxel_sh_render_rayts(const float* rays, int64_t R, const float* ts_ray, int M, const float* densities, const float* rgb, int S, int C,
                             int order, double grid_radius, int act_kind, int bg_kind, float* alpha, float* weights, float* out,
                             void* stream);
int na_voxel_fine_lanes(int head, int order, int lanes, int shared_row, const float* rays, int64_t R, const float* ts_ray, int M,
                        const float* densities, const float* rgb, int S, double grid_radius, int act_kind, int bg_kind, float* alpha,
                        float* weights, float* out, void* stream);

/* NeRFVoxel.sparsify (`--voxel-sparsify`, this build's flag; csrc/voxel_sparse.hip): a liveness table over the voxels and
 * a renderer that gathers and walks live steps only.  The grids are not modified.
 * na_voxel_live_table      one launch: keep[v] = !(densities[v] < d_thresh) (a NaN density is kept; the caller's d_thresh is the fp32
 *                          density whose softplus(d - 1) is the threshold, -inf keeps everything), live [S,S,S] uint8:
 *                          live[x,y,z] = any keep[min(x+i,S-1), min(y+j,S-1), min(z+k,S-1)], i, j, k in 0..2.  count: NULL, or one
 *                          int64 that receives the number of non-zero entries.
 * na_voxel_live_samples    flags [M,R] uint8 of the samples n = t R + r: explicit pts [M R,3], or o + ts[r stride + t] d of rays [R,6]
 *                          (stride 0: one shared row ts [M]; else per-ray rows, stride >= M).  A sample is live iff
 *                          live[ix0, iy0, iz0] != 0 for the LOWER ids of the lookup's cell, or a coordinate is not finite.
 * na_voxel_mask_rows       out[n,:] = flags[n] ? x[n,:] : (fill0, 0, .., 0) for x, out [N,C]; in place is allowed.
 * na_voxel_sparse_render   na_voxel_fine_lanes's renderers (head NA_VOX_HEAD_RGB / _PLV / _SH) honouring `live` (required: a table of
 *                          ones renders everything, bit for bit na_voxel_*_render_rayts): a dead sample has alpha = weight = 0 exactly,
 *                          its colour is not read, the walk skips it; step lengths come from the ray's original row.
 * Codes as na_voxel_fine_lanes's; a head outside the three and bad lanes are NA_EINVAL, a NULL table NA_ENULL.                     */
int na_voxel_live_table(const float* densities, int S, float d_thresh, uint8_t* live, int64_t* count, void* stream);
int na_voxel_live_samples(const float* pts, const float* rays, const float* ts, int64_t stride, int M, int64_t R, int S, double grid_radius,
                          const uint8_t* live, uint8_t* flags, void* stream);
int na_voxel_mask_rows(const float* x, const uint8_t* flags, int64_t N, int C, float fill0, float* out, void* stream);
int na_voxel_sparse_render(int head, int order, int lanes, int shared_row, const float* rays, int64_t R, const float* ts, int M,
                           const float* densities, const float* rgb, int S, double grid_radius, const uint8_t* live, int act_kind,
                           int bg_kind, float* alpha, float* weights, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DynamicNeRFVoxel (src/nerf.py:1526-1586; csrc/dyn_voxel.hip): the deformation of a voxel D-NeRF.  ctrl_pts_grid [S,S,S,3(n-1)] holds
 * control points 1 .. n-1 of a Bezier spline per voxel (control point 0 is zero), rigidity_grid [S,S,S,1] a rigidity logit; both are
 * read by NeRFVoxel's lookup above at the UNWARPED pts [N,3] (same cells, same weights, same memory-safety rule), t [N] is the time of
 * each sample (expanded by the caller).  n = n_ctrl is 2 .. 11 (else NA_EUNSUPPORTED), S even, 2 .. 1024.
 * na_dyn_voxel_warp           one launch: dp [N,3] = cubic_bezier (n == 4, src/nerf.py:1201-1206) else de_casteljau (:1173-1178) of the
 *                             interpolated control points at t; rigidity [N] = sigmoid(interpolated logit) (the plain sigmoid);
 *                             warped [N,3] = pts + dp * rigidity.  dp and rigidity may be NULL.  A non-finite coordinate gives NaN in
 *                             that sample's outputs only.
 * na_dyn_voxel_warp_backward  g_ctrl_pts_grid += and g_rigidity_grid += (zeroed by the caller) given any of g_warped [N,3], g_dp [N,3],
 *                             g_rigidity [N] (NULL = zero) and the forward's dp and rigidity: with r the rigidity, G = g_warped,
 *                             D = G r + g_dp and q = (G . dp + g_rigidity) r (1 - r), control block k of the 8 rows gets w_u B_k(t) D and
 *                             the rigidity row w_u q.  No gradient w.r.t. pts.  fp32 atomics by default; under na_set_deterministic
 *                             every contribution goes to 2^-40 fixed point on its own (workspace >= 8 S^3 (1 + 3(n-1)) bytes, else
 *                             NA_EWORKSPACE) and the result is bitwise independent of the order of the samples.                    */
int na_dyn_voxel_warp(const float* pts, const float* t, int64_t N, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int n_ctrl,
                      double grid_radius, float* warped, float* dp, float* rigidity, void* stream);
int na_dyn_voxel_warp_backward(const float* pts, const float* t, int64_t N, const float* dp, const float* rigidity, const float* g_warped,
                               const float* g_dp, const float* g_rigidity, int S, int n_ctrl, double grid_radius, float* g_ctrl_pts_grid,
                               float* g_rigidity_grid, void* stream);
/* na_dyn_voxel_render         DynamicNeRFVoxel's test-time render as ONE launch (csrc/dyn_voxel_render.hip): per ray r of rays [R,6] at
 *                             time t_ray [R] (the reference's time is per batch element; the caller expands it), for the steps ts [T] in
 *                             order: the position o + t d as na_compute_pts forms it, na_dyn_voxel_warp's deformation at it,
 *                             na_voxel_render's lookup at the warped point, activation and compositing step (NA_SIG_* act_kind,
 *                             NA_BG_BLACK / NA_BG_WHITE; bg random: composite against black, then na_sky_random), and the maps of
 *                             runner.py:894-916 summed as na_integrate sums them (acc = acc + w * other, ascending t, from 0):
 *                               out [R,3]; depth [R] = sum w ts; acc [R] = sum of w[:-1]; flow [R,3] = sum w (dp * rigidity);
 *                               rigidity_map [R] = sum w rigidity; alpha, weights [T,R].
 *                             Every output but `out` may be NULL and is then not written; the others' bits do not depend on which are
 *                             asked for.  The result equals, bit for bit, na_compute_pts -> na_dyn_voxel_warp -> na_voxel_render(pts =
 *                             warped) -> na_integrate x 4, without their per-sample arrays.  S even, 2 .. 1024; C == 3 and n_ctrl 2 .. 11
 *                             (else NA_EUNSUPPORTED); T >= 1; R == 0 returns NA_OK without a launch; a NULL required pointer is NA_ENULL
 *                             and named in na_last_error.  Memory safety as above: every grid read goes through an id clamped as an
 *                             integer, and a non-finite coordinate makes that ray's outputs NaN and touches nothing else.          */
int na_dyn_voxel_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities, const float* rgb,
                        const float* ctrl_pts_grid, const float* rigidity_grid, int S, int C, int n_ctrl, double grid_radius, int act_kind,
                        int bg_kind, float* out, float* depth, float* acc, float* flow, float* rigidity_map, float* alpha, float* weights,
                        void* stream);
/* na_dyn_voxel_plv_render     na_dyn_voxel_render over a canonical model with the pos-linear-view head of `order` 0 .. 4 (else NA_EINVAL;
 *                             rgb [S^3, 3 + (order+1)^2], 16-byte aligned where the rows are): same contract and outputs, the canonical
 *                             step being na_voxel_plv_render's (the ray's basis once per thread, the lookup with the coefficients
 *                             contracted in registers, the linear scale).  The result equals, bit for bit, na_compute_pts ->
 *                             na_dyn_voxel_warp -> na_voxel_plv_render(pts = warped) -> na_integrate x 4.                          */
int na_dyn_voxel_plv_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities,
                            const float* rgb, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int order, int n_ctrl,
                            double grid_radius, int act_kind, int bg_kind, float* out, float* depth, float* acc, float* flow,
                            float* rigidity_map, float* alpha, float* weights, void* stream);

/* na_dyn_voxel_sh_render      na_dyn_voxel_render over a canonical model with the spherical-harmonic colour head of `order` 0 .. 4
 *                             (rgb [S^3, C], C == 3 (order+1)^2 else NA_EINVAL; 16-byte aligned at orders 1 and 3): same contract and
 *                             outputs, the canonical step being na_voxel_sh_render's.  The result equals, bit for bit, na_compute_pts ->
 *                             na_dyn_voxel_warp -> na_voxel_sh_render(pts = warped) -> na_integrate x 4.                             */
int na_dyn_voxel_sh_render(const float* rays, const float* t_ray, int64_t R, const float* ts, int T, const float* densities,
                           const float* rgb, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int C, int order, int n_ctrl,
                           double grid_radius, int act_kind, int bg_kind, float* out, float* depth, float* acc, float* flow,
                           float* rigidity_map, float* alpha, float* weights, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Operators on a dense channel-last grid [s0,s1,s2,C], 1 <= C <= 32 (NeRFVoxel's densities and rgb; csrc/grid_ops.hip).
 * na_grid_tv            total_variation (src/nerf.py:381-399) at n flat indices idxs (int64): x = idx % s0, y = (idx / s0) % s1,
 *                       z = (idx / (s0 s1)) % s2 -- x is the fastest digit of idx and the slowest axis in memory, as in the
 *                       reference --, neighbour v + 1 (v - 1 at v == s - 1) per axis, t = sqrt(clamp(dx^2 + dy^2 + dz^2, min = 1e-10))
 *                       per (sample, channel) in the reference's fp32 operations, out[0] = mean of t over the K = n C elements.  One
 *                       launch.  out is TWO floats zeroed by the caller (out[1] counts the arriving waves).  An index outside
 *                       0 .. s0 s1 s2 - 1 is clamped before any address is formed; a NaN / Inf voxel among the sampled rows gives a
 *                       non-finite value.  Under na_set_deterministic the waves' partial sums are combined in 2^-40 fixed point
 *                       (sum of t below 2^23) and the value is bitwise reproducible.
 * na_grid_tv_backward   g_grid [s0,s1,s2,C] += the gradient of that mean times the device scalar g_up[0] (g_grid zeroed by the
 *                       caller): nothing where q = dx^2 + dy^2 + dz^2 < fp32(1e-10), else (dx + dy + dz) w to the voxel and -d w to
 *                       each neighbour, w = (g_up / K) / t; duplicates of an index add up.  fp32 atomics by default; under
 *                       na_set_deterministic every addend goes through 2^-40 fixed point on its own (workspace >= 8 s0 s1 s2 C
 *                       bytes, else NA_EWORKSPACE) and the result is bitwise independent of the order of idxs.
 * na_grid_upsample      dst [R,R,R,C] = F.interpolate(mode="trilinear", align_corners=False) of src [S,S,S,C] (src/nerf.py:377-379):
 *                       per axis scale = (float)S / R, src = max(fmaf(scale, i + 0.5f, -0.5f), 0) in fp32 as torch's builds form it, i0 = floor,
 *                       i1 = min(i0 + 1, S - 1), the output the sum of 8 products.  One launch.  S, R even, 2 .. 1024; R < S samples
 *                       the grid down the same way.                                                                              */
int na_grid_tv(const float* grid, int s0, int s1, int s2, int C, const int64_t* idxs, int64_t n, float* out, void* stream);
int na_grid_tv_backward(const float* grid, int s0, int s1, int s2, int C, const int64_t* idxs, int64_t n, const float* g_up,
                        float* g_grid, void* stream);
int na_grid_upsample(const float* src, int S, float* dst, int R, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Spline-length regularisers of DynamicNeRFVoxel (arc_len, src/nerf.py:1509-1520; csrc/spline_len.hip): the length of the polyline
 * through the M points de_casteljau(control points, t[j]), j = 0 .. M-1, in the reference's fp32 operations.  t [M] is an input table
 * (the caller passes torch.linspace(0, 1, M)'s own values); M is 2 .. 32 (else NA_EUNSUPPORTED).  A segment of length 0 adds 0 to
 * the length and exactly 0 to the gradient.  out is TWO floats zeroed by the caller (na_grid_tv's protocol: out[1] counts the
 * arriving waves); under na_set_deterministic the waves' partial sums are combined in 2^-40 fixed point and the value is bitwise
 * reproducible.  Every entry point is one launch.
 * na_grid_spline_len                 grid [rows, 3 m]: the m = 1 .. 10 control points of a row (no zero point is prepended); idxs [K]
 *                                    int64 flat rows, clamped to 0 .. rows-1 before any address is formed.  lens (NULL or [K]) = the
 *                                    length per index, out[0] = their mean.
 * na_grid_spline_len_backward        g_grid [rows, 3 m] += the gradient of that mean times the device scalar g_up[0] (g_grid zeroed by
 *                                    the caller); duplicates of an index add up.  fp32 atomics by default; under na_set_deterministic
 *                                    every addend goes through 2^-40 fixed point on its own (workspace >= 8 rows 3 m bytes, else
 *                                    NA_EWORKSPACE) and the result is bitwise independent of the order of idxs.
 * na_dyn_voxel_spline_len            per sample of pts [N,3]: control points 1 .. n-1 interpolated from ctrl_pts_grid [S,S,S,3(n-1)] by
 *                                    NeRFVoxel's lookup (the cells, weights and memory-safety rule of na_dyn_voxel_warp) behind the
 *                                    zero control point 0, n = n_ctrl in 2 .. 11.  lens (NULL or [N]) = the length per sample,
 *                                    out[0] = mean over N of w[n] lens[n]; w is NULL (1) or [N].  A non-finite coordinate makes
 *                                    that sample's length, and the value, NaN.
 * na_dyn_voxel_spline_len_backward   g_ctrl_pts_grid += (zeroed by the caller) the gradient of that mean times g_up[0]: control
 *                                    block k of the 8 rows of a sample gets w_u (g_up w[n] / N) sum_j dir_j (B_k(t[j+1]) - B_k(t[j])),
 *                                    dir_j the unit direction of segment j.  No gradient w.r.t. pts or w.  Accumulation modes as
 *                                    na_dyn_voxel_warp_backward (workspace >= 8 S^3 3(n-1) bytes).                                 */
int na_grid_spline_len(const float* grid, int64_t rows, int m, const int64_t* idxs, int64_t K, const float* t, int M, float* lens, float* out,
                       void* stream);
int na_grid_spline_len_backward(const float* grid, int64_t rows, int m, const int64_t* idxs, int64_t K, const float* t, int M,
                                const float* g_up, float* g_grid, void* stream);
int na_dyn_voxel_spline_len(const float* pts, int64_t N, const float* ctrl_pts_grid, int S, int n_ctrl, double grid_radius, const float* w,
                            const float* t, int M, float* lens, float* out, void* stream);
int na_dyn_voxel_spline_len_backward(const float* pts, int64_t N, const float* ctrl_pts_grid, int S, int n_ctrl, double grid_radius,
                                     const float* w, const float* t, int M, const float* g_up, float* g_ctrl_pts_grid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Divergence regularisers of DynamicNeRFVoxel (runner.py:694-700, src/utils.py:461-478; csrc/dyn_voxel_div.hip): quadratic forms of the
 * Jacobian of the deformation w.r.t. the unwarped position.  Only xyzs = (pts - centre) / voxel_len carries a gradient in the
 * reference's lookup, so with w_u the trilinear weights, (sx, sy, sz) = +1 / -1 by the bits of corner u and vl = voxel_len
 *   grad w_u = (sx wy wz, wx sy wz, wx wy sz) / vl,       J_dp v = spline_t(sum_u (v . grad w_u) c_{u,k}),
 *   J_rigid v = s (J_dp v) + dp s (1 - s) sum_u (v . grad w_u) r_u,   s = sigmoid(sum_u w_u r_u),  dp = spline_t(sum_u w_u c_{u,k}).
 * pts [N,3], t [N], the grids, S, n_ctrl (2 .. 11, else NA_EUNSUPPORTED) and grid_radius are na_dyn_voxel_warp's, with its cells,
 * weights, id clamping and memory-safety rule.
 * na_dyn_voxel_jac_quad           one launch: out [N] = v . (J v), J = J_dp if rigidity_grid is NULL (--dyn-diverge-decay: v = ones gives
 *                                 the sum of the nine entries of J_dp, utils.divergence) else J_rigid (--ffjord-div-decay: v the
 *                                 normal draw, utils.div_approx).  v is [N,3] or NULL (= ones, bit for bit).  One thread per sample;
 *                                 the eight rows are read once, nothing per sample but out is written.  A non-finite coordinate
 *                                 gives NaN for that sample only.  N == 0 returns NA_OK without a launch; a NULL required pointer is
 *                                 NA_ENULL and named in na_last_error.
 * na_dyn_voxel_jac_quad_backward  g_ctrl_pts_grid += (zeroed by the caller) the gradient of sum_n g[n] out[n] of the J_dp form:
 *                                 channel 3(k-1) + a of row u of a sample gets g[n] (v . grad w_u) B_k(t) v_a.  The J_rigid form has
 *                                 no gradient in the reference and none here.  No gradient w.r.t. pts, t or v.  Accumulation modes
 *                                 as na_dyn_voxel_warp_backward: fp32 atomics by default; under na_set_deterministic every
 *                                 contribution goes to 2^-40 fixed point on its own (workspace >= 8 S^3 3(n-1) bytes, else
 *                                 NA_EWORKSPACE) and the result is bitwise independent of the order of the samples.             */
int na_dyn_voxel_jac_quad(const float* pts, const float* t, int64_t N, const float* ctrl_pts_grid, const float* rigidity_grid, int S, int n_ctrl,
                          double grid_radius, const float* v, float* out, void* stream);
int na_dyn_voxel_jac_quad_backward(const float* pts, const float* t, int64_t N, int S, int n_ctrl, double grid_radius, const float* v,
                                   const float* g, float* g_ctrl_pts_grid, void* stream);

/* ---------------------------------------------------------------------------------------------
 * SSIM and the pieces of MS-SSIM (Wang et al. with the choices of pytorch_msssim, which the reference calls: src/utils.py:186-195;
 * csrc/ssim.hip).  Images x, y are fp32 channel-last [N,H,W,C], C = 1 .. 4 (else NA_EUNSUPPORTED), read in place.
 * The window G is 11 taps, Gaussian with sigma 1.5, normalised in double and rounded once to fp32, separable, "valid": an H x W image
 * gives an (H-10) x (W-10) map, and H < 11 or W < 11 is NA_EUNSUPPORTED (pytorch_msssim warns and skips the axis).  Per map pixel
 *   mu1 = G*x, mu2 = G*y, s1 = G*(x x) - mu1^2, s2 = G*(y y) - mu2^2, s12 = G*(x y) - mu1 mu2, C1 = (0.01 L)^2, C2 = (0.03 L)^2,
 *   cs = (2 s12 + C2) / (s1 + s2 + C2),   ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) cs,          L = data_range.
 * N == 0 returns NA_OK without a launch; a NULL required pointer is NA_ENULL and named in na_last_error.  Nothing here uses atomics or
 * allocates: every result is bit-identical from run to run in every mode.
 * na_ssim_workspace_bytes  the bytes of workspace na_ssim needs for this shape (0 for a shape it refuses): two floats per 16 x 16
 *                          tile of the map, image and channel.
 * na_ssim                  out [N,C,2] = (mean of ssim, mean of cs) over the map, per (n, c).  Two launches on the stream: one forms
 *                          the moments of a tile with its halo in LDS (the variances centred on the pixel's own means: no
 *                          cancellation) and writes one pair of partial sums per tile to the workspace, the second adds them in a
 *                          fixed order (in double) and divides.  A non-finite pixel makes the means of its own (n, c) NaN and touches
 *                          no other.  A workspace smaller than the query's answer is NA_EWORKSPACE.
 * na_ssim_backward         g_x [N,H,W,C] = the gradient of sum_{n,c} g[n,c] mean_ssim[n,c] w.r.t. x (y takes none); g is [N,C].  With
 *                          B1 = mu1^2 + mu2^2 + C1, B2 = s1 + s2 + C2, A1 = 2 mu1 mu2 + C1, S = ssim:  dS/ds1 = -S / B2,
 *                          dS/ds12 = 2 A1 / (B1 B2),  dS/dmu1 = 2 mu2 (2 s12 + C2) / (B1 B2) - 2 mu1 S / B1,
 *                          dm = dS/dmu1 - 2 mu1 dS/ds1 - mu2 dS/ds12,  g_x = (G^T[dm] + 2 x G^T[dS/ds1] + y G^T[dS/ds12]) g[n,c] /
 *                          ((H-10)(W-10)), G^T the transposed ("full") filter.  One launch; the moments are recomputed per tile; every
 *                          element of g_x is written by exactly one thread.
 * na_image_halve           out_x, out_y [N,Ho,Wo,C] = F.avg_pool2d(kernel 2, padding (H % 2, W % 2), count_include_pad=True) of x and
 *                          y in one launch: Ho = H / 2 + H % 2 (Wo alike), every output is ((a + b) + c) + d times 0.25 with 0 for a
 *                          padded pixel.  y and out_y may both be NULL (one image).                                              */
size_t na_ssim_workspace_bytes(int64_t N, int H, int W, int C);
int na_ssim(const float* x, const float* y, int64_t N, int H, int W, int C, float data_range, float* out, void* workspace,
            size_t workspace_bytes, void* stream);
int na_ssim_backward(const float* x, const float* y, const float* g, int64_t N, int H, int W, int C, float data_range, float* g_x,
                     void* stream);
int na_image_halve(const float* x, const float* y, int64_t N, int H, int W, int C, float* out_x, float* out_y, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The reference's loss wrapper (runner.py:552-594, src/utils.py:198-204, 279-314; csrc/image_loss.hip): --loss-fns
 * l2 | l1 | rmse in --color-spaces rgb | hsv | luminance | xyz under --tone-map and --gamma-correct-loss, of got, ref [P,3] fp32.
 *   gamma (only when gamma != 1)   got <- f(clamp(got, min 1e-10)), ref <- f(ref);  f = sqrt at gamma == 0.5, pow(., gamma) otherwise
 *   tone map (when tone_map != 0)  v <- v / (1 + v) on both
 *   spaces                         rgb: v;  hsv: (0, 0, max v) -- what the reference's rgb2hsv returns --;  luminance: one channel,
 *                                  0.2126 r + 0.7152 g + 0.0722 b;  xyz: the CIE matrix / 0.17697
 *   per space                      l2 = mean d^2, l1 = mean |d|, rmse = sqrt(clamp(l2, min 1e-10)) over P x channels (hsv: 3, luminance: 1)
 *   loss                           mean over the spaces of the mean over the functions
 * A NaN in got makes the loss NaN.  spaces / fns are non-empty masks of NA_SPACE_* / NA_LOSS_*, P >= 1, gamma finite and > 0 (else
 * NA_EINVAL); a NULL pointer is NA_ENULL.  No floating-point atomics: every result is bit-identical from run to run in every mode.
 * na_image_loss_workspace_bytes  the bytes of workspace na_image_loss needs for P pixels (0 for a P it refuses): a 64-byte header and
 *                                eight partial sums per workgroup.
 * na_image_loss                  ONE launch: out[0] = the loss, stats[8] = (mean d^2 of the four spaces in bit order, then mean |d|;
 *                                0 for a space that is off): what the backward needs.  The workspace's first word is an arrival
 *                                counter: it must be 0 before the first call and every call leaves it 0 (one workspace serves any
 *                                number of calls in stream order).  A workspace smaller than the query's answer is NA_EWORKSPACE,
 *                                returned before anything is written.
 * na_image_loss_backward         ONE launch, elementwise: g_got [P,3] = g_up[0] d loss / d got (g_up a device scalar; ref takes none)
 *                                from got, ref and the forward's stats.  Per channel d a / d x = gamma a / x at x >= 1e-10 and exactly 0
 *                                below, d b / d a = 1 / (1 + a)^2; hsv's term goes to the arg-max channel, the lowest index on a tie;
 *                                |d| takes the gradient 0 at d = 0 and the rmse term is exactly 0 while l2 < 1e-10.               */
enum { NA_SPACE_RGB = 1, NA_SPACE_HSV = 2, NA_SPACE_LUMINANCE = 4, NA_SPACE_XYZ = 8 };
enum { NA_LOSS_L2 = 1, NA_LOSS_L1 = 2, NA_LOSS_RMSE = 4 };
size_t na_image_loss_workspace_bytes(int64_t P);
int na_image_loss(const float* got, const float* ref, int64_t P, int spaces, int fns, float gamma, int tone_map, float* out, float* stats,
                  void* workspace, size_t workspace_bytes, void* stream);
int na_image_loss_backward(const float* got, const float* ref, int64_t P, int spaces, int fns, float gamma, int tone_map, const float* stats,
                           const float* g_up, float* g_got, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NERF_ATLAS_AMD_H */
