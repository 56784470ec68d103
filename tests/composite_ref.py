"""Plain fp64 reference of alpha compositing (src/nerf.py:22-27,60-80,96-109 of the reference), the per-element error bounds the
tests hold every compositing kernel to, the inputs they share, an fp32 emulation of the layer-synchronous order and weights that
steer a fused renderer's density.  Imported by tests/test_composite_ref.py (CPU) and tests/test_gpu_composite.py.

Layout: density / alpha / weights [T, R], colours [T, R, C], steps ts [T] (shared) or [R, T] (per ray), directions [R, 3].

THE BOUNDS (derived, not tuned).  u = 2^-24, x = sigma dist, e = exp(-x), a = 1 - e, f = (1 - a) + 1e-10, P_t = prod_{s<t} f_s.

  instruction accuracies (csrc/common.h:74: v_exp_f32, v_log_f32, v_rcp_f32 are 1 ulp = 2u relative), roundings counted in
  csrc/common.h:77-94:
    fast_exp       t = fl(x log2e) with its rounding recovered in r (second order: (88 u)^2), exp2 2u, the closing fma u:
                   EPS_EXP = 3u (+ u/16 for the dropped second-order terms)
    fast_softplus  series branch (e < 2^-6): e with EPS_EXP, the polynomial 1.05u, its truncation e^4/5 <= 0.2u, the product u;
                   log branch: log2 2u, * ln2 u, rcp 2u, e * rcp u, the last product u, U - 1 (U >= 2 only) u = 8u; the quotient
                   e / (U - 1) undoes the rounding of U = fl(1 + e) to second order:  EPS_SOFTPLUS = EPS_EXP + 8u
                   The logit meets `- 1.0f` first: u |v| absolute on v = d - 1 when the difference is inexact, sigmoid(v) / softplus(v)
                   of it relative on sigma.
    fast_sigmoid   e with EPS_EXP (weight 1 - s < 1), the sum u, rcp 2u: EPS_SIGMOID = EPS_EXP + 3u; the `thin` kind adds a product
                   and two sums and 0.98 in fp32: + 4u
    libm (the standalone backward, the register engine): expf, log1pf 1 ulp: EPS_EXP_LIBM = 2u, EPS_SOFTPLUS_LIBM = 4u,
                   sigmoid = 1 / (1 + expf(-v)): 2u + u + 2u
  dist = max(ts[t+1] - ts[t], 1e-5f) |d|: the difference u, 1e-5f against 1e-5 u/2, |d| (three squares, two sums, a root) 2.5u,
  the product u; x = sigma dist one more: 6u.
    eps_x = eps_sigma + 6u
    |da| <= x e eps_x + e EPS_EXP + u a          (x e^-x <= 1/e: <= (eps_sigma + 6u) / e + EPS_EXP + u)
    |df| <= |da| + 2u f                          (1 - a, + 1e-10)
  weights.  w_t = a_t P_t.  An opaque sample has f = 1e-10 in fp32 (a rounds to 1) against e + 1e-10 up to 3e-8 in exact arithmetic:
  its RELATIVE error is unbounded, its absolute error is |df| <= u.  The product is therefore bounded through leave-one-out products,
  D_t >= |P~_t - P_t| exactly as a recurrence over the fp64 values, never dividing by an f:
    D_0 = 0,  D_{t+1} = D_t (f_t + g_t) + g_t P_t,  g_t = |df_t| + u (f_t + |df_t|)       (the product's own rounding folded in)
  (= prod (f_s + g_s) - prod f_s: the sum over s of g_s times the leave-one-out product, all higher orders included; a product
  of n factors carries n - 1 roundings in ANY association -- sequential, a 32-lane scan, a block carry --, KX = 8 more relative
  roundings cover the block product, the carry across at most 5 blocks and the rescaling by the transmittance in front)
    |dw_t| <= |da_t| (P_t + D_t) + a_t D_t + u (a_t + |da_t|)(P_t + D_t) + (t + KX) 2^-126
  (2^-126 per operation: a result below the smallest normal number may be flushed)
  out_c = sum_t w_t c_tc + sky:  sum_t (|dw_t| |c| + (w_t + |dw_t|) |dc|) + (T + 2) u sum_t w_t |c|  (any summation order)
  sky = 1 - sum_{t<T-1} w_t (times the ray's draw for the random background): sum |dw_t| + (T + 1) u sum w_t + u |sky|, + u |out|.

  backward.  dL/da_t = G_t P_t - (sum_{s>t} G_s w_s) / f_t = P_t (G_t - V_t),  V_t = sum_{s>t} G_s a_s prod_{t<r<s} f_r,
  G_t = sum_c g_c c_tc - [t < T-1] sum_c g_c (white; times the draw: random).  The bound is the same expression with absolute
  values inside -- |G|, and Va_{t-1} = |G_t| a_t + f_t Va_t for V -- evaluated as a forward error recurrence, because two of its
  inputs have absolute, not relative, errors (a near 0: u; f of an opaque sample: u against 1e-10):
    dV_{t-1} = dG_t (a_t + da_t) + |G_t| da_t + df_t (Va_t + dV_t) + f_t dV_t,   dG_t = (2C + 2) u |G|_t
    |d dLda_t| <= D_t (|G_t| + Va_t) + (P_t + D_t) (dG_t + dV_t + (T + 4) u (|G_t| + Va_t + dV_t))
  ((T + 4) u: at most T products and sums and one quotient lie between the inputs and dLda_t in either kernel; the quotient by
  f_t cancels the factor f_t every w_s behind t carries, to rounding), and the chain factor K_t = dist_t e_t sigma'(d_t):
    dK_t = dist sigma' e (x eps_x + EPS_EXP_LIBM) + K_t (5u + eps_dsig + 3u)
    |dg_t| <= |d dLda_t| (K_t + dK_t) + |dLda_t| dK_t + (T + 8)(1 + dist_t) 2^-126.
  Against the closed form N u (|G_t| P_t + sum_{s>t} |G_s| w_s / f_t) K_t with N = T + 4 roundings: the recurrence contains that
  term ((P + D)(T + 4) u (|G| + Va)) and adds to it only what the closed form cannot express -- da and df propagated through D,
  dV and dK.  It is therefore LOOSER than the closed form exactly where those absolute errors dominate: behind an opaque sample
  (f = 1e-10 in fp32 against up to 3e-8) and on rays whose alphas are near 0 (da = u against a = 1e-19); there the closed form is
  not a bound at all (fp32 and exact arithmetic differ by more than it allows).  Elsewhere the two agree to the factor
  1 + (eps_sigma + 6u + EPS_EXP_LIBM) x / ((T + 4) u) <= 2 for x <= 10.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from oracle.procedural import proc_uniform

U = 2.0 ** -24
TINY = 2.0 ** -126
KX = 8
EPS_EXP = (3.0 + 1.0 / 16.0) * U
EPS_SOFTPLUS = EPS_EXP + 8.0 * U
EPS_SIGMOID = EPS_EXP + 3.0 * U
EPS_COLOUR_THIN = EPS_SIGMOID + 4.0 * U
EPS_EXP_LIBM = 2.0 * U
EPS_SOFTPLUS_LIBM = 4.0 * U
EPS_SIGMOID_LIBM = 5.0 * U
KINDS = ("softplus", "relu", "laplace")


# ---------------------------------------------------------------------------------------------------------- reference
def sigma_of(density, kind, beta=None):
    """softplus(d - 1) | relu(d) | relu((1 / beta) laplace_cdf(-sdf, beta)) (src/nerf.py:60-68, :1000-1006), in density's dtype"""
    if kind == "softplus":
        return F.softplus(density - 1)
    if kind == "relu":
        return F.relu(density)
    assert kind == "laplace" and beta is not None
    return F.relu((1 / beta) * O.laplace_cdf(-density, beta))


def dists_of(ts, dirs):
    """[T, R] interval lengths: max(ts[t+1] - ts[t], 1e-5) |d|, the closing one 1e10 |d|"""
    tsr = ts[None, :] if ts.dim() == 1 else ts                                   # [1 | R, T]
    d = torch.cat([tsr[:, 1:] - tsr[:, :-1], torch.full_like(tsr[:, :1], 1e10)], dim=1).clamp(min=1e-5)
    return (d * torch.linalg.norm(dirs, dim=-1)[:, None]).t()


def composite_ref(density, feat, ts, dirs, kind="softplus", bg="black", rand=None, beta=None):
    """-> dict(alpha, weights [T,R], out [R,C], sky [R,1]) and the intermediates x, e, f, P the bounds are built from, in the dtype
    of the inputs (fp64 is THE reference, the same code on fp32 inputs is the reference's own fp32 forward)."""
    sigma = sigma_of(density, kind, beta)
    dist = dists_of(ts, dirs)
    x = sigma * dist
    e = torch.exp(-x)
    alpha = 1 - e
    f = 1.0 - alpha + 1e-10
    P = torch.cat([torch.ones_like(f[:1]), torch.cumprod(f, dim=0)[:-1]], dim=0)
    weights = alpha * P
    head = weights[:-1].sum(dim=0).unsqueeze(-1)
    sky = torch.zeros_like(head) if bg == "black" else 1 - head if bg == "white" else rand.reshape(-1, 1) * (1 - head)
    assert bg in ("black", "white", "random")
    out = (weights[..., None] * feat).sum(dim=0) + sky
    return dict(alpha=alpha, weights=weights, out=out, sky=sky, sigma=sigma, dist=dist, x=x, e=e, f=f, P=P)


def oracle_forward(density, feat, ts, dirs, kind="softplus", bg="black", rand=None, beta=None):
    """the same through oracle.alpha_from_density / volumetric_integrate / sky_white / sky_random, one ray at a time when the steps
    are per ray (the oracle differences ts along its last axis: shared steps only)"""
    T, R = density.shape
    if ts.dim() == 2:
        parts = [oracle_forward(density[:, r:r + 1], feat[:, r:r + 1], ts[r], dirs[r:r + 1], kind, bg,
                                None if rand is None else rand[r:r + 1], beta) for r in range(R)]
        return tuple(torch.cat([p[i] for p in parts], dim=(1 if i < 2 else 0)) for i in range(4))
    if kind == "laplace":
        density, kind = (1 / beta) * O.laplace_cdf(-density, beta), "relu"
    alpha, weights = O.alpha_from_density(density.reshape(T, R, 1, 1), ts, dirs.reshape(R, 1, 1, 3), softplus=(kind == "softplus"))
    out = O.volumetric_integrate(weights, feat.reshape(T, R, 1, 1, -1))
    sky = torch.zeros_like(out[..., :1]) if bg == "black" else O.sky_white(weights) if bg == "white" else \
        O.sky_random(weights, rand.reshape(R, 1, 1, 1))
    return alpha.reshape(T, R), weights.reshape(T, R), (out + sky).reshape(R, -1), sky.reshape(R, 1)


def composite_grads(density, feat, ts, dirs, g_out, kind="softplus", bg="black", rand=None):
    """fp64 autograd of sum(out * g_out) -> (g_density [T,R], g_feat [T,R,C])"""
    d = density.double().clone().requires_grad_(True)
    c = feat.double().clone().requires_grad_(True)
    ref = composite_ref(d, c, ts.double(), dirs.double(), kind, bg, None if rand is None else rand.double())
    (ref["out"] * g_out.double()).sum().backward()
    return d.grad, c.grad


# -------------------------------------------------------------------------------------------------------------- bounds
def eps_sigma_of(density, kind, beta=None, libm=False):
    """[T, R] fp64: relative error of sigma as the kernels compute it from the fp32 input `density`"""
    d = density.double()
    if kind == "relu":
        return torch.zeros_like(d)
    if kind == "softplus":
        v = d - 1
        inexact = (density - 1.0).double() != v                    # the fp32 difference
        amp = torch.sigmoid(v) / F.softplus(v).clamp(min=1e-300)   # d log softplus / dv  (-> 1 for v -> -inf)
        return (EPS_SOFTPLUS_LIBM if libm else EPS_SOFTPLUS) + inexact.double() * U * v.abs() * amp
    # (1 / beta) cdf(-sdf / beta): the quotient u, its exp EPS_EXP with |s| u on the exponent, 1 - e / 2 u, 1 / beta u, the product u
    s = (-d / beta).abs()
    es = torch.exp(-s)
    cdf = torch.where(-d <= 0, es / 2, 1 - es / 2)
    return (es / 2 * (s * U + EPS_EXP) + U * cdf) / cdf.clamp(min=1e-300) + 2 * U


def forward_bounds(ref, eps_sigma, feat, err_c=0.0, bg="black", rand=None, eps_exp=EPS_EXP):
    """per-element bounds of alpha, weights [T,R], out [R,C], sky [R,1] (module docstring); ref = composite_ref in fp64,
    err_c the absolute error of the colours (0: they are inputs)"""
    x, e, a, f, P, w = ref["x"], ref["e"], ref["alpha"], ref["f"], ref["P"], ref["weights"]
    T = x.shape[0]
    xe = torch.where(torch.isinf(x), torch.zeros_like(x), x * e)
    da = xe * (eps_sigma + 6 * U) + e * eps_exp + U * a + TINY
    df = da + 2 * U * f
    g = df + U * (f + df)
    D = torch.zeros_like(x)
    for t in range(T - 1):
        D[t + 1] = D[t] * (f[t] + g[t]) + g[t] * P[t]
    D = D + KX * U * (P + D)
    steps = torch.arange(T, dtype=torch.float64)[:, None]
    dw = da * (P + D) + a * D + U * (a + da) * (P + D) + (steps + KX) * TINY
    c = feat.double().abs()
    err_c = torch.as_tensor(err_c, dtype=torch.float64)
    acc = (dw[..., None] * c + (w + dw)[..., None] * err_c).sum(0) + (T + 2) * U * ((w + dw)[..., None] * (c + err_c)).sum(0)
    head = w[:-1].sum(0).unsqueeze(-1)
    dsky = dw[:-1].sum(0).unsqueeze(-1) + (T + 1) * U * head + U * (1 - head).abs()
    if bg == "black":
        dsky = torch.zeros_like(dsky)
    elif bg == "random":
        r = rand.double().reshape(-1, 1)
        dsky = r * dsky + U * r * (1 - head).abs()
    out = acc + dsky + U * ref["out"].abs()
    return dict(alpha=da, weights=dw, out=out, sky=dsky)


def backward_bounds(ref, eps_sigma, density, feat, g_out, kind, bg="black", rand=None):
    """-> (bound of g_density [T,R], bound of g_feat [T,R,C]) for the standalone backward kernels (libm transcendentals)"""
    x, e, a, f, P, w, dist = ref["x"], ref["e"], ref["alpha"], ref["f"], ref["P"], ref["weights"], ref["dist"]
    T, R = x.shape
    C = feat.shape[-1]
    fb = forward_bounds(ref, eps_sigma, feat, eps_exp=EPS_EXP_LIBM)
    da, dw = fb["alpha"], fb["weights"]
    df = da + 2 * U * f
    g = df + U * (f + df)
    D = torch.zeros_like(x)
    for t in range(T - 1):
        D[t + 1] = D[t] * (f[t] + g[t]) + g[t] * P[t]
    D = D + KX * U * (P + D)
    go = g_out.double()
    gsky = torch.zeros(R, dtype=torch.float64) if bg == "black" else go.sum(-1) if bg == "white" else go.sum(-1) * rand.double().reshape(-1)
    head = torch.ones(T, 1, dtype=torch.float64)
    head[T - 1] = 0
    G = (feat.double() * go[None]).sum(-1) - head * gsky[None]
    Gabs = (feat.double() * go[None]).abs().sum(-1) + head * gsky.abs()[None]
    dG = (2 * C + 2) * U * Gabs
    V, Va, dV = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    for t in range(T - 1, 0, -1):
        V[t - 1] = G[t] * a[t] + f[t] * V[t]
        Va[t - 1] = Gabs[t] * a[t] + f[t] * Va[t]
        dV[t - 1] = dG[t] * (a[t] + da[t]) + Gabs[t] * da[t] + df[t] * (Va[t] + dV[t]) + f[t] * dV[t]
    dLda = P * (G - V)
    d_dLda = D * (Gabs + Va) + (P + D) * (dG + dV + (T + 4) * U * (Gabs + Va + dV))
    v = density.double() - 1
    dsig = torch.sigmoid(v) if kind == "softplus" else (density.double() > 0).double()
    inexact = ((density - 1.0).double() != v).double() if kind == "softplus" else 0.0
    eps_dsig = (EPS_SIGMOID_LIBM + inexact * U * v.abs()) if kind == "softplus" else 0.0
    xe = torch.where(torch.isinf(x), torch.zeros_like(x), x * e)
    K = dist * e * dsig
    dK = dist * dsig * (xe * (eps_sigma + 6 * U) + e * EPS_EXP_LIBM) + K * (8 * U + eps_dsig)
    b_d = d_dLda * (K + dK) + dLda.abs() * dK + (T + 8) * (1 + dist) * TINY
    b_f = (dw + U * (w + dw))[..., None] * go.abs()[None] + TINY
    return b_d, b_f


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (a zero bound demands an exact value: ratio 0 or inf).  A non-finite value where
    the reference is finite is inf, never NaN: a NaN ratio would slip through every `<= 1` and every max()"""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio) | ~torch.isfinite(got), torch.full_like(ratio, float("inf")), ratio)
    return float(ratio.max()) if ratio.numel() else 0.0


# -------------------------------------------------------------------------------------------------------------- inputs
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _dirs(R, seed, norm=None):
    """un-normalised directions, lengths in about [0.4, 1.7] (or exactly `norm` up to rounding)"""
    d = proc_uniform((R, 3), seed, 1.0).astype(np.float64) + np.array([0.0, 0.0, 0.35])
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    scale = (1.05 + 0.65 * proc_uniform((R, 1), seed + 1, 1.0)) if norm is None else np.asarray(norm, dtype=np.float64).reshape(-1, 1)
    return _t(d * scale)


def _steps(T, lo, hi, seed):
    """T increasing steps in [lo, hi], jittered inside their cells"""
    if T == 1:
        return _t(np.array([lo]))
    base = np.linspace(lo, hi, T)
    return _t(base + 0.3 * (hi - lo) / (T - 1) * proc_uniform((T,), seed, 1.0))


def _colours(T, R, seed):
    return _t(0.5 + 0.5 * proc_uniform((T, R, 3), seed, 1.0))


def _half(v):
    """onto the grid of the steerable weights: multiples of 1/2 in [-41, 22.5]"""
    return np.clip(np.rint(np.asarray(v, dtype=np.float64) * 2) / 2, -41.0, 22.5)


A_SIZES = (1, 2, 31, 32, 33, 64, 65)


def input_a(T, R=70):
    """ragged T: generic logits in [-6, 6]; 70 rays = more than one wave of the one-thread-per-ray kernels, T around every multiple
    of the 32-step block of the layer-synchronous kernels and of the 8-step unroll / 16-step segment of the standalone ones"""
    return dict(density=_t(proc_uniform((T, R), 5100 + T, 6.0)), ts=_steps(T, 2.0, 6.0, 5200 + T), dirs=_dirs(R, 5300 + T),
                feat=_colours(T, R, 5400 + T), kind="softplus")


def wall_steps(T):
    return sorted({s for s in (0, 15, 16, 31, 32, 63, 64, T - 2, T - 1) if 0 <= s < T})


def input_b(T=67):
    """walls: ray i has ONE opaque sample (logit +22: sigma 21 over unit steps, e = 7.6e-10 < u, a = 1 in fp32) at wall_steps(T)[i] --
    the last lane of a block (31, 63), the first of the next (32, 64), the backward's segment edge (15, 16), the step in front
    of the closing interval and the closing interval itself -- and -40 everywhere else (a = 0 in fp32 but for the closing interval)"""
    w = wall_steps(T)
    d = np.full((T, len(w)), -40.0)
    for i, s in enumerate(w):
        d[s, i] = 22.0
    return dict(density=_t(d), ts=_t(np.arange(T) + 1.0), dirs=_dirs(len(w), 5500, norm=np.linspace(1.0, 1.5, len(w))),
                feat=_colours(T, len(w), 5501), kind="softplus")


C_LOGITS = tuple(-30.0 + 0.5 * k for k in range(25))
C_NORMS = (1e-3, 1.0, 1e3)


def input_c(T=33):
    """empty rays: -41 everywhere (a = 0) but the last sample, whose logit in [-30, -18] times the 1e10-long closing interval times
    |d| in {1e-3, 1, 1e3} gives an alpha from 3e-7 to 1: only the RELATIVE accuracy of softplus far below 0 gets it right"""
    R = len(C_LOGITS) * len(C_NORMS)
    d = np.full((T, R), -41.0)
    d[T - 1] = np.repeat(np.array(C_LOGITS), len(C_NORMS))
    return dict(density=_t(d), ts=_steps(T, 2.0, 6.0, 5600), dirs=_dirs(R, 5601, norm=np.tile(np.array(C_NORMS), len(C_LOGITS))),
                feat=_colours(T, R, 5602), kind="softplus")


def input_d(T=65):
    """dense fog: logit +5 everywhere, steps 1/2 apart: the transmittance passes 1e-38 (and the smallest denormal) inside the ray"""
    R = 5
    return dict(density=_t(np.full((T, R), 5.0)), ts=_t(2.0 + 0.5 * np.arange(T)), dirs=_dirs(R, 5700, norm=(0.5, 1.0, 1.0, 2.0, 4.0)),
                feat=_colours(T, R, 5701), kind="softplus")


E_SIZES = tuple((T, R) for T in (72, 129, 160) for R in (1, 5, 70, 1517))


def input_e(T, R):
    """pass straddling: 3 or 5 blocks per ray against passes of 2 and 4 blocks, so that rays share passes; ray r has an opaque
    sample (+22 over a step of 4 / T times |d| of 200 to 300: x > 60) at the first or last step of a block, cycling through all
    of them, and thin haze elsewhere (logits in [-12, -6]: x of 1e-3 .. 0.5 per step) so that the wall is SEEN through what lies
    in front of it"""
    edges = sorted({s for b in range((T + 31) // 32) for s in (32 * b, min(32 * b + 31, T - 1))})
    d = 3.0 * proc_uniform((T, R), 5800 + T + R, 1.0).astype(np.float64) - 9.0
    for r in range(R):
        d[edges[r % len(edges)], r] = 22.0
    return dict(density=_t(d), ts=_steps(T, 2.0, 6.0, 5801 + T), dirs=_dirs(R, 5802 + R, norm=250.0 + 50.0 * proc_uniform((R, 1), 5803, 1.0)),
                feat=_colours(T, R, 5804 + T + R), kind="softplus")


F_GAPS = ("equal", "ulp", "0.9e-5", "1.1e-5")


def input_f(T=40, const_logit=None):
    """ties: per-ray steps 0.023 apart, |d| = 40; ray (wall w in {31, 32}, side, gap) has its wall (+22) at step w, logit +2 in front
    of it, haze in [-6, 0] elsewhere, and the interval in front of the wall (side 0) or the wall's own (side 1) of length 0, one ulp,
    0.9e-5 (below the 1e-5 floor) or 1.1e-5 (above it).  const_logit: every sample carries that logit instead and the directions
    have no x component (renderers that derive the position, hence the logit, from the step)"""
    cases = [(w, side, gap) for w in (31, 32) for side in (0, 1) for gap in F_GAPS]
    R = len(cases)
    base = np.linspace(1.0, 1.9, T)
    ts = np.repeat(base[None], R, 0).astype(np.float32)
    d = _half(3.0 * proc_uniform((T, R), 5900, 1.0) - 3.0)
    for r, (w, side, gap) in enumerate(cases):
        i = w - 1 + side                      # the interval [ts[i], ts[i+1]] is the short one
        lo = ts[r, i]
        ts[r, i + 1] = {"equal": lo, "ulp": np.nextafter(lo, np.float32(4)), "0.9e-5": np.float32(lo + np.float32(0.9e-5)),
                        "1.1e-5": np.float32(lo + np.float32(1.1e-5))}[gap]
        d[w, r], d[w - 1, r] = 22.0, 2.0
    assert (np.diff(ts, axis=1) >= 0).all()
    dirs = _dirs(R, 5901, norm=40.0)
    if const_logit is not None:
        d = np.full((T, R), float(const_logit))
        dirs = dirs.clone()
        dirs[:, 0] = 0.0
    return dict(density=_t(d), ts=_t(ts), dirs=dirs, feat=_colours(T, R, 5902), kind="softplus")


G_BETAS = (1e-3, 0.1, 1.5)


def input_g(beta, T=33):
    """sdf mode: signed distances in +-0.5 through the Laplace density with scale beta (1e-3: 0 or 1000; 1.5: nearly flat)"""
    R = 12
    return dict(density=_t(proc_uniform((T, R), 6000, 0.5)), ts=_steps(T, 2.0, 6.0, 6001), dirs=_dirs(R, 6002),
                feat=_colours(T, R, 6003), kind="laplace", beta=float(np.float32(beta)))


H_T = 65
H_RAY = 37
H_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
H_STEPS = (0, 31, 32, H_T - 1)


def input_h(value, step):
    """non-finite: input A (T = 65) with ONE bad logit in ray H_RAY"""
    c = dict(input_a(H_T))
    d = c["density"].clone()
    d[step, H_RAY] = H_VALUES[value]
    c["density"] = d
    return c


def h_args(value, step, bg="white"):
    c = input_h(value, step)
    return dict(density=c["density"], feat=c["feat"], ts=c["ts"], dirs=c["dirs"], kind="softplus", bg=bg)


def h_pattern(value, step):
    """where the reference's own fp32 forward of input H is NaN: alpha, weights [T, R] and out [R] (any channel) as bool"""
    ref = composite_ref(**h_args(value, step))
    return dict(alpha=torch.isnan(ref["alpha"]), weights=torch.isnan(ref["weights"]), out=torch.isnan(ref["out"]).any(-1))


def tiny_forward(pts, c, bg="white", act="thin"):
    """the oracle's TinyNeRF on the steered weights at explicit positions pts [T, R, 3], in the dtype of pts -> composite_ref dict"""
    p = {k: v.to(pts.dtype) for k, v in steer_tiny().items()}
    y = O.skip_mlp(p, "estim.", pts)
    return composite_ref(y[..., 0], O.sigmoid(act)(y[..., 1:]), c["ts"].to(pts.dtype), c["dirs"].to(pts.dtype), "softplus", bg)


def tiny_h_pts(value, step):
    """input H for a renderer whose logit is dictated by the position: p_x of ONE sample of ray H_RAY is NaN / +Inf / -Inf"""
    c = on_grid(input_a(H_T))
    pts = steer_pts(c, tiny=True)
    pts[step, H_RAY, 0] = H_VALUES[value]
    return c, pts


def tiny_h_pattern(value, step):
    """where the reference's fp32 TinyNeRF forward is NaN (the zero weights of the other units make +-Inf a NaN as well: 0 x Inf)"""
    c, pts = tiny_h_pts(value, step)
    ref = tiny_forward(pts, c)
    return dict(alpha=torch.isnan(ref["alpha"]), weights=torch.isnan(ref["weights"]), out=torch.isnan(ref["out"]).any(-1))


def on_grid(c):
    """the same input with its logits on the grid of the steerable weights"""
    c = dict(c)
    c["density"] = _t(_half(c["density"].numpy()))
    return c


@functools.lru_cache(maxsize=None)
def case(name, grid=False):
    """a named input: 'A<T>', 'B', 'B<T>', 'C', 'D', 'E<T>x<R>', 'F', 'G<beta>'; grid: logits on multiples of 1/2 (shared, do not modify)"""
    k, arg = name[0], name[1:]
    if k == "A":
        c = input_a(int(arg))
    elif k == "B":
        c = input_b(int(arg)) if arg else input_b()
    elif k == "C":
        c = input_c()
    elif k == "D":
        c = input_d(int(arg)) if arg else input_d()
    elif k == "E":
        c = input_e(*(int(v) for v in arg.split("x")))
    elif k == "F":
        c = input_f()
    else:
        assert k == "G", name
        c = input_g(float(arg))
    return on_grid(c) if grid and c["kind"] == "softplus" else c


def rays_of(c):
    """[R, 6] rays (origin 0) carrying the directions"""
    return torch.cat([torch.zeros_like(c["dirs"]), c["dirs"]], dim=-1)


def rand_of(c, seed=6100):
    return _t(0.5 + 0.5 * proc_uniform((c["dirs"].shape[0], 1), seed, 1.0))


CASES = tuple(f"A{T}" for T in A_SIZES) + ("B", "C", "D") + tuple(f"E{T}x{R}" for T, R in E_SIZES) + ("F",) + tuple(f"G{b}" for b in G_BETAS)


def reference(c, kind=None, bg="black", rand=None, feat=None):
    """fp64 composite_ref of an input dict (kind overrides the input's density kind)"""
    kind = c["kind"] if kind is None else kind
    feat = c["feat"] if feat is None else feat
    return composite_ref(c["density"].double(), feat.double(), c["ts"].double(), c["dirs"].double(), kind, bg,
                         None if rand is None else rand.double(), c.get("beta"))


# ------------------------------------------------------------------------------- fp32 emulation of the layer-synchronous order
def _scan32(x, op):
    """inclusive 32-lane scan in fp32, doubling distances (the association of a DPP row-shift scan)"""
    x = x.copy()
    d = 1
    while d < 32:
        y = x.copy()
        y[d:] = op(x[d:], x[:-d])
        x, d = y, 2 * d
    return x


def emulate_ls(density, feat, ts, dirs, kind="softplus", bg="black", beta=None):
    """csrc/ls_kernel.h composite / combine in numpy float32: per 32-step block an exclusive product scan of f, the block product and
    block-local colour sums; across the blocks of a ray a carried transmittance that scales them.  libm in fp32 stands in for the
    hardware transcendentals.  density [T,R], feat [T,R,3] -> alpha, weights [T,R], out [R,3] (float32)"""
    f32 = np.float32
    d, c = density.numpy().astype(f32), feat.numpy().astype(f32)
    T, R = d.shape
    tsr = ts.numpy().astype(f32)
    tsr = np.repeat(tsr[None], R, 0) if tsr.ndim == 1 else tsr
    dn = dirs.numpy().astype(f32)
    nrm = np.sqrt((dn[:, 0] * dn[:, 0] + dn[:, 1] * dn[:, 1]) + dn[:, 2] * dn[:, 2]).astype(f32)
    if kind == "softplus":
        v = (d - f32(1.0)).astype(f32)
        sigma = np.where(v > 20, v, np.log1p(np.exp(np.minimum(v, f32(20.0)), dtype=f32), dtype=f32)).astype(f32)
    elif kind == "relu":
        sigma = np.maximum(d, f32(0))
    else:
        sc = f32(beta)
        s = ((-d) / sc).astype(f32)
        cdf = np.where(s <= 0, np.exp(np.minimum(s, f32(0)), dtype=f32) * f32(0.5), f32(1) - np.exp(-np.maximum(s, f32(0)), dtype=f32) * f32(0.5)).astype(f32)
        sigma = np.maximum(((f32(1) / sc) * cdf).astype(f32), f32(0))
    alpha, weights, out = np.zeros((T, R), f32), np.zeros((T, R), f32), np.zeros((R, 3), f32)
    nb = (T + 31) // 32
    for r in range(R):
        gap = np.maximum(tsr[r, 1:] - tsr[r, :-1], f32(1e-5)).astype(f32)
        dist = (np.concatenate([gap, np.array([1e10], f32)]) * nrm[r]).astype(f32)
        cT, acc, cwh = f32(1), np.zeros(3, f32), f32(0)
        for b in range(nb):
            n = min(32, T - 32 * b)
            sl = slice(32 * b, 32 * b + n)
            a = np.zeros(32, f32)
            with np.errstate(over="ignore", under="ignore"):
                a[:n] = f32(1) - np.exp(-(sigma[sl, r] * dist[sl]).astype(f32), dtype=f32)
            f = ((f32(1) - a) + f32(1e-10)).astype(f32)
            fs = np.concatenate([np.array([1], f32), f[:-1]])
            with np.errstate(under="ignore"):
                excl = _scan32(fs, lambda p, q: (p * q).astype(f32))
                w = (a * excl).astype(f32)
                P = f32(excl[31] * f[31])
                col = np.zeros((32, 3), f32)
                col[:n] = c[sl, r]
                s3 = [_scan32((w * col[:, k]).astype(f32), lambda p, q: (p + q).astype(f32))[31] for k in range(3)]
                t_idx = 32 * b + np.arange(32)
                wh = _scan32(np.where(t_idx < T - 1, w, f32(0)).astype(f32), lambda p, q: (p + q).astype(f32))[31]
                mine = cT
                for k in range(3):
                    acc[k] = f32(acc[k] + f32(cT * s3[k]))
                cwh = f32(cwh + f32(cT * wh))
                cT = f32(cT * P)
                alpha[sl, r] = a[:n]
                weights[sl, r] = (w[:n] * mine).astype(f32)
        sky = f32(1) - cwh if bg == "white" else f32(0)
        out[r] = acc + sky
    return torch.from_numpy(alpha), torch.from_numpy(weights), torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------ steerable weights
# A LeakyReLU SkipConnMLP that hands input column p_x through unit 0 of every layer into output row 0: with every other weight zero
# (the skip layers' init columns and the duplicate x column of a hash-encoded MLP included), zero hash tables and out-bias LOGIT_BIAS
# the density logit of a sample is p_x + LOGIT_BIAS EXACTLY in every operand format: p_x = k / 2, k = 0..127, is positive (LeakyReLU is
# the identity), has at most 7 significant bits (exact in bf16, f16 and f16 + fp6) and stays far inside the half range.
LOGIT_BIAS = -41.0
COLOUR_LOGITS = (-1.0, 0.5, 2.0)   # three distinct constant colour logits (exact in every format)
TINY_PY, TINY_PZ = 1.0, 2.0        # TinyNeRF: p_y, p_z of every sample; colour rows u1 - 2, u2 - 1.5, u1 + u2 - 1 = COLOUR_LOGITS


def _mlp(prefix, shapes):
    p = {}
    names = ["init"] + [f"layers.{i}" for i in range(len(shapes) - 2)] + ["out"]
    for n, (o, i) in zip(names, shapes):
        p[f"{prefix}{n}.weight"] = torch.zeros(o, i)
        p[f"{prefix}{n}.bias"] = torch.zeros(o)
    return p, names


def steer_view(prefix="refl.mlp."):
    """refl.View's MLP with all-zero weights: its colour logits are the out-bias"""
    p, _ = _mlp(prefix, [(256, 69), (256, 325), (256, 256), (256, 256), (256, 256), (3, 256)])
    p[prefix + "out.bias"] = torch.tensor(COLOUR_LOGITS)
    return p


def steer_plain():
    """PlainNeRF (hash-encoded first MLP 38 -> 65, View head): state dict with zero hash tables"""
    p, names = _mlp("first.", [(256, 38), (256, 294), (256, 256), (256, 256), (256, 256), (65, 256)])
    for n in names:
        p[f"first.{n}.weight"][0, 0] = 1.0
    p["first.out.bias"][0] = LOGIT_BIAS
    for i in range(8):
        p[f"first.enc.embs.{i}.weight"] = torch.zeros(65536, 4)
    p.update(steer_view())
    return p


def steer_tiny():
    """TinyNeRF.estim (3 -> 4, six hidden layers, skips at 0 and 3): unit 0 carries p_x, units 1 and 2 carry p_y and p_z"""
    p, names = _mlp("estim.", [(256, 3), (256, 259), (256, 256), (256, 256), (256, 259), (256, 256), (256, 256), (4, 256)])
    for n in names[:-1]:
        for k in range(3):
            p[f"estim.{n}.weight"][k, k] = 1.0
    W, b = p["estim.out.weight"], p["estim.out.bias"]
    W[0, 0] = 1.0
    W[1, 1] = 1.0
    W[2, 2] = 1.0
    W[3, 1] = W[3, 2] = 1.0
    b[0], b[1], b[2], b[3] = LOGIT_BIAS, -2.0, -1.5, -1.0
    return p


def mlp_lists(p, prefix):
    """(weights, biases) in the order init, layers.., out"""
    n = 0
    while f"{prefix}layers.{n}.weight" in p:
        n += 1
    names = ["init"] + [f"layers.{i}" for i in range(n)] + ["out"]
    return [p[f"{prefix}{k}.weight"] for k in names], [p[f"{prefix}{k}.bias"] for k in names]


def steer_pts(c, tiny=False):
    """explicit sample positions [T, R, 3] dictating the (grid) logits of an input: p_x = logit - LOGIT_BIAS"""
    d = c["density"].double()
    px = d - LOGIT_BIAS
    assert bool(((px * 2) == (px * 2).round()).all()) and float(px.min()) >= 0 and float(px.max()) <= 63.5, "logits off the grid"
    py = torch.full_like(px, TINY_PY if tiny else 0.0)
    pz = torch.full_like(px, TINY_PZ if tiny else 0.0)
    return torch.stack([px, py, pz], dim=-1).float()


def colour_of(kind="thin"):
    """the three constant colours of the steered heads, fp64"""
    return O.sigmoid(kind)(torch.tensor(COLOUR_LOGITS, dtype=torch.float64))


def view_feat(c, ld=65):
    """rows of na_render_view_ls: column 0 the logit / signed distance, the latent (and the padding of a wider row) zero"""
    T, R = c["density"].shape
    rows = torch.zeros(T, R, ld)
    rows[..., 0] = c["density"]
    return rows
