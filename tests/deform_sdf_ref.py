"""Plain references of the small operators of the D-NeRF and VolSDF paths -- the spline warp and its gradient, the FFJORD divergence,
the Laplace density, the forward-mode tangent operators, normalize3 / PosLinearView combine / point light, the marching state machines
(csrc/basic_ops.hip, csrc/backward.hip, csrc/march.hip) --, the error bounds the tests hold the kernels to, and the inputs they share.
Imported by tests/test_deform_sdf_ref.py (CPU), tests/test_gpu_deform_sdf.py and tests/test_gpu_march_edges.py.

THE REFERENCES are fp64 restatements built from oracle/nerf_oracle.py and plain torch; gradients are torch autograd in fp64; the
divergence is torch.autograd.functional.jvp of est -> dp(est) * rig(est) along the tangent rows, dotted with e (an independent route:
tests/test_deform_sdf_ref.py holds it against the closed form the kernel writes out).  The marching steps are vectorised torch on
fp32 state tensors and are compared EXACTLY: every operation in them is a comparison or one fp32 add / halving of given values.

THE BOUNDS (derived, not tuned; first order in u = 2^-24; "mag" is the same expression on absolute values, so cancellation is paid for).
  transcendentals   fast_exp: 2e-7 relative (csrc/common.h).  expf / sinf / cosf of the device libm: E_exp (relative), E_sin, E_cos
                    (absolute) = max(2 u, twice the worst error of torch.exp / sin / cos ON THE SAME GPU against fp64 over `libm_probe()`,
                    |x| <= 100); `set_libm` installs them, the default (CPU tests) is the floor 2 u.
  sigmoid           s = 1 / (1 + expf(-v)): E_exp on the exponential, one add, one division: SIG = E_exp + 2 u relative to s; an
                    exponential that under- / overflows leaves s at 0 or 1 where fp64 is 4e-44 away: + TINY = 2^-126 on every entry
                    that holds a sigmoid.  1 - s inherits s SIG absolutely (the cancellation near s = 1 is paid with s SIG, not q SIG).
  warp forward      m1t = 1 - t (u); a de Casteljau level is two products and an add of terms that carry m1t: 3 u per level, n - 1 levels,
                    one of slack: dp within (3 (n - 1) + 1) u mag(dp); the cubic form's ten roundings meet the same constant at n = 4.
                    rig within SIG rig + TINY; warped = pts + dp rig: bound(dp) rig + |dp| bound(rig) + u |dp rig| + u (|pts| + |dp rig|);
                    latent = v s like dp rig, one product: + u |v s|.
  warp backward     Bernstein recurrence: 3 u per level on B_k (mag: binomial |t|^k |1 - t|^(n-1-k)); dp = sum B_k P_k: n products, n - 1
                    adds: (4 n - 3) u mag.  ge[0] = D rig (1 - rig) / 2, D = g_rig + <g_pts, dp>: (4 n + 6) u mag + D_mag rig SIG / 2 + TINY;
                    ge[P_ka] = B_k (g_pts rig + g_dp): B_mag ((3 (n - 1) + 3) u mag + |g_pts| rig SIG) + TINY; the latent columns alike
                    (ge[s] sums n_rl more addends).  Columns behind the used ones: bound 0.
  divergence        sum_a e_a (ddp_a rig + dp_a drig), drig = rig (1 - rig) / 2 * tan_0: (4 n + 4) u (T1 + T2) + SIG (T1 + T2) + 4 u T2
                    + sum |e| mag(dp) |tan_0| rig^2 SIG / 2 + TINY, T1 = sum |e| mag(ddp) rig, T2 = sum |e| mag(dp) |drig|.
  Laplace density   a = |sdf| / beta; scaled (u: a u on the exponent), fast_exp, 1 / beta (u), product (u), one of slack:
                    sdf >= 0: ref (2e-7 + a u + 4 u), 4e-7 where a log2(e) > 126: there the kernel squares exp(-a / 2), one more product,
                    because v_exp_f32 flushes a denormal result (csrc/basic_ops.hip laplace_density_of); sdf < 0: (exp(-a) / 2 (2e-7 + a u) + u (1 - exp(-a) / 2)) / beta + 2 u ref; a result
                    in the denormal range is rounded to a multiple of 2^-149 before and after the scaling: + 2^-149 (1 / beta + 1).
                    backward: expf (E_exp), r^2 (3 u), products: g_sdf = (-g e) r^2 within ref (E_exp + a u + 6 u) + 2^-149 ((|g| + 1/2) / beta^2 + 1)
                    (a denormal e = expf / 2 is off by 2^-149, the product g e by 2^-150 BEFORE it is scaled by r^2); a NaN sdf gets 0, like
                    torch's clamp; g_beta: the
                    terms e v / beta^3 and cdf / beta^2 within (E_exp + a u + 10 u) mag each, the sum of P = ceil(N / 256) workgroups'
                    partials (6 shuffle levels, 2 adds, P - 1 atomics, 1 slack): (8 + P) u mag.  Deterministic mode is not exercised here.
  tangents          act' / act'': cosf / -sinf within E_cos / E_sin, the piecewise ones exact; mul_bcast: u |ref|; mul_reduce over J: J u mag.
                    (mul_bcast, and mul_reduce at J = 1, are ONE correctly rounded product: u |ref| is then round-to-nearest's own
                    guarantee, |err| <= u |exact| / (1 + u) -- met by construction, without slack, and a worst ratio just under 1 is
                    what a correct kernel shows over thousands of products; any second rounding would leave it.)
  eikonal           |n| within 3 u |n| (three squares, two adds, sqrtf), d = |n| - 1 one more u: per row (2 |d| (3 |n| + |d|) + d^2) u / N, the sum
                    like g_beta plus 1 / N and its product: (11 + P) u loss.  backward: |x| |g| 2 / N ((3 |n| + |d|) / |n| + 8 |d| / |n|) u.
  normalize3        5 u |ref| (2.5 u on the norm, the division, fp32(1e-12) against 1e-12, slack); a zero row is exact.
  PosLinearView     (s / 2 + 0.5) pos: |pos| (s SIG / 2 + u (s / 2 + 0.5)) + u |ref|; g_pos the same with g; g_lin = acc s (1 - s) / 2:
                    (C + 5) u mag + sum |g pos| s SIG / 2 + TINY.  Columns at or beyond C_out: bound 0.
  point light       direction 6 u |ref|, distance 4 u |ref|, spectrum 12 u |ref| (differences u, squares and adds 5 u, sqrtf, 4 pi in fp32).
An entry whose bound is 0 must be exact.  No element is left out: where a result depends on which side of a threshold an input
falls (the LeakyReLU kink, the 1e-12 / 1e-6 norms, eps, far, the sign of an SDF value), the inputs are exactly on the threshold or at
least 1e-3 of its scale away, and `clean_*` below ASSERT that for every input set the GPU tests use.

MEASURED on an MI355X (tests/test_gpu_deform_sdf.py prints them: worst |err| / bound over every entry of every case).
  libm: torch.exp 7.9e-8 relative, torch.sin 6.1e-8, torch.cos 6.6e-8 absolute over libm_probe() -> E_exp 1.59e-7, E_sin 1.23e-7, E_cos 1.31e-7.
  warp: warped 0.85, dp 0.58, rigidity 0.42, latent 0.46; warp backward 0.42; divergence 0.22;
  Laplace: forward 0.54 (0.89 on the sweep of sdf > 0 down to the denormals), g_sdf 0.54, g_beta 0.06;
  act' 0.51, act'' 0.48, LeakyReLU / none exact; mul_bcast 0.988 and mul_reduce 0.995 (J = 1: ONE rounding against u |ref|, see above); eikonal 0.16, its
  gradient 0.45; normalize3 0.46; PosLinearView 0.86, g_lin 0.28, g_pos 0.87; light direction 0.51, distance 0.57, spectrum 0.48.
  The marching kernels equal the restatement bit for bit.

NOT COVERED: the second sweep of the grid-stride loops (more than 32768 workgroups' worth of rows: about a gigabyte of `est` for
the staged warp), the deterministic accumulation mode of g_beta / eikonal, the
sigmoid-kind kernels and the occlusion kinds.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import oracle as O
from grid_ref import U
from oracle.procedural import proc_uniform

TINY = 2.0 ** -126
DENORM = 2.0 ** -149
FAST_EXP_REL = 2e-7
CLEAR = 1e-3            # "well clear" of a threshold: at least this fraction of its scale
LIBM = {"exp": 2 * U, "sin": 2 * U, "cos": 2 * U}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def worst_ratio(got, ref, bound):
    """max over ALL entries of |got - ref| / bound (bound 0: the entry must be exact -- ratio 0 or inf); NaN where the two disagree about
    NaN; entries that are NaN in both, or the same infinity in both, count as equal"""
    got = got.detach().cpu().double().reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand(ref.shape)
    if bool((torch.isnan(got) != torch.isnan(ref)).any()):
        return float("nan")
    same = (torch.isnan(got) & torch.isnan(ref)) | (got == ref)
    err = torch.where(same, torch.zeros_like(ref), (got - ref).abs())
    ratio = torch.where(same, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def uniform(shape, seed, amp=1.0):
    return _t(proc_uniform(tuple(shape), seed, amp))


# ------------------------------------------------------------------------------------------------------------ libm
@functools.lru_cache(maxsize=None)
def libm_probe():
    """the arguments the transcendental accuracy is measured on: |x| <= 100, dense near 0 (callers must not modify it)"""
    return torch.cat([uniform((1 << 16,), 6000, 100.0), uniform((1 << 14,), 6001, 10.0), uniform((1 << 14,), 6002, 1.0)])


def libm_errors(exp_f32, sin_f32, cos_f32):
    """worst errors of fp32 results on libm_probe() against fp64: exp relative (where the result is a normal number), sin / cos absolute"""
    x = libm_probe().double()
    ok = x.abs() <= 87.0
    e = ((exp_f32.cpu().double() - x.exp()).abs() / x.exp())[ok].max()
    return dict(exp=float(e), sin=float((sin_f32.cpu().double() - x.sin()).abs().max()),
                cos=float((cos_f32.cpu().double() - x.cos()).abs().max()))


def set_libm(measured):
    """install E = max(2 u, 2 x measured) for exp / sin / cos"""
    for k in ("exp", "sin", "cos"):
        LIBM[k] = max(2 * U, 2.0 * float(measured[k]))


def sig_rel():
    return LIBM["exp"] + 2 * U


# ------------------------------------------------------------------------------------------------------------ spline warp
def est_min_width(n, n_rl=0):
    return 1 + 3 * n if n_rl == 0 else 2 + (3 + n_rl) * n


def warp_fp64(e, pts, td, n, n_rl=0):
    """e [N, >= min] / pts [N,3] / td [N,1], all fp64 -> (warped, dp, rig [N,1], latent [N,n_rl] | None, unscaled latent | None);
    src/nerf.py:1267-1278 through the oracle's curves"""
    N = e.shape[0]
    rig = torch.sigmoid(e[:, :1] / 2)
    fn = O.cubic_bezier if n == 4 else O.de_casteljau
    P = e[:, 1:1 + 3 * n].reshape(N, n, 3).permute(1, 0, 2)
    dp = fn(P, td, n).reshape(N, 3)
    warped = pts + dp * rig
    if n_rl == 0:
        return warped, dp, rig, None, None
    s = torch.sigmoid(e[:, 3 * n + 1:3 * n + 2])
    C = e[:, 3 * n + 2:3 * n + 2 + n * n_rl].reshape(N, n, n_rl).permute(1, 0, 2)
    v = fn(C, td, n).reshape(N, n_rl)
    return warped, dp, rig, v * s, v


def bernstein(td, n, mag=False):
    """[N, n] Bernstein weights of degree n - 1 at td [N,1] fp64 (mag: of |t| and |1 - t|)"""
    a, b = (td.abs(), (1 - td).abs()) if mag else (td, 1 - td)
    return torch.cat([math.comb(n - 1, k) * a ** k * b ** (n - 1 - k) for k in range(n)], dim=1)


def curve_mag(e_cols, td, n, width):
    """sum_k B_mag_k |P_k|: e_cols [N, n * width] fp64 -> [N, width]"""
    N = e_cols.shape[0]
    return (bernstein(td, n, True).unsqueeze(-1) * e_cols.reshape(N, n, width).abs()).sum(1)


def warp_ref(est, pts, t, n, n_rl=0):
    """fp32 inputs (est [N, S >= min]: trailing columns unused) -> dict of fp64 references and per-entry bounds of the four outputs"""
    e, p, td = est.double(), pts.double(), t.double().reshape(-1, 1)
    warped, dp, rig, enc, v = warp_fp64(e, p, td, n, n_rl)
    c = 3 * (n - 1) + 1
    dp_b = c * U * curve_mag(e[:, 1:1 + 3 * n], td, n, 3)
    rig_b = sig_rel() * rig + TINY
    dr = (dp * rig).abs()
    out = dict(warped=warped, dp=dp, rig=rig, dp_b=dp_b, rig_b=rig_b,
               warped_b=dp_b * rig + dp.abs() * rig_b + U * dr + U * (p.abs() + dr))
    if n_rl:
        s = torch.sigmoid(e[:, 3 * n + 1:3 * n + 2])
        vmag = curve_mag(e[:, 3 * n + 2:3 * n + 2 + n * n_rl], td, n, n_rl)
        out.update(enc=enc, enc_raw=v, enc_b=c * U * vmag * s + v.abs() * (sig_rel() * s + TINY) + U * enc.abs())
    return out


def warp_backward_ref(est, t, n, n_rl=0, g_pts=None, g_dp=None, g_rig=None, g_enc=None):
    """fp64 autograd of sum <g, output> w.r.t. est [N,S] and its per-entry bound; an absent upstream gradient is zero"""
    N, S = est.shape
    e = est.double().requires_grad_()
    td = t.double().reshape(-1, 1)
    zero3 = torch.zeros(N, 3, dtype=torch.float64)
    warped, dp, rig, enc, _ = warp_fp64(e, zero3, td, n, n_rl)
    d = lambda g, shape: torch.zeros(shape, dtype=torch.float64) if g is None else g.double().reshape(shape)
    gw, gd, gr = d(g_pts, (N, 3)), d(g_dp, (N, 3)), d(g_rig, (N, 1))
    loss = (gw * warped).sum() + (gd * dp).sum() + (gr * rig).sum()
    if n_rl and g_enc is not None:
        loss = loss + (g_enc.double().reshape(N, n_rl) * enc).sum()
    (ge,) = torch.autograd.grad(loss, e, allow_unused=False) if loss.requires_grad else (torch.zeros_like(e),)
    e = e.detach()
    Bm = bernstein(td, n, True)                                  # [N, n]
    r, q = rig.detach(), 1 - rig.detach()
    dpm = curve_mag(e[:, 1:1 + 3 * n], td, n, 3)
    Dm = gr.abs() + (gw.abs() * dpm).sum(1, keepdim=True)
    b = torch.zeros(N, S, dtype=torch.float64)
    b[:, :1] = (4 * n + 6) * U * (0.5 * Dm * r * q) + 0.5 * Dm * r * sig_rel() + TINY
    ddm = gw.abs() * r + gd.abs()                                # [N, 3]
    per = (3 * (n - 1) + 3) * U * ddm + gw.abs() * r * sig_rel() + TINY
    b[:, 1:1 + 3 * n] = (Bm.unsqueeze(-1) * per.unsqueeze(1)).reshape(N, 3 * n) + TINY
    if n_rl and g_enc is not None:
        g = g_enc.double().reshape(N, n_rl).abs()
        s = torch.sigmoid(e[:, 3 * n + 1:3 * n + 2])
        vm = curve_mag(e[:, 3 * n + 2:3 * n + 2 + n * n_rl], td, n, n_rl)
        Ds = (g * vm).sum(1, keepdim=True)
        b[:, 3 * n + 1:3 * n + 2] = (4 * n + n_rl + 2) * U * Ds * s * (1 - s) + Ds * s * sig_rel() + TINY
        per = g * s * ((3 * (n - 1) + 2) * U + sig_rel()) + TINY
        b[:, 3 * n + 2:3 * n + 2 + n * n_rl] = (Bm.unsqueeze(-1) * per.unsqueeze(1)).reshape(N, n * n_rl)
    return ge, b


def warp_inputs(n, n_rl, N, t_kind="interior", seed=6100):
    """(est at the minimum width, pts, t) fp32, computed per call from the procedural hash (cheap).  t_kind: interior (0, 1) |
    zero | one | outside (in (-0.5, 0) or (1, 1.5)); est[:, 0] spans +-4, everything else +-1."""
    S = est_min_width(n, n_rl)
    sd = seed + 97 * n + 13 * n_rl + N
    est = uniform((N, S), sd, 1.0)
    est[:, 0] *= 4.0
    pts = uniform((N, 3), sd + 1, 2.0)
    u01 = uniform((N,), sd + 2, 0.5) + 0.5
    if t_kind == "interior":
        t = u01.clamp(2.0 ** -10, 1 - 2.0 ** -10)
    elif t_kind == "zero":
        t = torch.zeros(N)
    elif t_kind == "one":
        t = torch.ones(N)
    else:
        t = torch.where(u01 < 0.5, -u01, 1 + (u01 - 0.5)).clamp(-0.5, 1.5)
        assert bool(((t < 0) | (t > 1)).all())
    return est, pts, t


def pad_cols(est, pitch, seed=6200):
    """est [N, S] -> [N, pitch]: the unused trailing columns hold OTHER procedural values (a kernel that read them would show)"""
    N, S = est.shape
    assert pitch >= S
    if pitch == S:
        return est
    return torch.cat([est, uniform((N, pitch - S), seed + pitch + N, 3.0)], dim=1).contiguous()


WARP_PITCHES = (None, 31, 32, 33, 62, 63, 64, 65, 255)      # None: the minimum width
WARP_ROWS = (1, 63, 64, 65, 255, 256, 257, 1000)


def warp_pitches(n, n_rl, extra=()):
    S = est_min_width(n, n_rl)
    return sorted({S} | {p for p in WARP_PITCHES + tuple(extra) if p is not None and p >= S})


# ------------------------------------------------------------------------------------------------------------ FFJORD divergence
def ffjord_ref(est, tan, t, e, n):
    """e^T J e by torch.autograd.functional.jvp of est -> dp(est) * rig(est) along tan, dotted with e; -> (div [N], bound [N])"""
    N = est.shape[0]
    ed, tand, td, ee = est.double(), tan.double(), t.double().reshape(-1, 1), e.double().reshape(N, 3)
    zero3 = torch.zeros(N, 3, dtype=torch.float64)

    def rigid_dp(x):
        _, dp, rig, _, _ = warp_fp64(x, zero3, td, n)
        return dp * rig
    _, jv = torch.autograd.functional.jvp(rigid_dp, ed, tand)
    div = (jv * ee).sum(1)
    _, dp, rig, _, _ = warp_fp64(ed, zero3, td, n)
    dpm = curve_mag(ed[:, 1:1 + 3 * n], td, n, 3)
    ddpm = curve_mag(tand[:, 1:1 + 3 * n], td, n, 3)
    drig = (rig * (1 - rig) * 0.5 * tand[:, :1]).abs()
    T1 = (ee.abs() * ddpm * rig).sum(1)
    T2 = (ee.abs() * dpm * drig).sum(1)
    b = ((4 * n + 4) * U + sig_rel()) * (T1 + T2) + 4 * U * T2 + (ee.abs() * dpm).sum(1) * (0.5 * tand[:, 0].abs() * rig[:, 0] ** 2 * sig_rel()) + TINY
    return div, b


def ffjord_closed_form(est, tan, t, e, n):
    """the kernel's own formula in fp64: e . (ddp rig + dp drig)"""
    N = est.shape[0]
    ed, tand, td, ee = est.double(), tan.double(), t.double().reshape(-1, 1), e.double().reshape(N, 3)
    B = bernstein(td, n).unsqueeze(-1)
    dp = (B * ed[:, 1:1 + 3 * n].reshape(N, n, 3)).sum(1)
    ddp = (B * tand[:, 1:1 + 3 * n].reshape(N, n, 3)).sum(1)
    rig = torch.sigmoid(ed[:, :1] / 2)
    drig = rig * (1 - rig) * 0.5 * tand[:, :1]
    return (ee * (ddp * rig + dp * drig)).sum(1)


def ffjord_inputs(n, N, pitch, t_kind="interior", seed=6300):
    est, _, t = warp_inputs(n, 0, N, t_kind, seed)
    est = pad_cols(est, pitch)
    tan = uniform(est.shape, seed + 5 + n + N + pitch, 1.0)
    e = uniform((N, 3), seed + 6 + n + N, 1.0)
    return est, tan, t, e


# ------------------------------------------------------------------------------------------------------------ Laplace density
LAPLACE_BETAS = (1e-3, 0.05, 1.5)
LAPLACE_ROWS = (1, 3, 4, 5, 1023, 4099)


def laplace_inputs(N, beta, special=True, seed=6400):
    """sdf [N] fp32 in +-6 beta with (special, as far as N allows) +-0, |sdf| / beta beyond 88 and beyond 104, +-inf and a NaN in front"""
    sdf = uniform((N,), seed + N, 6.0) * float(beta)
    if special:
        vals = [0.0, -0.0, 95.0 * beta, -95.0 * beta, 110.0 * beta, -110.0 * beta, 87.5 * beta, float("inf"), float("-inf"), float("nan")]
        k = min(N, len(vals))
        sdf[:k] = torch.tensor(vals[:k], dtype=torch.float32)
    return sdf


def laplace_ref(sdf, beta):
    """-> (density fp64, bound); beta: the fp32 value as a python float"""
    s, bt = sdf.double(), float(beta)
    dens = O.laplace_cdf(-s, torch.tensor(bt, dtype=torch.float64)) / bt
    a = s.abs() / bt
    ex = torch.exp(-a)
    # the kernel squares exp(x / 2) where v_exp_f32 would flush (twice the error); which elements: ITS decision, restated in fp32 torch
    # operation by operation -- scaled = (-sdf) / beta, scaled * fp32(log2 e) < -126 (a correctly rounded division and product on both sides)
    scaled32 = (-sdf.float()) / torch.tensor(bt, dtype=torch.float32)
    deep = (scaled32 * torch.tensor(1.4426950408889634, dtype=torch.float32)) < -126.0
    assert scaled32.dtype == torch.float32
    rel = FAST_EXP_REL * (1 + deep.double()) + a * U
    pos = dens * (rel + 4 * U)
    neg = (ex / 2 * rel + U * (1 - ex / 2)) / bt + 2 * U * dens
    b = torch.where(s >= 0, pos, neg)
    b = torch.where(torch.isfinite(s), b, 2 * U * torch.nan_to_num(dens)) + DENORM * (1 / bt + 1)   # (+-inf: 0 or 1 / beta)
    return dens, b


def laplace_backward_ref(sdf, beta, g):
    """finite or infinite sdf -> (g_sdf, its bound, g_beta, its bound) by fp64 autograd; the g_beta bound needs finite inputs"""
    s = sdf.double().requires_grad_()
    bt = torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    dens = O.laplace_cdf(-s, bt) / bt
    gs, gb = torch.autograd.grad((dens * g.double()).sum(), (s, bt))
    s, bt = s.detach(), float(beta)
    a = s.abs() / bt
    fin = torch.isfinite(s)
    a_f = torch.where(fin, a, torch.zeros_like(a))
    gs_b = gs.abs() * (LIBM["exp"] + a_f * U + 6 * U) + DENORM * ((g.double().abs() + 0.5) / bt ** 2 + 1)
    ex = torch.exp(-a_f) / 2
    cdf = torch.where(s >= 0, ex, 1 - ex)
    term = g.double().abs() * (ex * torch.where(fin, s.abs(), torch.zeros_like(s)) / bt ** 3 + cdf / bt ** 2)
    P = (sdf.numel() + 255) // 256
    gb_b = float((term * (LIBM["exp"] + a_f * U + 10 * U)).sum() + (8 + P) * U * term.sum()) + DENORM
    return gs, gs_b, gb, gb_b


# ------------------------------------------------------------------------------------------------------------ tangent operators
ACT_ROWS = (1, 255, 257, 5000)
LEAKY_SLOPE = float(np.float32(0.01))


def act_inputs(n, seed=6500):
    """pre-activations in +-100 with the LeakyReLU kink exact: |x| < 0.1 is snapped to +0 / -0 alternately"""
    x = uniform((n,), seed + n, 100.0)
    small = x.abs() < 0.1
    x[small] = 0.0
    x[small & (torch.arange(n) % 2 == 1)] = -0.0
    clean_threshold(x, 0.0, 100.0)
    return x


def act_deriv_ref(x, act, order):
    """-> (fp64 reference, bound): sin by torch (cos, -sin), LeakyReLU (slope fp32(0.01), v > 0) and none piecewise: exact"""
    xd = x.double()
    if act == "sin":
        return (xd.cos(), torch.full_like(xd, LIBM["cos"])) if order == 1 else (-xd.sin(), torch.full_like(xd, LIBM["sin"]))
    if order == 2:
        return torch.zeros_like(xd), torch.zeros_like(xd)
    if act == "leaky_relu":
        clean_threshold(x, 0.0, 100.0)
        return torch.where(xd > 0, torch.ones_like(xd), torch.full_like(xd, LEAKY_SLOPE)), torch.zeros_like(xd)
    return torch.ones_like(xd), torch.zeros_like(xd)


def mul_bcast_ref(a, b):
    ref = a.double().unsqueeze(0) * b.double()
    return ref, U * ref.abs()


def mul_reduce_ref(g, b):
    prod = g.double() * b.double()
    return prod.sum(0), g.shape[0] * U * prod.abs().sum(0)


def eikonal_ref(nrm):
    """nrm [3, N] fp32 -> (loss fp64, bound)"""
    x = nrm.double()
    N = x.shape[1]
    ln = x.norm(dim=0)
    d = ln - 1
    loss = (d * d).mean()
    P = min((N + 255) // 256, 1024)
    return loss, float(((2 * d.abs() * (3 * ln + d.abs()) + d * d) * U).sum() / N + (11 + P) * U * loss)


def eikonal_backward_ref(nrm, g):
    x = nrm.double().requires_grad_()
    ln = x.norm(dim=0)
    (gx,) = torch.autograd.grad(((ln - 1) ** 2).mean() * float(g), x)
    x = x.detach()
    N = x.shape[1]
    ln, d = x.norm(dim=0), (x.norm(dim=0) - 1).abs()
    return gx, x.abs() * abs(float(g)) * 2 / N * ((3 * ln + d) / ln + 8 * d / ln) * U


# ------------------------------------------------------------------------------------------------------------ normalize3 / PosLinearView / light
def clean_threshold(v, thr, scale):
    """ASSERT that every element of v is exactly on the threshold or at least CLEAR * scale away from it"""
    dist = (v.double() - thr).abs()
    bad = torch.isfinite(v) & (dist != 0) & (dist < CLEAR * scale)
    assert not bool(bad.any()), f"{int(bad.sum())} inputs sit within {CLEAR * scale} of the threshold {thr}"


def normalize3_ref(v):
    """F.normalize(eps=1e-12) on the fp64 rows; the fp32 norm is ASSERTED exactly 0 or >= 1e-9 (clear of the 1e-12 clamp)"""
    q = v.double()
    n32 = (v * v).sum(-1).sqrt()
    fin = torch.isfinite(n32)
    assert bool((~fin | (n32 == 0) | (n32 >= 1e-9)).all()), "a row's norm sits near the 1e-12 clamp"
    nd = q.norm(dim=-1)
    assert bool((~fin | (nd < 1e-15) | (nd >= 1e-9)).all())
    ref = F.normalize(q, dim=-1, eps=1e-12)
    return ref, 5 * U * ref.abs()


def pos_linear_ref(lin, pos, C):
    """lin [N,1], pos [N,W >= C] -> ((sigmoid(lin) / 2 + 0.5) * pos[:, :C], bound)"""
    s = torch.sigmoid(lin.double())
    p = pos.double()[:, :C]
    ref = (s / 2 + 0.5) * p
    return ref, p.abs() * (0.5 * s * sig_rel() + U * (s / 2 + 0.5)) + U * ref.abs()


def pos_linear_backward_ref(lin, pos, g, C):
    """-> (g_lin [N,1], bound, g_pos [N,W], bound) by fp64 autograd"""
    l = lin.double().requires_grad_()
    p = pos.double().requires_grad_()
    out = (torch.sigmoid(l) / 2 + 0.5) * p[:, :C]
    gl, gp = torch.autograd.grad((out * g.double()).sum(), (l, p))
    s = torch.sigmoid(lin.double())
    gd, pd = g.double().abs(), pos.double()[:, :C].abs()
    gp_b = torch.zeros_like(gp)
    gp_b[:, :C] = gd * (0.5 * s * sig_rel() + U * (s / 2 + 0.5)) + U * gp[:, :C].abs()
    m = (gd * pd).sum(1, keepdim=True)
    gl_b = (C + 5) * U * m * s * (1 - s) / 2 + m * 0.5 * s * sig_rel() + TINY
    return gl, gl_b, gp, gp_b


def point_light_ref(x, center, intensity, decay):
    """O.point_light on the fp64 inputs (one light [3] or one per point [N,3]); the fp32 distance is ASSERTED 0 or >= 1e-3"""
    d32 = (center - x).norm(dim=-1)
    clean_threshold(d32, 0.0, 1.0)
    d, dist, spec = O.point_light(x.double(), center.double(), intensity.double(), decay)
    spec = spec if decay else intensity.double().expand_as(x.double())
    return (d, 6 * U * d.abs()), (dist, 4 * U * dist.abs()), (spec, (12 if decay else 0) * U * torch.nan_to_num(spec.abs(), posinf=0.0))


NORMALIZE_ROWS = (1, 8, 257, 5000)
LIGHT_ROWS = (1, 257, 3000)


def normalize3_nan_rows():
    """normalize3_rows(257) with a NaN in the middle of one row and in front of another"""
    v = normalize3_rows(257)
    v[7] = torch.tensor([1.0, float("nan"), 2.0])
    v[200] = torch.tensor([float("nan"), 0.0, 0.0])
    return v


def light_nan_inputs():
    """light_inputs(257) with one NaN coordinate in row 9"""
    x, c, i = light_inputs(257)
    x[9, 1] = float("nan")
    return x, c, i


def normalize3_rows(N):
    """rows for normalize3: procedural, then zero rows, rows of 1e-25 (their squares underflow) and one row with a NaN"""
    v = uniform((N, 3), 7100 + N, 2.0)
    v[v.norm(dim=-1) < 1e-3] = 0.0
    if N >= 8:
        v[1], v[5] = 0.0, 0.0
        v[2], v[6] = 1e-25, torch.tensor([1e-25, -1e-25, 0.0])
    return v


def light_inputs(N, per_point=False):
    """(x, centre, intensity): one light or one per point; row 3 sits ON its light"""
    x = uniform((N, 3), 7200 + N, 2.0)
    c = uniform((N, 3) if per_point else (3,), 7201 + N, 2.0)
    i = uniform((N, 3) if per_point else (3,), 7202 + N, 0.5) + 1.0
    if N > 3:
        x[3] = c[3] if per_point else c
    near = ((c - x).norm(dim=-1) < 1e-3) & ((c - x).norm(dim=-1) > 0)
    x[near] += 0.5
    return x, c, i


# ------------------------------------------------------------------------------------------------------------ marching
def f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def sphere_step(sdf, eps, far, dist, hits, rem):
    """src/march.py:39-45 for fp32 sdf / dist [R] and bool hits / rem [R]: only the rows with rem are updated -> (dist, hits, rem)"""
    assert sdf.dtype == dist.dtype == torch.float32 and hits.dtype == rem.dtype == torch.bool
    eps, far = f32(eps), f32(far)
    hits2 = torch.where(rem, hits | ((sdf < eps) & (dist <= far)), hits)
    dist2 = torch.where(rem, dist + sdf, dist)
    rem2 = rem & ~(hits2 | (dist2 > far))
    return dist2, hits2, rem2


def sign_change_step(sd, step, curr_min, idxs, last_pos, first_neg):
    """src/march.py:96-103 (step = the reference's i) -> (curr_min, idxs, last_pos, first_neg); NaN as torch.minimum has it"""
    assert sd.dtype == curr_min.dtype == torch.float32
    idxs2 = torch.where(sd < curr_min, torch.full_like(idxs, step + 1), idxs)
    cm2 = torch.minimum(curr_min, sd)
    mask = (first_neg == -1) & (sd < 0)
    return cm2, idxs2, torch.where(mask, torch.full_like(last_pos, step), last_pos), torch.where(mask, torch.full_like(first_neg, step + 1), first_neg)


def _bisect_todo(low, high, sl, sh, eps):
    return ((high - low) > f32(eps)) & (sl > 0) & (sh < 0) & (high > low)


def bisection_init(low, high, sl, sh, eps):
    """src/march.py:162-163 -> (z, todo)"""
    assert low.dtype == torch.float32
    return (low + high) / 2, _bisect_todo(low, high, sl, sh, eps)


def bisection_step(sm, eps, low, high, sl, sh, z, todo):
    """src/march.py:166-179 -> (low, high, sdf_low, sdf_high, z, todo)"""
    lm, hm = (sm > 0) & todo, (sm < 0) & todo
    low, sl = torch.where(lm, z, low), torch.where(lm, sm, sl)
    high, sh = torch.where(hm, z, high), torch.where(hm, sm, sh)
    return low, high, sl, sh, (low + high) / 2, todo & _bisect_todo(low, high, sl, sh, eps)


def analytic_sdf(p):
    """the two-sphere SDF of tests/golden/g15_march.npz"""
    a = torch.linalg.norm(p - torch.tensor([0.1, -0.2, 0.0]), dim=-1) - 1.1
    b = torch.linalg.norm(p - torch.tensor([0.9, 0.6, 0.3]), dim=-1) - 0.5
    return torch.minimum(a, b)


MARCH_ROWS = (1, 255, 256, 257, 4099)
EPS, FAR = 1e-3, 4.0


def _cycle(vals, R, dtype=torch.float32):
    v = torch.tensor(vals, dtype=dtype)
    return v.repeat((R + len(vals) - 1) // len(vals))[:R].clone()


def _off_threshold(R, seed, amp, thr_list, scale):
    """procedural values with everything closer than CLEAR * scale to a threshold moved ONTO it"""
    v = uniform((R,), seed + R, amp)
    for thr in thr_list:
        near = (v.double() - thr).abs() < CLEAR * scale
        v[near] = float(np.float32(thr))
    return v


def sphere_states(R, seed=6600):
    """chosen states in front, procedural ones behind: (sdf, dist, hits, rem), eps = EPS, far = FAR"""
    eps32, far32 = float(np.float32(EPS)), float(np.float32(FAR))
    above = float(np.nextafter(np.float32(FAR), np.float32(np.inf)))
    nan, inf = float("nan"), float("inf")
    # rows: sdf == eps | below eps | dist == far, hit | dist == far, no hit | one ulp above far | four rows with rem == 0 | inf | NaN |
    #       negative at dist == far | dist + sdf == far exactly: not stopped
    sdf = [eps32, 0.5 * eps32, 0.5 * eps32, 0.5, above - 3.0, nan, inf, -inf, 0.25, inf, nan, -1.0, 1.0]
    dist = [1.0, 1.0, far32, far32, 3.0, 1.0, 2.0, 3.0, 5.0, 1.0, 1.0, far32, 3.0]
    hits = [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    rem = [1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1]
    k = len(sdf)
    s = _off_threshold(R, seed, 1.0, (EPS,), EPS)
    d = uniform((R,), seed + 1 + R, 2.5) + 2.5            # [0, 5)
    tot = (d + s).double()
    s[(tot - FAR).abs() < CLEAR * FAR] = 0.5               # keeps dist + sdf clear of far
    d[(d.double() - FAR).abs() < CLEAR * FAR] = far32
    h = uniform((R,), seed + 2 + R, 1.0) > 0.8
    r = uniform((R,), seed + 3 + R, 1.0) > -0.5
    clean_sphere(s, d)
    m = min(k, R)
    s[:m], d[:m] = torch.tensor(sdf[:m]), torch.tensor(dist[:m])
    h[:m], r[:m] = torch.tensor(hits[:m], dtype=torch.bool), torch.tensor(rem[:m], dtype=torch.bool)
    return s, d, h, r


def clean_sphere(sdf, dist):
    """the procedural rows: sdf on eps or clear of it, dist and dist + sdf (in fp32) on far or clear of it.  (The chosen rows in front
    are on the thresholds on purpose, one of them ONE ULP above far: `dist + sdf just above far stops the ray`.)"""
    clean_threshold(sdf, float(np.float32(EPS)), EPS)
    clean_threshold(dist, float(np.float32(FAR)), FAR)
    clean_threshold(dist + sdf, float(np.float32(FAR)), FAR)


def sign_states(R, seed=6700):
    """(sd, curr_min, idxs, last_pos, first_neg): ties, +-0, an already written first_neg, NaN on either side"""
    nan = float("nan")
    sd = [0.25, 0.25, 0.0, -0.0, -0.5, -0.5, nan, 0.5, nan, -0.125, 0.75]
    cm = [0.25, 0.5, 0.5, 0.5, 0.5, -0.75, 0.5, nan, nan, -0.125, 0.5]
    fn = [-1, -1, -1, -1, -1, 3, -1, -1, -1, 3, 5]
    s = _off_threshold(R, seed, 1.0, (0.0,), 1.0)
    c = uniform((R,), seed + 1 + R, 1.0)
    c[::7] = s[::7]                                           # ties
    first = torch.where(uniform((R,), seed + 2 + R, 1.0) > 0, torch.full((R,), -1), torch.full((R,), 2)).int()
    last = torch.where(first == -1, first, first - 1).int()
    idxs = torch.where(uniform((R,), seed + 3 + R, 1.0) > 0, torch.zeros(R), torch.full((R,), 4.0)).int()
    m = min(len(sd), R)
    s[:m], c[:m] = torch.tensor(sd[:m]), torch.tensor(cm[:m])
    first[:m] = torch.tensor(fn[:m], dtype=torch.int32)
    last[:m] = torch.where(first[:m] == -1, first[:m], first[:m] - 1)
    clean_threshold(s, 0.0, 1.0)
    d = (s.double() - c.double()).abs()
    assert bool((~torch.isfinite(d) | (d == 0) | (d >= 1e-6)).all())
    return s, c, idxs, last, first


def bisect_states(R, seed=6800):
    """(low, high, sdf_low, sdf_high, sdf_mid), eps = BISECT_EPS: high == low, high - low == eps, brackets of the wrong sign, sdf_mid == +-0"""
    e = float(np.float32(BISECT_EPS))
    lo = [1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0, 2.0]
    hi = [1.0, 2.0, e, 2 * e, 2.0, 2.0, 2.0, 2.0, 1.0]
    sl = [0.5, 0.5, 0.5, 0.5, -0.5, 0.5, 0.0, 0.5, 0.5]
    sh = [-0.5, -0.5, -0.5, -0.5, -0.5, 0.5, -0.5, -0.0, -0.5]
    sm = [0.25, 0.0, 0.25, -0.25, 0.25, -0.25, 0.25, 0.25, 0.25]
    low = uniform((R,), seed + R, 1.0) + 1.0                   # [0, 2)
    width = _off_threshold(R, seed + 1, 1.0, (0.0, BISECT_EPS, -BISECT_EPS), BISECT_EPS).abs()
    width[::9] = 0.0
    high = low + width
    high = torch.where(((high - low).double() - e).abs() < CLEAR * e, low, high)   # the fp32 difference is 0 or clear of eps
    clean_threshold(high - low, e, e)
    slo = _off_threshold(R, seed + 2, 1.0, (0.0,), 1.0)
    shi = _off_threshold(R, seed + 3, 1.0, (0.0,), 1.0)
    smid = _off_threshold(R, seed + 4, 1.0, (0.0,), 1.0)
    smid[::5] = 0.0
    smid[1::10] = -0.0
    m = min(len(lo), R)
    low[:m], high[:m], slo[:m], shi[:m], smid[:m] = (torch.tensor(v[:m]) for v in (lo, hi, sl, sh, sm))
    return low, high, slo, shi, smid


BISECT_EPS = 2.0 ** -10     # a power of two: 0 + eps and 0 + 2 eps are exact, `high - low == eps` can be hit on the nose


def live_mask(R, seed=6900):
    return (uniform((R,), seed + R, 1.0) > 0.2).to(torch.uint8)
