"""Plain fp64 restatement of SSIM and MS-SSIM (csrc/ssim.hip; Wang et al. with the choices of pytorch_msssim, which the reference calls in
src/utils.py:186-195 and which is not installed anywhere this project is built, so no fixture of the reference exists: THIS MODULE IS THE PIN),
the error bounds the tests hold the kernels to, the mutants the bounds must tell apart, and the inputs the tests share.  Imported by
tests/test_ssim_ref.py (CPU) and tests/test_gpu_ssim.py.

DEFINITION.  Images are channel-last [N,H,W,C] in [0, data_range].  G: 11 taps exp(-(i - 5)^2 / (2 1.5^2)), normalised in fp64, ROUNDED ONCE TO
FP32 (the table the kernel holds; the restatement filters with those same values), applied as two grouped F.conv2d without padding.  Per pixel
of the (H-10) x (W-10) map: mu1 = G*x, mu2 = G*y, s1 = G*(x x) - mu1^2, s2 = G*(y y) - mu2^2, s12 = G*(x y) - mu1 mu2, C1 = (0.01 L)^2,
C2 = (0.03 L)^2, cs = (2 s12 + C2) / (s1 + s2 + C2), ssim = (2 mu1 mu2 + C1) / (mu1^2 + mu2^2 + C1) cs.  `ssim_ref` returns the means of ssim
and cs per (n, c).  MS-SSIM: five scales, between them F.avg_pool2d(kernel 2, padding (H % 2, W % 2)) (count_include_pad: every output / 4),
relu(cs) of scales 0 .. 3 and relu(ssim) of scale 4, prod v_i ** w_i with w = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333); min(H, W) > 160.
The gradient of the ssim means w.r.t. x is autograd's on this restatement; `ssim_grad_terms` restates the closed form the kernel uses
(tests/test_ssim_ref.py holds the two together).

THE BOUNDS (derived, not tuned; first order in u = 2^-24; every quantity on the right is the fp64 reference's, per pixel).
  means      mu = G*x is two passes of eleven taps, each tap a product and (but the first) an addition:  d(mu) = 22 u G*|x|.
  variances  the kernel sums the window about the pixel's OWN means, c11 = sum g g (x - mu1)^2, and adds the defect of the table
             (the 121 products of the fp32 taps sum to 1 - 2.8e-9) times mu1^2, which makes it s1 exactly; an error of mu1 enters squared, i.e. not at first
             order.  Every addend is >= 0, so the roundings -- the difference (twice), the square, two tap products, 10 + 10 additions,
             the defect's addition -- are relative:  d(s1) = 26 u s1,  d(s2) alike,  d(s12) = 26 u sqrt(s1 s2)  (Cauchy-Schwarz over the
             window for sum g g |x - mu1| |y - mu2|, which also covers |s12|).  This is what "the cancellation in s = G*(xx) - mu^2, divided
             by the pixel's own denominators" comes to: the uncentred form would carry 24 u G*(x x) instead, 4e-7 against a denominator of
             1e-3 in a smooth region, which no mutant below could be told from.
  ratios     N2 = 2 s12 + C2:  d(N2) = 2 d(s12) + u |N2| + u C2        (the doubling is exact; u C2: the constant's own rounding)
             B2 = (s1 + s2) + C2:  d(B2) = d(s1) + d(s2) + u (s1 + s2) + u B2 + u C2
             cs = N2 / B2:  d(cs) = d(N2) / B2 + |cs| d(B2) / B2 + u |cs|
             mu1^2:  2 |mu1| d(mu1) + u mu1^2;   mu1 mu2:  |mu1| d(mu2) + |mu2| d(mu1) + u |mu1 mu2|
             A1, B1 and l = A1 / B1 as N2, B2, cs with C1;   ssim = l cs:  d(S) = |cs| d(l) + |l| d(cs) + u |S|
  tile sum   a 16 x 16 tile: six levels of the wave's tree and three additions of the four waves, each rounding at most u times the sum of
             the magnitudes: 9 u mean|v|.  The tiles are added in double and the quotient is rounded once:  + u |mean|.
                 |got - ref| <= mean(d(v)) + 9 u mean|v| + u |mean v|                                       v = ssim or cs
  gradient   P = B1 B2:  d(P) = B2 d(B1) + B1 d(B2) + u P;   d1 = -S / B2:  d(S) / B2 + |d1| d(B2) / B2 + u |d1|
             d12 = 2 A1 / P:  2 d(A1) / P + |d12| d(P) / P + u |d12|
             ta = 2 mu2 N2 / P:  2 (|N2| d(mu2) + |mu2| d(N2)) / P + |ta| d(P) / P + 2 u |ta|;   tb = 2 mu1 S / B1 alike
             dm = ((ta - tb) - 2 mu1 d1) - mu2 d12:  the parts' errors + u for each of the two products and three differences, on the
             magnitudes of their operands.  G^T is two passes again: 22 u G^T|D| + G^T[d(D)] per map, and
             g_x = ((T_dm + 2 x T_d1) + y T_d12) s adds u per product and 2 u (|T_dm| + 2 |x T_d1| + |y T_d12|) for the two sums, then
             2 u |g_x| for s = fl(g / count) and the last product.
  halve      ((a + b) + c) + d, times 0.25 (exact): three additions, 3 u (|a| + |b| + |c| + |d|) / 4.
  ms-ssim    scale i >= 1 sees images that carry the halvings' error E_i = pool(E_{i-1}) + 3 u pool(|X_{i-1}|); it moves v_i by at most
             sum |d v_i / d X_i| E_i over both images (autograd on the restatement).  The combination is fp32 torch: the weight's
             rounding moves v ** w by w |ln v| u, powf is good to 4 u, the product of five to 4 u:
                 |got - ref| <= ref (sum_i [w_i d(v_i) / v_i + w_i |ln v_i| u + 4 u] + 4 u);   a v_i <= 0 makes the result exactly 0.
An entry whose bound is 0 must be exact.

THE DISCRIMINATION CONDITION (tests/test_ssim_ref.py): on the inputs the GPU tests use, every mutant -- sigma 1.0, a 9-tap window, pooling
without the odd-side padding, no relu, C1 and C2 swapped -- moves the value by at least 10 x the bound.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.procedural import proc_uniform

U = 2.0 ** -24
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
C_MEAN = 22.0     # two passes of (1 product + 10 additions)
C_VAR = 26.0      # 2 (difference) + 1 (square) + 2 (tap products) + 20 (additions) + 1 (the defect's addition)
C_TILE = 9.0      # 6 levels of the wave tree + 3 additions of the waves
C_POW = 4.0


def window(taps=11, sigma=1.5):
    """the normalised Gaussian, formed in fp64, rounded once to fp32, returned as fp64"""
    c = torch.arange(taps, dtype=torch.float64) - taps // 2
    g = torch.exp(-c ** 2 / (2 * sigma ** 2))
    return (g / g.sum()).float().double()


def _nchw(x):
    assert x.dim() == 4 and not x.is_cuda
    return x.double().permute(0, 3, 1, 2)


def gfilter(x, g, full=False):
    """x [N,C,h,w] fp64 -> G*x as two grouped F.conv2d, "valid" (full: the transposed filter, zero padding of taps - 1)"""
    C, k = x.shape[1], g.numel()
    p = k - 1 if full else 0
    x = F.conv2d(x, g.reshape(1, 1, k, 1).expand(C, 1, k, 1), padding=(p, 0), groups=C)
    return F.conv2d(x, g.reshape(1, 1, 1, k).expand(C, 1, 1, k), padding=(0, p), groups=C)


def ssim_terms(x, y, L=1.0, taps=11, sigma=1.5, swap=False):
    """x, y [N,C,H,W] fp64 -> dict of the per-pixel maps [N,C,H-10,W-10] (differentiable)"""
    g = window(taps, sigma)
    C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    if swap:
        C1, C2 = C2, C1
    mu1, mu2 = gfilter(x, g), gfilter(y, g)
    s1, s2, s12 = gfilter(x * x, g) - mu1 * mu1, gfilter(y * y, g) - mu2 * mu2, gfilter(x * y, g) - mu1 * mu2
    N2, B2 = 2 * s12 + C2, s1 + s2 + C2
    A1, B1 = 2 * mu1 * mu2 + C1, mu1 * mu1 + mu2 * mu2 + C1
    cs = N2 / B2
    return dict(g=g, C1=C1, C2=C2, mu1=mu1, mu2=mu2, s1=s1, s2=s2, s12=s12, N2=N2, B2=B2, A1=A1, B1=B1, cs=cs, l=A1 / B1, S=A1 / B1 * cs)


def ssim_ref(x, y, L=1.0, **mutant):
    """channel-last x, y [N,H,W,C] -> (ssim [N,C], cs [N,C]) fp64"""
    t = ssim_terms(_nchw(x), _nchw(y), L, **mutant)
    return t["S"].mean(dim=(2, 3)), t["cs"].mean(dim=(2, 3))


def pixel_bounds(x, y, t):
    """the module docstring's per-pixel bounds of every quantity the kernels form (x, y [N,C,H,W] fp64, t = ssim_terms): dict of maps"""
    g, C1, C2 = t["g"], t["C1"], t["C2"]
    a = lambda v: v.abs()
    mu1, mu2, B1, B2, N2, A1, S, cs, l = (t[k] for k in ("mu1", "mu2", "B1", "B2", "N2", "A1", "S", "cs", "l"))
    s1, s2 = t["s1"].clamp(min=0), t["s2"].clamp(min=0)
    d = {}
    d["mu1"], d["mu2"] = C_MEAN * U * gfilter(a(x), g), C_MEAN * U * gfilter(a(y), g)
    d["s1"], d["s2"], d["s12"] = C_VAR * U * s1, C_VAR * U * s2, C_VAR * U * (s1 * s2).sqrt()
    d["N2"] = 2 * d["s12"] + U * a(N2) + U * C2
    d["B2"] = d["s1"] + d["s2"] + U * (s1 + s2) + U * B2 + U * C2
    d["cs"] = d["N2"] / B2 + a(cs) * d["B2"] / B2 + U * a(cs)
    d["mu1sq"], d["mu2sq"] = 2 * a(mu1) * d["mu1"] + U * mu1 * mu1, 2 * a(mu2) * d["mu2"] + U * mu2 * mu2
    d["mu12"] = a(mu1) * d["mu2"] + a(mu2) * d["mu1"] + U * a(mu1 * mu2)
    d["A1"] = 2 * d["mu12"] + U * a(A1) + U * C1
    d["B1"] = d["mu1sq"] + d["mu2sq"] + U * (mu1 * mu1 + mu2 * mu2) + U * B1 + U * C1
    d["l"] = d["A1"] / B1 + a(l) * d["B1"] / B1 + U * a(l)
    d["S"] = a(cs) * d["l"] + a(l) * d["cs"] + U * a(S)
    return d


def mean_bound(v, dv):
    """bound of the mean over the map of v [N,C,h,w] whose per-pixel bound is dv"""
    return dv.mean(dim=(2, 3)) + C_TILE * U * v.abs().mean(dim=(2, 3)) + U * v.mean(dim=(2, 3)).abs()


def ssim_bounds(x, y, L=1.0):
    """channel-last x, y -> (bound of ssim [N,C], bound of cs [N,C])"""
    xc, yc = _nchw(x), _nchw(y)
    t = ssim_terms(xc, yc, L)
    d = pixel_bounds(xc, yc, t)
    return mean_bound(t["S"], d["S"]), mean_bound(t["cs"], d["cs"])


def ssim_grad_ref(x, y, gup, L=1.0):
    """autograd's gradient of sum gup[n,c] ssim[n,c] w.r.t. x, channel-last [N,H,W,C] fp64"""
    with torch.enable_grad():
        xc = _nchw(x).clone().requires_grad_(True)
        S = ssim_terms(xc, _nchw(y), L)["S"].mean(dim=(2, 3))
        (gx,) = torch.autograd.grad((S * gup.double()).sum(), xc)
    return gx.permute(0, 2, 3, 1).contiguous()


def ssim_grad_terms(x, y, gup, L=1.0):
    """the closed form the kernel evaluates and its bound: channel-last x, y, gup [N,C] -> (g_x, bound) [N,H,W,C] fp64"""
    xc, yc = _nchw(x), _nchw(y)
    t = ssim_terms(xc, yc, L)
    d = pixel_bounds(xc, yc, t)
    g = t["g"]
    a = lambda v: v.abs()
    mu1, mu2, B1, B2, N2, A1, S = (t[k] for k in ("mu1", "mu2", "B1", "B2", "N2", "A1", "S"))
    P = B1 * B2
    dP = B2 * d["B1"] + B1 * d["B2"] + U * P
    d1 = -S / B2
    dd1 = d["S"] / B2 + a(d1) * d["B2"] / B2 + U * a(d1)
    d12 = 2 * A1 / P
    dd12 = 2 * d["A1"] / P + a(d12) * dP / P + U * a(d12)
    ta, tb = 2 * mu2 * N2 / P, 2 * mu1 * S / B1
    dta = 2 * (a(N2) * d["mu2"] + a(mu2) * d["N2"]) / P + a(ta) * dP / P + 2 * U * a(ta)
    dtb = 2 * (a(S) * d["mu1"] + a(mu1) * d["S"]) / B1 + a(tb) * d["B1"] / B1 + 2 * U * a(tb)
    p1, p2 = 2 * mu1 * d1, mu2 * d12
    dm = ((ta - tb) - p1) - p2
    ddm = (dta + dtb + 2 * (a(mu1) * dd1 + a(d1) * d["mu1"]) + a(mu2) * dd12 + a(d12) * d["mu2"]
           + U * (a(p1) + a(p2)) + U * (a(ta) + a(tb)) + U * (a(ta - tb) + a(p1)) + U * (a(ta - tb - p1) + a(p2)))
    T = lambda v: gfilter(v, g, full=True)
    t_dm, t_d1, t_d12 = T(dm), T(d1), T(d12)
    g0 = t_dm + 2 * xc * t_d1 + yc * t_d12
    m1, m12 = a(2 * xc * t_d1), a(yc * t_d12)
    dg0 = ((T(ddm) + C_MEAN * U * T(a(dm))) + 2 * a(xc) * (T(dd1) + C_MEAN * U * T(a(d1))) + a(yc) * (T(dd12) + C_MEAN * U * T(a(d12)))
           + U * m1 + U * m12 + 2 * U * (a(t_dm) + m1 + m12))
    count = float(S.shape[2] * S.shape[3])
    s = (gup.double() / count)[:, :, None, None]
    gx = g0 * s
    bound = a(s) * dg0 + 2 * U * a(gx)
    return gx.permute(0, 2, 3, 1).contiguous(), bound.permute(0, 2, 3, 1).contiguous()


def halve_ref(x, pad=True):
    """channel-last [N,H,W,C] -> F.avg_pool2d(kernel 2, padding (H % 2, W % 2)) in fp64, channel-last (pad=False: the mutant)"""
    xc = _nchw(x)
    p = [s % 2 for s in xc.shape[2:]] if pad else [0, 0]
    return F.avg_pool2d(xc, kernel_size=2, padding=p).permute(0, 2, 3, 1).contiguous()


def halve_bound(x):
    """3 u (|a| + |b| + |c| + |d|) / 4 per output"""
    return 3 * U * halve_ref(x.abs())


def ms_ssim_values(x, y, L=1.0, pad=True, **mutant):
    """the [5,N,C] values under the relu: cs of scales 0 .. 3, ssim of scale 4"""
    if min(x.shape[1], x.shape[2]) <= 160:
        raise ValueError("image size should be larger than 160 due to the 4 downsamplings in ms-ssim")
    vals = []
    for i in range(5):
        s, cs = ssim_ref(x, y, L, **mutant)
        vals.append(cs if i < 4 else s)
        if i < 4:
            x, y = halve_ref(x, pad), halve_ref(y, pad)
    return torch.stack(vals)


def combine_ref(vals, relu=True):
    """[5,N,C] -> prod relu(v_i) ** w_i (relu=False: the mutant, NaN for a negative v)"""
    w = torch.tensor(WEIGHTS, dtype=torch.float64)[:, None, None]
    v = vals.double()
    return torch.prod((torch.relu(v) if relu else v) ** w, dim=0)


def ms_ssim_ref(x, y, L=1.0, pad=True, relu=True, **mutant):
    return combine_ref(ms_ssim_values(x, y, L, pad, **mutant), relu)


def ms_ssim_bound(x, y, L=1.0):
    """(reference [N,C], bound [N,C]) of ops.ms_ssim: the kernels' bounds per scale, the halvings' error carried through each scale's
    own gradient, the fp32 combination"""
    X, Y = x.double(), y.double()
    Ex, Ey = torch.zeros_like(X), torch.zeros_like(Y)
    vals, dvals = [], []
    for i in range(5):
        with torch.enable_grad():
            xc, yc = _nchw(X).clone().requires_grad_(True), _nchw(Y).clone().requires_grad_(True)
            t = ssim_terms(xc, yc, L)
            key = "cs" if i < 4 else "S"
            v = t[key].mean(dim=(2, 3))
        with torch.no_grad():
            dv = mean_bound(t[key], pixel_bounds(xc, yc, t)[key])
        for n in range(v.shape[0]):          # |d v[n,c] / d image| E, per (n, c): the sums do not mix
            for c in range(v.shape[1]):
                with torch.enable_grad():
                    gx, gy = torch.autograd.grad(v[n, c], (xc, yc), retain_graph=True)
                dv[n, c] += float((gx.abs() * _nchw(Ex)).sum() + (gy.abs() * _nchw(Ey)).sum())
        vals.append(v.detach())
        dvals.append(dv)
        if i < 4:
            Ex, Ey = halve_ref(Ex) + halve_bound(X), halve_ref(Ey) + halve_bound(Y)
            X, Y = halve_ref(X), halve_ref(Y)
    vals, dvals = torch.stack(vals), torch.stack(dvals)
    ref = combine_ref(vals)
    w = torch.tensor(WEIGHTS, dtype=torch.float64)[:, None, None]
    pos = vals > 0
    safe = torch.where(pos, vals, torch.ones_like(vals))
    rel = (w * dvals / safe + w * safe.log().abs() * U + C_POW * U).sum(dim=0) + 4 * U
    return ref, torch.where(pos.all(dim=0), ref * rel, torch.zeros_like(ref))


def worst_ratio(got, ref, bound):
    """max over ALL entries of |got - ref| / bound (bound 0: the entry must be exact -- ratio 0 or inf); NaN where the two disagree about NaN"""
    got = got.detach().cpu().double().reshape(ref.shape)
    if bool((torch.isnan(got) != torch.isnan(ref)).any()):
        return float("nan")
    both = torch.isnan(got) & torch.isnan(ref)
    err = torch.where(both, torch.zeros_like(ref), (got - ref).abs())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


# inputs ------------------------------------------------------------------------------------------------------
TILE = 16                                   # the kernel's tile: 16 x 16 pixels of the map (forward) or of the image (backward)
# (N, H, W, C): one map pixel; one row of three; exactly one forward tile; a tile plus one in each axis, ragged; N = 3; C = 1, 3, 4
SSIM_CASES = ((1, 11, 11, 1), (1, 11, 13, 3), (2, 26, 26, 3), (1, 27, 43, 4), (3, 18, 18, 3))
MS_CASES = ((1, 161, 161, 3), (1, 176, 163, 3))   # the smallest legal side (the last scale is one map pixel); even and odd halvings
# (177 x 179: the smallest odd sides at which pooling WITHOUT the padding still leaves an 11 x 11 last scale -- a value to compare)
CPU_MS_CASES = ((1, 176, 161, 3), (1, 163, 170, 3), (1, 177, 179, 3))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@functools.lru_cache(maxsize=None)
def image_pair(N, H, W, C, seed=6100):
    """(x, y) fp32 channel-last in [0, 1]: a smooth image plus noise, y = a second noise draw on the same image at another contrast, and a
    flat black corner (the top-left quarter of both: the constant region, where the uncentred variances cancel worst).  Callers must
    not modify them."""
    i = np.arange(H, dtype=np.float64)[None, :, None, None]
    j = np.arange(W, dtype=np.float64)[None, None, :, None]
    n = np.arange(N, dtype=np.float64)[:, None, None, None]
    c = np.arange(C, dtype=np.float64)[None, None, None, :]
    smooth = 0.5 + 0.3 * np.sin(0.11 * i + 0.7 * c + n) * np.cos(0.07 * j - 0.4 * n)
    k = seed + 7 * H + 3 * W + C + N
    x = smooth + proc_uniform((N, H, W, C), k, 0.15)
    y = 0.5 + 0.85 * (smooth - 0.5) + proc_uniform((N, H, W, C), k + 1, 0.15)
    x, y = np.clip(x, 0, 1), np.clip(y, 0, 1)
    x[:, :H // 4, :W // 4] = 0
    y[:, :H // 4, :W // 4] = 0
    return _t(x.astype(np.float32)), _t(y.astype(np.float32))


@functools.lru_cache(maxsize=None)
def noise_pair(N, H, W, C, seed=6200):
    """(x, 1 - x) on uniform noise: anticorrelated, every cs is negative and MS-SSIM is exactly 0 through the relu"""
    x = _t((proc_uniform((N, H, W, C), seed + H + W, 0.5).astype(np.float64) + 0.5).astype(np.float32)).clamp(0, 1)
    return x, 1 - x


@functools.lru_cache(maxsize=None)
def upstream(N, C, seed=6300):
    """the gradient tests' g [N,C] fp32, both signs"""
    return _t(proc_uniform((N, C), seed + N + C, 1.0))


@functools.lru_cache(maxsize=None)
def ssim_reference(case):
    """(ssim, cs, bound of ssim, bound of cs) of image_pair(*case), computed once per process and shared"""
    x, y = image_pair(*case)
    return ssim_ref(x, y) + ssim_bounds(x, y)


@functools.lru_cache(maxsize=None)
def grad_reference(case):
    """(autograd's g_x, bound) of image_pair(*case) under upstream(N, C)"""
    x, y = image_pair(*case)
    g = upstream(case[0], case[3])
    return ssim_grad_ref(x, y, g), ssim_grad_terms(x, y, g)[1]


@functools.lru_cache(maxsize=None)
def ms_reference(case):
    x, y = image_pair(*case)
    return ms_ssim_bound(x, y)


MUTANTS = {"sigma 1.0": dict(sigma=1.0), "9 taps": dict(taps=9), "no padding": dict(pad=False), "no relu": dict(relu=False),
           "C1 / C2 swapped": dict(swap=True)}
