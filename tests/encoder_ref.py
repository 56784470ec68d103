"""Plain fp64 references of the four encoders every model starts at -- the eight-level hash grid (src/neural_blocks.py:126-193 of the
reference), the Fourier / positional features (src/utils.py:14-17, src/neural_blocks.py:30-34), elevation / azimuth of the view direction
(src/utils.py:247-254) and the mip integrated positional encoding (src/utils.py:23-101) --, the per-element bounds the tests hold the
kernels to, the named edge inputs, and fp32 restatements of the kernels' own sine reductions (csrc/common.h) with their seeded mistakes.
Imported by tests/test_encoder_ref.py (CPU) and tests/test_gpu_encoders.py.  Everything is procedural; there are no golden files.

u = U = 2^-24 (half an ulp of 1: one fp32 rounding is u relative).  The library is built with -ffp-contract=off: every `*` and `+` of the
kernels is one rounding, every fmaf one.

HASH.  Contract domain: |x| 16 < 2^31 on every axis (N_0 = 16 is the largest resolution; the kernels convert floor(x N_l) to int32, the
reference to int64).  Beyond it nothing is asserted.  The reference takes v = fl32(x N_l), floor(v) and w = fl32(v - floor(v)) in fp32 -- one
rounding each, the same bits on the CPU and the GPU, and w is exact by Sterbenz wherever it does not round to 1 -- and evaluates the
trilinear sum, its position derivative N_l sum_c dW_c/dw_a <e_c, g> and the directional derivative in fp64 from those fp32 weights.
  forward    sum_c e_c W_c, W_c = u_x u_y u_z, u = w or fl(1 - w):  (1 - w) one rounding per factor (3), the weight product 2, e_c W_c 1, the
             eight-term sum 7:                                      K_HASH_FWD = 13,   bound = 13 u sum_c |e_c| |W_c| + 2^-126
  gradient   per level N_l sum_c d_c (s u u): d_c = <e_c, g> 4 products 3 sums = 4 roundings deep, (1 - w) 2, u u 1, d_c (.) 1, the sum
             over corners 8 (it starts from 0.f), N_l 1 = 17; the levels' xor tree 3, the input's and the lead copy's own gradient 2:
                                                                    K_HASH_GRAD = 22,  on sum_l N_l sum_c |d|_c |u u| + |g_in| + |g_lead|
  jvp        N_l e_a 1, (1 - w) 2, u u 1, s (u u) 1, the three-term sum 2, w e 1, the corner sum 8:          K_HASH_JVP = 16
  (first order in u; the second-order terms are below 2^-40 of the magnitude)

FOURIER.  The inputs are ARGUMENT-EXACT: x and basis dyadic so that every product and partial sum of m = x . (scale B) is exact in fp32 in
any order, fused or not (asserted at import: the fp32 and the fp64 evaluation of m agree bit for bit).  What is left is the sine itself.
  |m| <= 3e3   sincos_cw (three-term Cody-Waite by pi, degree-9 / degree-10 polynomials), restated here in numpy fp32 (fma = the fp64
               product and sum rounded once to fp32: a double rounding, which is what the factor 1.25 covers).  Its worst error against
               fp64 over the sets and 4 10^6 uniform arguments is measured by cw_worst(): 1.45e-7 (sin) and 5.81e-7 (cos) when this was
               written (the cosine's degree-10 polynomial truncates at (pi / 2)^12 / 12! = 4.7e-7).  The GPU bound is 1.25 x those.
  |m| >  3e3   libm's sinf / cosf: 4u absolute.
  positional   raw = fl32(x band) is ONE fp32 product, the same bits everywhere; fp64 sin / cos of that fp32 raw, 4u.
  bulk         random x and basis at sigma 16 / 32 against fp64 of the exact dot product: 2e-4 (the budget of the fp32 argument).

ELEVATION / AZIMUTH.  oracle.dir_to_elev_azim restated in fp64 with the clamp limit the kernels have, fl32(1 - fl32(1e-6)) = 1 - 17 u.
  elevation  4u (1 + 1 / sqrt(1 - z^2)) at the clamped z (the condition number of acos: 707 at the clamp);  azimuth 4u pi.
  The zero direction is compared bit for bit with the fp32 oracle: the signs of zero decide 0 against +-pi.

MIP.  ARGUMENT-EXACT crops: axis-aligned dyadic directions, dyadic origins and steps, so that t_mean and mean = d t_mean + o are exact in
fp32 for the cylinder (asserted at import) and y = 2^k mean is exact for every degree.  Reference: exp(-c 4^k / 2) sin(2^k m), the cosine
half as sin(fl32(y + fl32(pi / 2))) like the reference's fp32 forward; the covariance c from an fp64 evaluation of the moments.
  bound = 1.25 E damp + 0.37 K_c u (+ damp 2^k dm for the cone), E = the worst error of the restated mip_feature angle path (revolution
  count with a two-term 1 / 2 pi, sin_cw) against fp64, measured by mip_worst(): 3.8e-7.  x e^-x <= 0.37 turns the RELATIVE error K u of
  the exponent x = c 4^k / 2 into an absolute error of the damp.  K counted from mip_gaussian for axis-aligned directions (dsq / magn is
  exactly 0 or 1): rad = sqrt(sum of squares) 2 / fl32(sqrt 12): differences 1, squares 2 + 1, the sums 2, the root 2.5 + 1 = 3.5 (halved by
  the root, kept whole), the quotient and its constant 1.5 = 5; rad^2 2 x 5 + 1 = 11, / 4 exact; r_var (1 - .) 1, the sum 1: 13 (the
  t_var dsq path: 1 + 3 + 1 + 1 + 1 = 7 is shorter); the exponent's product and constant 2; exp2 (2u) and the closing product (u) are
  relative to damp <= 1 and enter as 3 / 0.37 -> 9:                                                       K_MIP_CYL = 24
  cone: r_var = rad^2 (mu^2 / 4 + 5 hw^2 / 12 - 4 hw^4 / (15 den)): the three terms carry 2, 3 and 8 roundings, the two sums 2, and the
  difference is at least 0.36 of the positive part (4 / 15 hw^4 / den <= 4 / 15 hw^2): 15 / 0.36 -> 42, rad^2 11, the product 1, as
  above 2 + 2 + 9:                                                                                        K_MIP_CONE = 67
  (t_var = hw / 3 - ...: the subtrahend is below 0.36 hw^4 / mu^2, a few percent of hw / 3 for the crops' mu >= 2: shorter again.)
  The cone's t_mean = mu + 2 mu hw^2 / den is not exact: dm = K_M u (|d t_mean| + |o|), K_M = 6 (the correction is below mu / 3 and
  carries 6 roundings: 2; the sum, the product with d and the sum with o: 3; one spare), amplified by 2^k in the angle.
"""
import functools
import math

import numpy as np
import torch

import oracle as O
from oracle.procedural import proc_param, proc_uniform

U = 2.0 ** -24
TINY = 2.0 ** -126
f32, f64 = np.float32, np.float64

K_HASH_FWD = 13
K_HASH_GRAD = 22
K_HASH_JVP = 16
K_MIP_CYL = 24
K_MIP_CONE = 67
K_MIP_MEAN = 6
LIBM = 4.0 * U           # sinf / cosf / the positional encoder
CW_MARGIN = 1.25         # the emulated fma's double rounding
BULK_TOL = 2e-4          # tests/test_gpu_ops.py::test_fourier_positional's budget for an fp32 argument
CW_SWITCH = 3.0e3        # fourier_sincos: |m| <= 3e3 takes sincos_cw


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements; a NaN / Inf anywhere in got or ref is +inf"""
    err = (torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(ref).double()).abs()
    r = err / torch.as_tensor(bound).double()
    return float("inf") if not bool(torch.isfinite(r).all()) else float(r.max()) if r.numel() else 0.0


def bits_equal(a, b):
    """bit for bit (torch.equal takes -0.0 == +0.0 and NaN != NaN)"""
    a, b = torch.as_tensor(a).detach().cpu().contiguous(), torch.as_tensor(b).detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32))


# =============================================================================================================== hash
RES32 = tuple(float(f32(r)) for r in O.hash_resolutions())
assert RES32[0] == 16.0 and max(RES32) == 16.0
HASH_COUNTS = (1, 7, 8, 9, 63, 64, 65, 257)
HASH_SETS = ("lattice", "below", "tiny_neg", "far", "bulk")


@functools.lru_cache(maxsize=None)
def hash_tables():
    """[8, 65536, 4] tables without a zero entry (a zero would hide a wrong weight and break the bit-for-bit lattice check)"""
    t = _t(proc_param("embs.weight", (8, 65536, 4), salt=11))
    assert bool((t != 0).all())
    return t


@functools.lru_cache(maxsize=None)
def hash_sets():
    a = (np.arange(-40, 41) / 16.0).astype(f32)                                   # N_0 = 16: level 0 sits on the lattice
    full = np.stack([a, np.roll(a, 13), np.roll(a, 29)], axis=1)                  # all three axes on the lattice
    parts = [full]
    for ax in range(3):                                                           # one axis on the lattice, the others anywhere
        r = proc_uniform((81, 3), 101 + ax, 3.0)
        r[:, ax] = a
        parts.append(r)
    z, nz = f32(0.0), f32(-0.0)
    parts.append(np.array([[z, z, z], [nz, nz, nz], [z, nz, z], [nz, z, nz]], dtype=f32))   # on the lattice of every level
    lattice = np.concatenate(parts).astype(f32)
    below = np.concatenate([np.nextafter(lattice, f32(-np.inf)), np.nextafter(lattice, f32(np.inf))]).astype(f32)
    tiny = []
    for ax in range(3):
        r = proc_uniform((6, 3), 111 + ax, 3.0)
        r[:, ax] = np.array([1e-30, -1e-30, 2.0 ** -126, -2.0 ** -126, 1e-8, -1e-8], dtype=f32)
        tiny.append(r)
    tiny_neg = np.concatenate(tiny).astype(f32)
    far = []
    for i, e in enumerate((10, 19, 20, 23, 26)):
        for s in (1.0, -1.0):
            b = f32(s * 2.0 ** e)
            low = np.abs(proc_uniform((4, 3), 121 + 2 * i + (s < 0), 0.99)) + f32(1.0)    # random low bits: |x| in [2^e, 2^(e+1))
            far.append(np.array([b, b, b], dtype=f32))
            far.append((b * low[0]).astype(f32) * np.array([1, -1, 1], dtype=f32))
            for ax in range(3):
                r = proc_uniform((3,), 131 + 6 * i + 3 * (s < 0) + ax, 3.0)
                r[ax] = b * low[1 + ax, ax]
                far.append(r)
    far = np.stack(far).astype(f32)
    bulk = proc_uniform((4096, 3), 141, 3.0)
    sets = dict(lattice=lattice, below=below, tiny_neg=tiny_neg, far=far, bulk=bulk)
    for v in sets.values():
        assert float(np.abs(v).max()) * 16.0 < 2.0 ** 31                          # the contract domain
    return {k: _t(v) for k, v in sets.items()}


@functools.lru_cache(maxsize=None)
def hash_concat():
    """the edge sets first, so that the short prefixes of HASH_COUNTS are made of edges"""
    s = hash_sets()
    return torch.cat([s["tiny_neg"], s["far"], s["lattice"], s["below"], s["bulk"]])


N_LATTICE_FULL = 81     # the first rows of `lattice` have all three axes on the level-0 lattice (so have its four zero rows at the end)

_BITS = [((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in range(8)]   # corner order of the reference: bit2 = x high, bit1 = y, bit0 = z


def hash_weights32(x, level):
    """(floor(v) as fp32, w) of one level exactly as the oracle and the kernels have them: three fp32 operations"""
    v = x * torch.tensor(RES32[level], dtype=torch.float32)
    fl = v.floor()
    return fl, v - fl


def hash_ref(x, tables):
    """x [N, 3] fp32 -> dict(idx [8, 8, N] int64, feat [N, 32], mag (sum |e| |W|), J [N, 32, 3] = d feat / d x, Jmag) in fp64"""
    N = x.shape[0]
    idx = O.hash_corner_indices(x)
    feat, mag = torch.zeros(N, 32, dtype=torch.float64), torch.zeros(N, 32, dtype=torch.float64)
    J, Jmag = torch.zeros(N, 32, 3, dtype=torch.float64), torch.zeros(N, 32, 3, dtype=torch.float64)
    for l in range(8):
        _, w = hash_weights32(x, l)
        w = w.double()
        iw = 1.0 - w
        e = tables[l][idx[l]].double()                                            # [8, N, 4]
        sl = slice(4 * l, 4 * l + 4)
        for c, bits in enumerate(_BITS):
            u = [w[:, a] if bits[a] else iw[:, a] for a in range(3)]
            W = u[0] * u[1] * u[2]
            feat[:, sl] += W[:, None] * e[c]
            mag[:, sl] += W.abs()[:, None] * e[c].abs()
            for a in range(3):
                o1, o2 = [b for b in range(3) if b != a]
                d = (1.0 if bits[a] else -1.0) * u[o1] * u[o2] * RES32[l]
                J[:, sl, a] += d[:, None] * e[c]
                Jmag[:, sl, a] += d.abs()[:, None] * e[c].abs()
    return dict(idx=idx, feat=feat, mag=mag, J=J, Jmag=Jmag)


def hash_fwd_bound(ref):
    return K_HASH_FWD * U * ref["mag"] + TINY


def hash_grad_ref(ref, g, g_in=None, g_lead=None):
    """g [N, 32] (feature columns) -> (g_x [N, 3], bound); g_in / g_lead [N, 3]: the raw copies' own gradient"""
    g = g.double()
    gx = (ref["J"] * g[:, :, None]).sum(1)
    mag = (ref["Jmag"] * g.abs()[:, :, None]).sum(1)
    for extra in (g_in, g_lead):
        if extra is not None:
            gx = gx + extra.double()
            mag = mag + extra.double().abs()
    return gx, K_HASH_GRAD * U * mag + TINY


def hash_jvp_ref(ref, tangent):
    """tangent [N, 3] -> (t [N, 32], bound)"""
    t = tangent.double()
    return (ref["J"] * t[:, None, :]).sum(2), K_HASH_JVP * U * (ref["Jmag"] * t.abs()[:, None, :]).sum(2) + TINY


def hash_fp32(x, tables, mistake=None):
    """the oracle's fp32 forward [N, 32] restated with one seeded mistake: 'trunc' (for floor), 'swap' (the weights' x and z bits
    exchanged against the indices' corner order), 'w64' (the fractional part taken from an fp64 v); None: the oracle itself"""
    out = []
    res = O.hash_resolutions()
    for l in range(8):
        v = x * res[l]
        fl = v.trunc() if mistake == "trunc" else v.floor()
        w = v - fl
        if mistake == "w64":
            v64 = x.double() * res[l]
            w = (v64 - v64.floor()).float()
        lo = fl.long()
        e = torch.stack([tables[l][(O.nerf_oracle._hash_fn(c) % 65536).squeeze(-1)] for c in O.nerf_oracle._corners(lo)], dim=0)
        iw = 1 - w
        acc = 0
        for c, bits in enumerate(_BITS):
            if mistake == "swap":
                bits = bits[::-1]
            W = (w[:, 0] if bits[0] else iw[:, 0]) * (w[:, 1] if bits[1] else iw[:, 1]) * (w[:, 2] if bits[2] else iw[:, 2])
            acc = acc + e[c] * W[:, None]
        out.append(acc)
    return torch.cat(out, dim=-1)


def hash_probe(N, seed, width=32):
    """an upstream gradient / a tangent"""
    return _t(proc_uniform((N, width), seed, 1.0))


# ============================================================================================ sincos_cw, restated in numpy fp32
def _fma(a, b, c):
    return (np.asarray(a, dtype=f64) * np.asarray(b, dtype=f64) + np.asarray(c, dtype=f64)).astype(f32)


def _cw_reduce(x, two_term=False):
    q = np.rint(x * f32(0.318309886183790672))
    r = _fma(q, f32(-3.140625), x)
    r = _fma(q, f32(-9.67502593994140625e-4), r)
    if not two_term:
        r = _fma(q, f32(-1.509957990978376432e-7), r)
    return q, r


def sincos_cw_emul(x, two_term=False, short_cos=False):
    """csrc/common.h sincos_cw, constant for constant; two_term: without the third reduction constant; short_cos: the cosine
    polynomial without its highest term"""
    x = np.asarray(x, dtype=f32)
    q, r = _cw_reduce(x, two_term)
    r2 = r * r
    p = _fma(r2, f32(2.5962193818e-06), f32(-1.9804804431e-04))
    p = _fma(p, r2, f32(8.3329907333e-03))
    p = _fma(p, r2, f32(-1.6666655917e-01))
    s = _fma(p * r2, r, r)
    c = np.full_like(r2, f32(2.4801587302e-05)) if short_cos else _fma(r2, f32(-2.7557319224e-07), f32(2.4801587302e-05))
    c = _fma(c, r2, f32(-1.3888888889e-03))
    c = _fma(c, r2, f32(4.1666666667e-02))
    c = _fma(c, r2, f32(-0.5))
    c = _fma(c, r2, f32(1.0))
    odd = (q.astype(np.int64) & 1).astype(bool)
    return np.where(odd, -s, s).astype(f32), np.where(odd, -c, c).astype(f32)


def sin_cw_emul(x):
    return sincos_cw_emul(x)[0]       # sin_cw is the sine half of sincos_cw, operation for operation


def fourier_sincos_emul(m, no_switch=False, **kw):
    """fourier_sincos: sincos_cw up to 3e3, libm (modelled as the correctly rounded value) beyond; no_switch: the polynomial everywhere"""
    m = np.asarray(m, dtype=f32)
    s, c = sincos_cw_emul(m, **kw)
    if no_switch:
        return s, c
    big = np.abs(m) > f32(CW_SWITCH)
    return np.where(big, np.sin(m.astype(f64)).astype(f32), s), np.where(big, np.cos(m.astype(f64)).astype(f32), c)


# ============================================================================================================ Fourier
F_VARIANTS = (128, 6, 1)
D_VARIANTS = (1, 2, 3)
SCALES = (1.0, 2.0, 0.5)
N_VARIANTS = (1, 31, 33, 257)


def _dyadic(shape, seed, amp, step):
    return (np.rint(proc_uniform(shape, seed, amp).astype(f64) / step) * step).astype(f32)


@functools.lru_cache(maxsize=None)
def fourier_sets():
    """name -> (x [N, 3], basis [3, 128]); a variant takes x[:N, :D], basis[:D, :F]"""
    P = (_dyadic((257, 3), 201, 4.0, 2.0 ** -6), _dyadic((3, 128), 202, 256.0, 2.0 ** -4))       # |m| <= 3072 on a 2^-10 grid
    L = (_dyadic((257, 3), 203, 128.0, 2.0 ** -2), _dyadic((3, 128), 204, 256.0, 2.0 ** -2))     # |m| up to 98304: the libm branch
    for x, b, top in ((P[0], P[1], 4.0), (L[0], L[1], 128.0)):       # the corners of the domain: m = +-3072, +-98304 in column 0
        x[0], x[1], b[:, 0] = top, -top, 256.0
    # E: explicit arguments.  x = (m, 0, 0), basis row 0 = +-1, +-1/2 (exact products), rows 1.. anything (times zero)
    k = np.arange(1, 1901)
    near = (k * (math.pi / 2)).astype(f32)                                                        # the fp32 neighbours of k pi / 2
    side = np.where(k % 2 == 0, np.nextafter(near, f32(-np.inf)), np.nextafter(near, f32(np.inf))).astype(f32)
    edge = np.array([3000 - 2.0 ** -10, 3000, 3000 + 2.0 ** -10, 3072], dtype=f32)
    m = np.concatenate([np.array([0.0], dtype=f32), edge, -edge, near, side]).astype(f32)
    xe = np.zeros((m.shape[0], 3), dtype=f32)
    xe[:, 0] = m
    be = _dyadic((3, 128), 205, 256.0, 2.0 ** -4)
    be[0] = np.tile(np.array([1.0, -1.0, 0.5, -0.5], dtype=f32), 32)
    return {n: (_t(x), _t(b)) for n, (x, b) in dict(P=P, L=L, E=(xe, be)).items()}


def fourier_m(x, basis, scale=1.0):
    """m = x . (scale basis) [N, F] in fp64, asserting that the fp32 evaluation in the kernels' order gives the same bits"""
    be = basis if scale == 1.0 else basis * torch.tensor(scale, dtype=torch.float32)
    m64 = x.double() @ be.double()
    m32 = x[:, :1] * be[:1]
    for d in range(1, x.shape[1]):
        m32 = (x[:, d:d + 1].double() * be[d:d + 1].double() + m32.double()).float()              # fmaf: one rounding
    assert torch.equal(m32.double(), m64), "the argument is not exact in fp32"
    return m64


for _n, (_x, _b) in fourier_sets().items():   # the module-level check: every variant's m is exact
    for _D in D_VARIANTS:
        for _s in SCALES:
            fourier_m(_x[:, :_D], _b[:_D], _s)


@functools.lru_cache(maxsize=None)
def cw_worst():
    """(worst |sin error|, worst |cos error|) of the restated sincos_cw against fp64 for |m| <= 3e3: the sets' arguments (all scales)
    and 4 10^6 uniform ones"""
    args = [proc_uniform((4_000_000,), 211, CW_SWITCH)]
    for x, b in fourier_sets().values():
        for s in SCALES:
            args.append(fourier_m(x, b, s).numpy().astype(f32).ravel())
    m = np.concatenate(args)
    m = m[np.abs(m) <= f32(CW_SWITCH)]
    s, c = sincos_cw_emul(m)
    m64 = m.astype(f64)
    return float(np.abs(s - np.sin(m64)).max()), float(np.abs(c - np.cos(m64)).max())


def fourier_ref(x, basis, scale=1.0):
    """-> (features [N, 2F] fp64, bound [N, 2F]) for argument-exact inputs"""
    m = fourier_m(x, basis, scale)
    ws, wc = cw_worst()
    small = m.abs() <= CW_SWITCH
    lib = torch.full_like(m, LIBM)
    return (torch.cat([m.sin(), m.cos()], dim=-1),
            torch.cat([torch.where(small, torch.full_like(m, CW_MARGIN * ws), lib), torch.where(small, torch.full_like(m, CW_MARGIN * wc), lib)], dim=-1))


def fourier_variant(name, N, D, F):
    x, b = fourier_sets()[name]
    return x[:N, :D].contiguous(), b[:D, :F].contiguous()


@functools.lru_cache(maxsize=None)
def fourier_bulk(sigma):
    """random x in [-1, 1)^3 and the reference's basis scale: (x, basis, fp64 features of the exact dot product)"""
    x = _t(proc_uniform((257, 3), 221 + sigma, 1.0))
    b = _t(proc_param("basis", (3, 128), salt=sigma)) * float(sigma)
    m = x.double() @ b.double()
    return x, b, torch.cat([m.sin(), m.cos()], dim=-1)


@functools.lru_cache(maxsize=None)
def positional_case(NB):
    """(x [257, 3], bands [NB], fp64 features of the fp32 raw); NB = 4: the 16-byte path, 5: the scalar path"""
    x = _t(proc_uniform((257, 3), 231 + NB, 3.0))
    bands = _t((2.0 ** np.arange(NB) * math.pi).astype(f32))
    raw = torch.tensordot(x, bands, dims=0).reshape(x.shape[0], -1).double()      # one fp32 product per element
    return x, bands, torch.cat([raw.sin(), raw.cos()], dim=-1)


# ================================================================================================ elevation / azimuth
LIM32 = float(f32(1.0) - f32(1e-6))
assert LIM32 == 1.0 - 17 * U
EPS32 = float(f32(1e-12))


@functools.lru_cache(maxsize=None)
def elaz_sets():
    def tilt(t, phi, s):
        return [math.sin(t) * math.cos(phi), math.sin(t) * math.sin(phi), s * math.cos(t)]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=f32)
    poles = np.array([tilt(t, phi, s) for t in (1e-7, 1e-4, 1e-3, 2e-3) for phi in (0.3, 2.0, -2.5) for s in (1.0, -1.0)], dtype=f32)
    z, nz = f32(0.0), f32(-0.0)
    seam = np.array([[-1, z, 0], [-1, nz, 0], [-1, z, 0.5], [-1, nz, 0.5], [-2, 1e-30, 0.3], [-2, -1e-30, 0.3], [-1, 1e-7, 0], [-1, -1e-7, 0],
                     [-0.25, z, -3], [-0.25, nz, -3]], dtype=f32)
    zero = np.array([[a, b, c] for a in (z, nz) for b in (z, nz) for c in (z, nz)], dtype=f32)
    unit = proc_uniform((9, 3), 301, 1.0)
    unit /= np.linalg.norm(unit, axis=1, keepdims=True)
    norms = (unit * np.repeat(np.array([1e-20, 1e-6, 1e18], dtype=f32), 3)[:, None]).astype(f32)
    bulk = proc_uniform((70, 3), 302, 1.3)
    return {k: _t(v) for k, v in dict(axes=axes, poles=poles, seam=seam, zero=zero, norms=norms, bulk=bulk).items()}


@functools.lru_cache(maxsize=None)
def elaz_dirs():
    """(dirs [R, 3], slice of the zero-direction rows)"""
    s = elaz_sets()
    names = list(s)
    start = sum(s[n].shape[0] for n in names[:names.index("zero")])
    return torch.cat([s[n] for n in names]), slice(start, start + s["zero"].shape[0])


def elaz_ref(d, keep_nan=True):
    """d [R, 3] fp32 -> ([R, 2] fp64 (elev, azim), bound [R, 2]); keep_nan = False: the clamp as fmin(fmax()) has it (a NaN becomes -lim)"""
    d = d.double()
    n = d.norm(dim=-1, keepdim=True).clamp(min=EPS32)
    v = d / n
    if keep_nan:
        v = v.clamp(min=-LIM32, max=LIM32)
    else:
        v = torch.from_numpy(np.fmin(np.fmax(v.numpy(), -LIM32), LIM32))
    x, y, z = v.unbind(-1)
    ref = torch.stack([z.acos(), torch.atan2(y, x)], dim=-1)
    bound = torch.stack([4 * U * (1 + 1 / (1 - z * z).sqrt()), torch.full_like(z, 4 * U * math.pi)], dim=-1)
    return ref, bound


# ================================================================================================================ mip
MIP_T = (1, 2, 5)
MIP_TS = _t(2.0 + np.array([0, 1, 2, 4, 7]) * 2.0 ** -6)


@functools.lru_cache(maxsize=None)
def mip_crop(H):
    """rays [1, H, 3, 6]: column w looks along axis w, row h scales the direction by 1 + h 2^-10 (rows differ by a dyadic step: the
    pixel radius is 2^-10 |s_w| / sqrt 3), origins on a 2^-10 grid"""
    rays = np.zeros((1, H, 3, 6), dtype=f32)
    rays[..., :3] = _dyadic((1, H, 3, 3), 401 + H, 4.0, 2.0 ** -10)
    sgn = (1.0, -1.0, 0.5)
    for h in range(H):
        for w in range(3):
            rays[0, h, w, 3 + w] = sgn[w] * (1.0 + h * 2.0 ** -10)
    return _t(rays)


def mip_t_end(T, form):
    """the closing edge: ('explicit' -> the value passed down, 'nan' -> what the kernel derives from ts, as torch's fp32 would)"""
    ts = MIP_TS[:T]
    if form == "explicit":
        return float(ts[-1]) + 2.0 ** -5
    return float(2 * ts[-1] - ts[-2]) if T > 1 else float(ts[-1] + 1)


def mip_moments(rays, ts, kind, end, dtype):
    t1 = torch.cat([ts[1:], torch.tensor([end], dtype=ts.dtype)]).to(dtype)
    t0, rd, ro = ts.to(dtype), rays[..., 3:].to(dtype), rays[..., :3].to(dtype)
    rad = O.radii_x(rd)
    if kind == "cylinder":
        t_mean, t_var, r_var = O.cylinder_moments(t0, t1, rad)
    else:
        t_mean, t_var, r_var = O.cone_moments(t0.reshape(-1, 1, 1, 1, 1), t1.reshape(-1, 1, 1, 1, 1), rad[None])
        t_mean, t_var = t_mean.reshape(-1), t_var.reshape(-1)
    mean, cov = O.lift_gaussian_intended(rd, t_mean, t_var, r_var)
    return mean + ro[None], cov, rd[None] * t_mean.reshape(-1, 1, 1, 1, 1), ro[None]


def _mip_layout(per_deg):
    """list over k of [..., 3] -> [..., 3 nd] k-major, axis-minor"""
    return torch.cat(per_deg, dim=-1)


def mip_ref(rays, ts, kind, end, min_deg=0, max_deg=16):
    """-> (features [T, B, H, W, 6 nd] fp64, bound).  The mean is the fp32 one where it is exact (cylinder, asserted), the fp64 one with
    the dm term for the cone; y = 2^k mean; the cosine half sin(fl32(y + fl32(pi / 2)))"""
    mean64, cov, dt, ro = mip_moments(rays, ts, kind, end, torch.float64)
    mean32 = mip_moments(rays, ts, kind, end, torch.float32)[0]
    if kind == "cylinder":
        assert torch.equal(mean32.double(), mean64), "the cylinder's mean is not exact in fp32"
        dm = torch.zeros_like(mean64)
    else:
        dm = K_MIP_MEAN * U * (dt.abs() + ro.abs())
    E = mip_worst()
    K = K_MIP_CYL if kind == "cylinder" else K_MIP_CONE
    hp = torch.tensor(math.pi / 2, dtype=torch.float32)
    sn, cs, bs, bc = [], [], [], []
    for k in range(min_deg, max_deg):
        y = mean64 * 2.0 ** k
        damp = (-0.5 * cov * 4.0 ** k).exp()
        if kind == "cylinder":
            yc = ((mean32 * 2.0 ** k) + hp).double()
        else:
            yc = y + float(hp)          # (the fp32 sum's rounding is an argument error of u |y|: inside the dm term)
        b = CW_MARGIN * E * damp + 0.37 * K * U + damp * 2.0 ** k * dm + TINY
        sn.append(damp * y.sin()); cs.append(damp * yc.sin()); bs.append(b); bc.append(b)
    return torch.cat([_mip_layout(sn), _mip_layout(cs)], dim=-1), torch.cat([_mip_layout(bs), _mip_layout(bc)], dim=-1)


def mip_sin_emul(m, deg, part, low=True):
    """the angle path of csrc/common.h mip_feature in numpy fp32: sin(2^deg m) (part 0) or sin(fl32(2^deg m + pi / 2)) (part 1);
    low = False: the revolution count without the low half of 1 / 2 pi"""
    m = np.asarray(m, dtype=f32)
    chi, clo = f32(np.ldexp(f32(0.15915494309189535), deg)), f32(np.ldexp(f32(6.4206383e-9), deg))
    p = m * chi
    e = _fma(m, chi, -p)
    if low:
        e = e + m * clo
    rev = (p - np.rint(p)) + e
    y = np.ldexp(m, deg).astype(f32)
    yc = y + f32(1.5707963267948966)
    delta = (yc - y) if part else np.zeros_like(y)
    return sin_cw_emul(f32(6.283185307179586) * rev + delta)


def mip_sin_ref(m, deg, part):
    m = np.asarray(m, dtype=f32)
    y = np.ldexp(m, deg).astype(f32)
    return np.sin((y + f32(1.5707963267948966)).astype(f64)) if part else np.sin(y.astype(f64))


@functools.lru_cache(maxsize=None)
def mip_args():
    """the means the crops produce (cylinder: exact) and 2 10^5 uniform ones in [-8, 8)"""
    ms = [proc_uniform((200_000,), 411, 8.0)]
    for H in (4, 2):
        for T in MIP_T:
            for form in ("explicit", "nan"):
                ms.append(mip_moments(mip_crop(H), MIP_TS[:T], "cylinder", mip_t_end(T, form), torch.float32)[0].numpy().ravel())
    return np.concatenate(ms).astype(f32)


@functools.lru_cache(maxsize=None)
def mip_worst(low=True):
    """worst error of the restated angle path against fp64 over mip_args(), degrees 0..15, both halves"""
    m = mip_args()
    return max(float(np.abs(mip_sin_emul(m, k, part, low) - mip_sin_ref(m, k, part)).max()) for k in range(16) for part in (0, 1))
