"""Plain references of the grid operators (csrc/grid_ops.hip; total_variation and upsample_grid, src/nerf.py:377-399 of the reference), the
error bounds the tests hold the kernels to, and the inputs they share.  Imported by tests/test_grid_ref.py (CPU) and
tests/test_gpu_grid.py.

TOTAL VARIATION.  The index decode is integer -- x = idx % s0, y = idx // s0 % s1, z = idx // (s0 s1) % s2: x is the FASTEST digit of idx
and the SLOWEST axis in memory, the reference's quirk --, the neighbour is v + 1, or v - 1 where v == s - 1.  The differences
d = voxel - neighbour and q = (dx^2 + dy^2) + dz^2 are torch operations on the CPU IN THE GRID'S DTYPE: fp32 for the operator (the
gradient jumps at q = fp32(1e-10), so which side an element is on is part of the operator's definition), fp64 for a `.double()` grid
(what the g24 fixtures record next to the fp32 value).  Everything behind q is fp64: t = sqrt(max(q, fp32(1e-10))), the mean, and the
gradient -- nothing where q < fp32(1e-10) (torch's clamp passes the gradient where q >= min), else (dx + dy + dz) w to the voxel and -d w
to each neighbour, w = (g / K) / t, K = samples x C.  A NaN q passes no gradient either (torch), so its addends are d x 0: NaN exactly
where the difference is not finite; an Inf q has w = 0 the same way.

`tv_ref(clean=True)` asserts that NO element sits near the jump: every q is exactly 0 or above 1e-8.  It leaves out no element.

THE BOUNDS (derived, not tuned; first order in u = 2^-24).
  value     an element's t carries the roundings of three differences, three squares, two adds and a sqrtf: 4 u t.  The kernel's sum: a
            thread adds the C values of its sample in channel order (C x trips - 1 additions, trips = ceil(n / (64 x 2^20)) = 1 below
            2^26 samples), wave_total_lane63 adds the 64 threads of a wave as a tree of depth 6, the P = min(ceil(n / 64), 2^20) waves'
            partials arrive by one atomic each in any order (at most P - 1 roundings on one path), one division by K.  All terms are
            >= 0, so every partial sum is below the total:
                |got - ref| <= (4 + (C trips - 1) + 6 + (P - 1) + 1) u mean(t)                         fp32 atomics
                |got - ref| <= (4 + (C trips - 1) + 6 + 1) u mean(t) + P 2^-41 / K                     deterministic mode
            (there each partial is rounded to 2^-40 fixed point, <= 2^-41, and the integers add exactly).
  gradient  voxel_ref.scatter_bound's form: |got - ref| <= (k + GRAD_C0) u mag + [deterministic mode] (k 2^-40 + u |ref|), k = addends
            of the entry, mag = sum |addend| -- for the voxel's own addend (|dx| + |dy| + |dz|) |w|, the three differences may cancel.
            GRAD_C0 = 8: one rounding for the difference, four for t, one each for the division, the scale and the slack of second order.
  upsample  the reference is F.interpolate on the float64 grid (its coordinates are float64).  blend term 12 u sum |w v| as for the
            voxel gather (1 - lambda, two products of the weight, times v, seven additions, one of slack) + coordinate term: the fp32
            source coordinate src = max(scale (i + 0.5) - 0.5, 0) is at most two ulps of src off the exact one per axis (`up_axis`
            ASSERTS this for every coordinate it forms), and the output moves by |d out / d lambda| = the blend of |difference of the two
            planes| per unit of it.
An entry whose bound is 0 must be exact.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.procedural import proc_uniform

U = 2.0 ** -24
TV_MIN = float(np.float32(1e-10))   # what the fp32 tensor is compared with
TV_CLEAN = 1e-8
VALUE_C_T = 4.0
GRAD_C0 = 8.0
BLEND_C = 12.0
MAX_WAVES = 1 << 20


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------ total variation
def decode(idxs, shape):
    """flat indices [n] int64 -> (x, y, z) and the neighbours (ax, ay, az), all int64 -- the reference's digits"""
    s0, s1, s2 = (int(s) for s in shape[:3])
    assert idxs.dtype == torch.int64 and min(s0, s1, s2) >= 2
    x, y, z = idxs % s0, (idxs // s0) % s1, (idxs // (s0 * s1)) % s2
    adj = lambda v, s: torch.where(v == s - 1, v - 1, v + 1)
    return (x, y, z), (adj(x, s0), adj(y, s1), adj(z, s2))


def tv_ref(grid, idxs, g=1.0, clean=True):
    """grid [s0,s1,s2,C] (fp32: the operator; fp64: the reference's `.double()` run), idxs [n] int64, upstream scalar g ->
    dict(value, grad [s0,s1,s2,C], mag, cnt (all fp64), q [n,C] in the grid's dtype)"""
    assert grid.dim() == 4 and grid.dtype in (torch.float32, torch.float64) and not grid.is_cuda
    (x, y, z), (ax, ay, az) = decode(idxs, grid.shape)
    e = grid[x, y, z]
    dx, dy, dz = e - grid[ax, y, z], e - grid[x, ay, z], e - grid[x, y, az]
    q = (dx * dx + dy * dy) + dz * dz
    assert q.dtype == grid.dtype
    if clean:
        assert bool(((q == 0) | (q > TV_CLEAN)).all()), "an element of a bounded case sits near the clamp's jump"
    n, C = q.shape
    K = n * C
    q64 = q.double()
    passes = q64 >= TV_MIN                                     # (False for NaN, like torch's clamp)
    t = torch.where(torch.isnan(q64), q64, q64.clamp(min=TV_MIN)).sqrt()
    w = torch.where(passes, (float(g) / K) / t, torch.zeros_like(t))
    d = [v.double() for v in (dx, dy, dz)]
    own = ((d[0] + d[1]) + d[2]) * w
    own_mag = ((d[0].abs() + d[1].abs()) + d[2].abs()) * w.abs()
    counted = (passes | torch.isnan(q64)).double()             # elements the kernel forms addends for
    S = grid.shape
    flat = lambda i, j, k: ((i * S[1] + j) * S[2] + k)
    grad = torch.zeros(S[0] * S[1] * S[2], C, dtype=torch.float64)
    mag, cnt = torch.zeros_like(grad), torch.zeros_like(grad)
    for rows, a, m in ((flat(x, y, z), own, own_mag), (flat(ax, y, z), -(d[0] * w), None), (flat(x, ay, z), -(d[1] * w), None),
                       (flat(x, y, az), -(d[2] * w), None)):
        grad.index_add_(0, rows, a)
        m = a.abs() if m is None else m
        mag.index_add_(0, rows, torch.where(torch.isnan(m), torch.zeros_like(m), m))
        cnt.index_add_(0, rows, counted)
    return dict(value=t.mean(), grad=grad.reshape(tuple(S)), mag=mag.reshape(tuple(S)), cnt=cnt.reshape(tuple(S)), q=q)


def waves(n):
    return min((n + 63) // 64, MAX_WAVES)


def value_bound(value, n, C, det):
    """the module docstring's bound of the TV value; value = mean(t) >= 0 in fp64"""
    trips = (n + 64 * MAX_WAVES - 1) // (64 * MAX_WAVES)
    P = waves(n)
    c = VALUE_C_T + (C * trips - 1) + 6 + 1 + (0 if det else P - 1)
    return c * U * abs(float(value)) + (P * 2.0 ** -41 / (n * C) if det else 0.0)


def grad_bound(ref, det):
    """per-entry bound of the TV gradient (ref: tv_ref's dict); the additive constant lives HERE and nowhere else"""
    b = (ref["cnt"] + GRAD_C0) * U * ref["mag"]
    if det:
        b = b + ref["cnt"] * 2.0 ** -40 + U * torch.nan_to_num(ref["grad"].abs(), nan=0.0, posinf=0.0)
    return b


def worst_ratio(got, ref, bound):
    """max over ALL entries of |got - ref| / bound (bound 0: the entry must be exact -- ratio 0 or inf); NaN where the two disagree about
    NaN, entries that are NaN in both count as equal"""
    got = got.detach().cpu().double().reshape(ref.shape)
    if bool((torch.isnan(got) != torch.isnan(ref)).any()):
        return float("nan")
    both_nan = torch.isnan(got) & torch.isnan(ref)
    err = torch.where(both_nan, torch.zeros_like(ref), (got - ref).abs())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


# inputs ------------------------------------------------------------------------------------------------------
TV_GRIDS = {"2x1": (2, 2, 2, 1), "4x3": (4, 4, 4, 3), "462x5": (4, 6, 2, 5), "16x28": (16, 16, 16, 28), "64x3": (64, 64, 64, 3)}
TV_COUNTS = (1, 63, 64, 65, 257, 32768)


@functools.lru_cache(maxsize=None)
def tv_grid(name):
    """uniform in +-1 (callers must not modify it)"""
    shape = TV_GRIDS[name]
    return _t(proc_uniform(shape, 5200 + sum(shape), 1.0))


def tv_idxs(n, n_elem, seed=5300):
    """n flat indices uniform over the grid, with replacement"""
    u = proc_uniform((n,), seed + n + n_elem, 0.5).astype(np.float64) + 0.5
    return _t(np.clip((u * n_elem).astype(np.int64), 0, n_elem - 1))


@functools.lru_cache(maxsize=None)
def tv_reference(name, n, g=1.0):
    """tv_ref of a named grid at tv_idxs, computed once per process and shared (callers must not modify it)"""
    grid = tv_grid(name)
    return tv_ref(grid, tv_idxs(n, grid[..., 0].numel()), g)


def duplicate_cases():
    """(name, grid, idxs): 256 copies of one index; a face-neighbour pair interleaved -- each row is voxel and (z-)neighbour"""
    grid = tv_grid("4x3")
    one = torch.full((256,), 27, dtype=torch.int64)                      # x = 3 (last plane: neighbour x - 1), y = 2, z = 1
    a = 1 + 4 * 2 + 16 * 1                                                # (x, y, z) = (1, 2, 1); its z-neighbour is (1, 2, 2)
    pair = torch.tensor([a, a + 16] * 64, dtype=torch.int64)
    return (("256 copies", grid, one), ("face pair", grid, pair))


# ------------------------------------------------------------------------------------------------------------ upsample
UP_CASES = ((2, 2, 1), (2, 4, 3), (4, 6, 28), (4, 2, 1), (16, 32, 3), (6, 16, 28), (64, 128, 1))   # (S, R, C), C cycled over (1, 3, 28)


def up_grid(S, C, seed=5400):
    return _t(proc_uniform((S, S, S, C), seed + S + C, 1.0))


def up_axis(S, R):
    """ATen's source coordinate of every output index along one axis, restated in fp32 torch operation by operation:
    scale = (float)S / R, src = max(fmaf(scale, i + 0.5f, -0.5f), 0), i0 = floor(src) (at most S - 1), i1 = min(i0 + 1, S - 1),
    lambda = src - i0 clamped to [0, 1].  -> i0, i1 int64 [R], lambda fp32 [R], dsrc fp64 [R] = two ulps of src"""
    scale = torch.tensor(float(S), dtype=torch.float32) / torch.tensor(float(R), dtype=torch.float32)
    # ONE rounding for scale * (i + 0.5) - 0.5: torch's builds contract ATen's expression into a fused multiply-add (the separately
    # rounded product puts src one ulp away at 4 -> 6, i = 3, and torch's fp32 result then leaves the blend bound:
    # tests/test_grid_ref.py).  The product of two fp32 numbers and the subtraction of 0.5 are exact in float64 at these magnitudes.
    src = (scale.double() * (torch.arange(R, dtype=torch.float64) + 0.5) - 0.5).float().clamp(min=0)
    assert src.dtype == torch.float32
    i0 = src.floor().long().clamp(max=S - 1)
    i1 = (i0 + 1).clamp(max=S - 1) if R != S else i0      # (R == S: ATen copies, both sources are voxel i itself)
    lam = (src - i0.float()).clamp(0, 1)
    ulp = (torch.nextafter(src, torch.tensor(float("inf"))) - src).double()
    dsrc = torch.where(src == 0, torch.zeros_like(ulp), 2 * ulp)
    exact = ((S / R) * (torch.arange(R, dtype=torch.float64) + 0.5) - 0.5).clamp(min=0)
    assert bool(((src.double() - exact).abs() <= dsrc).all()), "the fp32 source coordinate is more than two ulps off"
    assert bool((exact.floor().long().clamp(max=S - 1) == i0).all()), "fp32 and fp64 disagree about the cell"
    return i0, i1, lam, dsrc


def upsample_chain(grid, R):
    """grid [S,S,S,C] fp32 -> (value, blend magnitude sum |w v|, coordinate term) [R,R,R,C] fp64: the fp32 coordinate chain, the blend of
    the 8 sources in fp64"""
    S, C = grid.shape[0], grid.shape[-1]
    i0, i1, lam, dsrc = up_axis(S, R)
    idx, wt = (i0, i1), (1 - lam.double(), lam.double())
    v = grid.double()
    sh = lambda t, a: t.reshape([R if k == a else 1 for k in range(3)] + [1])
    val = torch.zeros(R, R, R, C, dtype=torch.float64)
    mag = torch.zeros_like(val)
    coord = torch.zeros_like(val)
    corner = lambda a, b, c: v[idx[a]][:, idx[b]][:, :, idx[c]]
    for a in range(2):
        for b in range(2):
            for c in range(2):
                w = sh(wt[a], 0) * sh(wt[b], 1) * sh(wt[c], 2)
                val += w * corner(a, b, c)
                mag += (w * corner(a, b, c)).abs()
    for a in range(2):
        for b in range(2):   # |plane 1 - plane 0| along each axis, blended over the other two
            coord += sh(dsrc, 0) * sh(wt[a], 1) * sh(wt[b], 2) * (corner(1, a, b) - corner(0, a, b)).abs()
            coord += sh(dsrc, 1) * sh(wt[a], 0) * sh(wt[b], 2) * (corner(a, 1, b) - corner(a, 0, b)).abs()
            coord += sh(dsrc, 2) * sh(wt[a], 0) * sh(wt[b], 1) * (corner(a, b, 1) - corner(a, b, 0)).abs()
    return val, mag, coord


def interpolate(grid, R):
    """torch's own F.interpolate on a channel-last grid, in the grid's dtype (src/nerf.py:377-379)"""
    return F.interpolate(grid.permute(3, 0, 1, 2)[None], size=R, mode="trilinear").squeeze(0).permute(1, 2, 3, 0).contiguous()


@functools.lru_cache(maxsize=None)
def up_reference(S, R, C):
    """(grid, F.interpolate of the float64 grid, per-entry bound), computed once per process and shared"""
    grid = up_grid(S, C)
    _, mag, coord = upsample_chain(grid, R)
    return grid, interpolate(grid.double(), R), BLEND_C * U * mag + coord
