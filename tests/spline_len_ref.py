"""Plain reference of the spline-length operators (csrc/spline_len.hip; arc_len, src/nerf.py:1509-1520 and runner.py:784-796 of the
reference) and the error bounds the tests hold the kernels to.  Imported by tests/test_spline_len_ref.py (CPU),
tests/test_gpu_spline_len.py and tests/test_gpu_spline_len_train.py.

The t table is torch.linspace(0, 1, 16)'s own fp32 values (T_TABLE), cast to fp64; cell membership and xyz of the per-sample term come
from voxel_ref.cells (the reference's fp32 chain, part of the operator's definition); everything else is fp64 here.  The points are
evaluated by de Casteljau's levels in fp64 (not as a sum of Bernstein products), so control points whose products with t and 1 - t
are exact -- zeros, powers of two -- give bitwise equal points, segments of length exactly 0 and, by the rule below, gradient exactly
0, as in the fp32 operators.

THE BOUNDS (derived, not tuned; first order in u = voxel_ref.U = 2^-24 unless stated; `mag` is always a sum of ABSOLUTE values of the
addends).  n control points c_k (k = 0 .. n-1), M = 16 points, t_j in [0, 1], so the Bernstein weights B_k(t_j) are >= 0 and sum to 1.

  inputs   grid term: c_ka is a grid entry, exact: e(c) = 0, mag_ka = |c_ka|, GATHER = 0.  Per-sample term: c_0 = 0 exactly and
           c_ka = sum_u w_u v_u is voxel_ref's gather: e(c) <= SAMPLE_C u mag_ka, mag_ka = sum_u |w_u| |v_u|, GATHER = SAMPLE_C.
  point    p_ja = sum_k B_k(t_j) c_ka by n - 1 levels of b <- b (1 - t) + b' t: per level the rounding of 1 - t, of the product and
           of the add, 3 u, on non-negative weights (dyn_voxel_ref's count), on top of the inputs' error:
               e(p_ja) <= POINT_C u magp_ja,  magp_ja = sum_k B_k(t_j) mag_ka,  POINT_C = GATHER + 3 (n - 1) [+ 1 for second order
               where that is not 0: a one-point spline of exact inputs is exact]
  segment  d_ja = p_{j+1,a} - p_ja: e(d_ja) <= e(p_{j+1,a}) + e(p_ja) + u |d_ja|.  len_j = |d_j|_2: NOT first order -- the triangle
           inequality | |d + e| - |d| | <= |e|_2 <= sum_a e(d_ja) =: E_j holds for any e, however short the segment --, plus the
           squares' and the two adds' roundings halved by the root and sqrtf's own, 3 u len_j, plus 2^-63 where len_j > 0 (squares below
           the normal range lose relative accuracy):   e(len_j) <= E_j + 3 u len_j + [len_j > 0] 2^-63
  length   L = sum_j len_j, 15 addends in any order: e(L) <= sum_j e(len_j) + (M - 2) u L
  value    addend a = w L (the product's rounding u |w L|; none without w).  The kernel's order of the sum (csrc/spline_len.hip): a
           thread holds one addend (N <= 2^26), the 64 lanes of a wave are added by a tree of depth 6, the 4 waves of a workgroup in
           order (3 additions), and the GROUPS = ceil(N / 256) partial sums by one atomic each in arrival order: no addend passes
           through more than 9 + GROUPS additions.  The division in double and one rounding:
               e(mean) <= (sum e(a) + (9 + GROUPS) u sum |a|) / N + u |mean|   + [deterministic mode] GROUPS 2^-40 / N
           (every workgroup's partial sum rounded to 2^-40 fixed point on its own).
  gradient d L / d c_ka = sum_j dir_ja dB_jk,  dir_j = d_j / len_j (0 where len_j = 0),  dB_jk = B_k(t_{j+1}) - B_k(t_j).
           dir_j: a segment's direction error is its difference's error over its length, | d^/|d^| - d/|d| | <= 2 |e|_2 / |d|_2 for
           any e, and never more than 2 (two vectors of length <= 1): near-degenerate segments widen their own bound and are not
           excluded; a segment whose difference is exactly 0 with E_j = 0 is exactly 0 in the kernel too and has bound 0.  On top, the
           root's 3 u and the division's 1 u:   e(dir_ja) <= min(2, 2 E_j / len_j) + 4 u |dir_ja|
           dB_jk: the recurrence on the weights is n - 1 levels of 3 u each on non-negative terms, the difference one rounding:
               e(dB_jk) <= (3 (n - 1) + 1) u (B_k(t_{j+1}) + B_k(t_j))          (n = 1: dB = 0 exactly)
           the products' roundings and the sum of M - 1 of them in any order: (M - 1) u absG_ka, absG_ka = sum_j |dir_ja| |dB_jk|:
               e(G_ka) <= sum_j (|dir_ja| e(dB_jk) + |dB_jk| e(dir_ja)) + (M - 1) u absG_ka
  scatter  grid term: the addend s G_ka with s = g_up / K (the quotient's rounding, the product's, 1 u second order):
               e(addend) <= |s| (e(G_ka) + 3 u absG_ka)
           per-sample term: the addend w_u s G_ka with s = g_up w[n] / N (quotient, times w[n], times G: 3) and w_u with the final
           product (4, voxel_ref's count), 1 u second order:   e(addend) <= |w_u| |s| (e(G_ka) + 8 u absG_ka)
           An entry sums cnt addends in any order (the LDS rows and the global atomics are one such order):
               |got - ref| <= sum e(addend) + cnt u mag   + [deterministic mode] (cnt 2^-40 + u |ref|),   mag = sum |addend| formed with absG
           (every addend rounded to 2^-40 fixed point on its own, <= 2^-41 each, and one rounding when the integer sum is folded).
An entry with bound 0 must be exact; no entry is left out of a comparison (voxel_ref.worst_ratio).
"""
from math import comb

import numpy as np
import torch

import voxel_ref as V
from oracle.procedural import proc_uniform

U = V.U
M = 16
T_TABLE = torch.linspace(0, 1, M)     # fp32: what the operators are given
ROUND = 256                            # samples of one round of a workgroup
F_N = 4096 * 256 + 1                   # the smallest N at which a workgroup of the backward takes two rounds (DV_WG x 256 samples)
SPLINES = (2, 4, 5, 11)
CHUNK = 1 << 15


def bernstein(n):
    """B_k(t_j), k = 0 .. n-1, of degree n - 1 at the table's points in fp64: [M, n]"""
    t = T_TABLE.double()
    return torch.stack([comb(n - 1, k) * t ** k * (1 - t) ** (n - 1 - k) for k in range(n)], dim=-1)


def points(cp):
    """de Casteljau's levels in fp64: cp [N, n, 3] -> [N, M, 3]"""
    t = T_TABLE.double()[None, :, None, None]
    b = cp[:, None].expand(-1, M, -1, -1)
    for _ in range(1, cp.shape[1]):
        b = b[:, :, :-1] * (1 - t) + b[:, :, 1:] * t
    return b[:, :, 0]


def _arc_chunk(cp, mag, gather_c):
    n = cp.shape[1]
    B = bernstein(n)
    p = points(cp)
    point_c = gather_c + 3.0 * (n - 1)
    point_c = point_c + (1.0 if point_c > 0 else 0.0)
    e_p = point_c * U * torch.einsum("jk,nka->nja", B, mag)
    d = p[:, 1:] - p[:, :-1]
    e_d = e_p[:, 1:] + e_p[:, :-1] + U * d.abs()
    seg = d.square().sum(-1).sqrt()                                   # [N, M-1]
    E = e_d.sum(-1)
    e_seg = E + 3 * U * seg + torch.where(seg > 0, torch.full_like(seg, 2.0 ** -63), torch.zeros_like(seg))
    L = seg.sum(-1)
    b_L = e_seg.sum(-1) + (M - 2) * U * L
    zero = seg == 0
    dirs = torch.where(zero[..., None], torch.zeros_like(d), d / seg[..., None])
    rel = torch.where(zero & (E == 0), torch.zeros_like(E), torch.minimum(torch.full_like(E, 2.0), 2 * E / seg))
    rel = torch.where(zero & (E > 0), torch.full_like(E, 2.0), rel)
    e_dir = rel[..., None] + 4 * U * dirs.abs()                       # [N, M-1, 3]
    dB = B[1:] - B[:-1]                                               # [M-1, n]
    e_dB = (3.0 * (n - 1) + 1.0) * U * (B[1:] + B[:-1]) if n > 1 else torch.zeros_like(dB)
    G = torch.einsum("nja,jk->nka", dirs, dB)
    absG = torch.einsum("nja,jk->nka", dirs.abs(), dB.abs())
    e_G = torch.einsum("nja,jk->nka", dirs.abs(), e_dB) + torch.einsum("nja,jk->nka", e_dir, dB.abs()) + (M - 1) * U * absG
    return L, b_L, G, e_G, absG


def arc(cp, mag, gather_c):
    """cp, mag [N, n, 3] fp64 -> per spline: length L [N] and its bound, d L / d cp G [N, n, 3], its bound and absG (module docstring)"""
    parts = [_arc_chunk(cp[i:i + CHUNK], mag[i:i + CHUNK], gather_c) for i in range(0, cp.shape[0], CHUNK)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(5))


def _mean(a, e_a):
    """(value, bound, bound in the deterministic mode)"""
    N = a.shape[0]
    value = a.sum() / N
    groups = -(-N // 256)
    bound = (e_a.sum() + (9 + groups) * U * a.abs().sum()) / N + U * value.abs()
    return value, bound, bound + groups * 2.0 ** -40 / N


def _scatter_bound(ref, err, mag, cnt):
    """(bound, bound in the deterministic mode)"""
    b = err + cnt * U * mag
    return b, b + cnt * 2.0 ** -40 + U * ref.abs()


def _result(L, b_L, mean, ref, scatter, **more):
    return dict(lens=L, b_lens=b_L, value=mean[0], b_value=mean[1], b_value_det=mean[2], grad=ref, b_grad=scatter[0], b_grad_det=scatter[1], **more)


def bound(r, what, det):
    return r["b_" + what + ("_det" if det else "")]


# ------------------------------------------------------------------------------------------------------------ the grid term
def grid_ref(grid, rows, g_up=1.0):
    """grid [R, 3 m] fp32 (a control-point grid flattened to rows), rows [K] int64 -> dict of fp64 tensors: lens [K], value, grad [R, 3 m]
    (the gradient of value times g_up) and their bounds b_lens, b_value, b_grad (+ b_value_det, b_grad_det for the deterministic mode: `bound`)"""
    R, m = grid.shape[0], grid.shape[1] // 3
    K = rows.shape[0]
    cp = grid.double()[rows].reshape(K, m, 3)
    L, b_L, G, e_G, absG = arc(cp, cp.abs(), 0.0)
    s = abs(float(g_up)) / K
    ref, err, mag, cnt = (torch.zeros(R, 3 * m, dtype=torch.float64) for _ in range(4))
    ref.index_add_(0, rows, (float(g_up) / K) * G.reshape(K, -1))
    err.index_add_(0, rows, s * (e_G + 3 * U * absG).reshape(K, -1))
    mag.index_add_(0, rows, s * absG.reshape(K, -1))
    cnt.index_add_(0, rows, torch.ones(K, 3 * m, dtype=torch.float64))
    return _result(L, b_L, _mean(L, b_L), ref, _scatter_bound(ref, err, mag, cnt))


def rows_of_flat(idxs, shape):
    """the memory row of the voxel that random_sample_grid's decode of a flat index names: x = idx % s0 is the slowest axis"""
    s0, s1, s2 = shape[:3]
    return ((idxs % s0) * s1 + idxs // s0 % s1) * s2 + idxs // (s0 * s1) % s2


# ------------------------------------------------------------------------------------------------------------ the per-sample term
def dyn_ref(pts, ctrl, spline, w=None, g_up=1.0, grid_radius=V.GRID_RADIUS):
    """pts [N,3] fp32, ctrl [S,S,S,3(n-1)] fp32, w [N] or None -> dict of fp64 tensors: lens [N], value (the mean of w lens), grad
    [S^3, 3(n-1)] (the gradient of value w.r.t. ctrl_pts_grid times g_up), their bounds as grid_ref names them, and `rows` [N,8], the
    rows every sample reads"""
    S, n, N = ctrl.shape[0], spline, pts.shape[0]
    ids, xyz = V.cells(pts, S, grid_radius)
    rows, wt = V.rows_of(ids, S), V.weights_of(xyz)                   # [N,8]
    cv = ctrl.double().reshape(S ** 3, n - 1, 3)[rows]                # [N,8,n-1,3]
    prod = wt[..., None, None] * cv
    z = torch.zeros(N, 1, 3, dtype=torch.float64)
    cp, mag = torch.cat([z, prod.sum(dim=1)], dim=1), torch.cat([z, prod.abs().sum(dim=1)], dim=1)
    L, b_L, G, e_G, absG = arc(cp, mag, V.SAMPLE_C)
    wd = torch.ones(N, dtype=torch.float64) if w is None else w.double().reshape(N)
    a = wd * L
    e_a = wd.abs() * b_L + (0.0 if w is None else 1.0) * U * a.abs()
    s = (float(g_up) / N) * wd                                        # [N]
    Gk, eG, aG = (x[:, 1:].reshape(N, -1) for x in (G, e_G + 8 * U * absG, absG))
    ref, err, mag_, cnt = (torch.zeros(S ** 3, 3 * (n - 1), dtype=torch.float64) for _ in range(4))
    ones = torch.ones(N, 3 * (n - 1), dtype=torch.float64)
    for u in range(8):
        ws = wt[:, u] * s
        ref.index_add_(0, rows[:, u], ws[:, None] * Gk)
        err.index_add_(0, rows[:, u], ws.abs()[:, None] * eG)
        mag_.index_add_(0, rows[:, u], ws.abs()[:, None] * aG)
        cnt.index_add_(0, rows[:, u], ones)
    return _result(L, b_L, _mean(a, e_a), ref, _scatter_bound(ref, err, mag_, cnt), rows=rows)


# ------------------------------------------------------------------------------------------------------------ inputs
def ctrl_grid(S, spline, seed=5700):
    """ctrl_pts_grid [S,S,S,3(n-1)] uniform in +-1"""
    return V._t(proc_uniform((S, S, S, 3 * (spline - 1)), seed + spline, 1.0))


def flat_grid(rows, m, seed=5750):
    """a control-point grid as the grid operators see it: [rows, 3 m] uniform in +-1"""
    return V._t(proc_uniform((rows, 3 * m), seed + m + rows, 1.0))


def indices(K, rows, seed=5800):
    """K seeded flat rows in 0 .. rows-1 (with duplicates once K > rows, as a draw with replacement has them)"""
    return V._t(((proc_uniform((K,), seed + K + rows, 0.5) + 0.5) * rows).astype(np.int64).clip(0, rows - 1))


def sample_weights(N, kind, seed=5900):
    """w [N]: None, signed uniform in +-1, or all zero"""
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(N)
    return V._t(proc_uniform((N,), seed + N, 1.0))


def fixture_points(g):
    """the sample positions of a g26 fixture: o + t d of its rays at its ts, [T H W, 3] in the fixture's [T, 1, H, W] order"""
    return V.pts_of(g["rays"], g["ts"]).reshape(-1, 3)
