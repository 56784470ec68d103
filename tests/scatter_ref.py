"""Plain fp64 reference of the hash-table scatter (csrc/backward.hip hash_backward_kernel), the per-entry error bound the
tests hold the kernel to, and the inputs they share.  Imported by tests/test_scatter_ref.py (CPU) and tests/test_gpu_scatter.py.

Cell membership is part of the operator's definition: v = x * N_l is computed in fp32 exactly like oracle.hash_encode /
oracle.hash_corner_indices do (N_l a Python double, cast when it meets the fp32 tensor), w = v - floor(v) is exact in fp32
(Sterbenz / same binade), the indices come from oracle.hash_corner_indices.  Everything behind that is fp64.

THE BOUND (derived, not tuned).  u = 2^-24, k = cnt (addends of the row), mag = sum |addend| of the entry:

    |got - ref| <= (k + C) u mag  +  [deterministic mode]  (k 2^-40 + u |ref|)          C = 8 (12 with a tangent)

  * an addend carries at most 5 fp32 roundings (1 - w, two products, times g; the tangent variant: the cast of N_l, e * N_l,
    three products and two sums on top of the shared ones, each relative to the sum of magnitudes `mag` is built from)
  * any summation order of k terms adds at most (k - 1) u mag
  * the deterministic mode converts every addend (or every merged group of a wave) to 2^-40 fixed point once, <= 2^-41 each,
    and folds the int64 with one rounding to fp32 onto the zeroed output.
"""
import functools

import numpy as np
import torch

import oracle as O
from oracle.procedural import proc_uniform

U = 2.0 ** -24
LEVELS, ROWS, FEAT = 8, 65536, 4
LDS_ROWS = 1024   # direct-mapped rows of a workgroup's LDS table (HB_ROWS)
ROUND = 256       # samples of one round of a workgroup


def _corner_bits(c):
    return (c >> 2) & 1, (c >> 1) & 1, c & 1   # oracle._corners order: x is the slowest bit


def scatter_ref(x, g, tangent=None):
    """x [N,3] fp32, g [N,32] (per-level gradient, level-major), tangent [N,3] or None
    -> ref, mag, cnt [8,65536,4] fp64: the table gradient, sum |addend| per entry, addends per row (the same in its 4 columns)."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3 and g.shape == (x.shape[0], 32)
    N = x.shape[0]
    idx = O.hash_corner_indices(x)                      # [8, 8, N]
    res = O.hash_resolutions(LEVELS)
    ref = torch.zeros(LEVELS, ROWS, FEAT, dtype=torch.float64)
    mag = torch.zeros_like(ref)
    cnt = torch.zeros_like(ref)
    g = g.double()
    ones = torch.ones(N, FEAT, dtype=torch.float64)
    for l in range(LEVELS):
        v = x * res[l]                                  # fp32, like the oracle (and the kernels)
        w = (v - v.floor()).double()                    # exact
        iw = 1.0 - w
        gl = g[:, 4 * l:4 * l + 4]
        e = None if tangent is None else tangent.double() * res[l]
        for c in range(8):
            b = _corner_bits(c)
            ux, uy, uz = (w[:, a] if b[a] else iw[:, a] for a in range(3))
            if e is None:
                wt = ux * uy * uz
                aw = wt
            else:  # N_l <grad w_corner, e> (hash_jvp_kernel)
                sx, sy, sz = (e[:, a] if b[a] else -e[:, a] for a in range(3))
                wt = sx * uy * uz + sy * ux * uz + sz * ux * uy
                aw = (sx * uy * uz).abs() + (sy * ux * uz).abs() + (sz * ux * uy).abs()
            ref[l].index_add_(0, idx[l, c], wt[:, None] * gl)
            mag[l].index_add_(0, idx[l, c], aw[:, None] * gl.abs())
            cnt[l].index_add_(0, idx[l, c], ones)
    return ref, mag, cnt


def bound(ref, mag, cnt, det, tangent=False):
    """the per-entry bound of the module docstring; the additive constant lives HERE and nowhere else"""
    c = 12.0 if tangent else 8.0
    b = (cnt + c) * U * mag
    if det:
        b = b + cnt * 2.0 ** -40 + U * ref.abs()
    return b


def worst_ratio(got, ref, mag, cnt, det, tangent=False, where=None):
    """max over the entries of |got - ref| / bound (an entry with bound 0 must be exact: ratio 0 or inf)"""
    err = (got.detach().cpu().double() - ref).abs()
    b = bound(ref, mag, cnt, det, tangent)
    if where is not None:
        err, b = err[where], b[where]
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)   # (x / 0 = inf for x > 0)
    return float(ratio.max()) if ratio.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------- inputs
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _order(n, seed):
    """a seeded permutation of range(n)"""
    return np.argsort(proc_uniform((n,), seed, 1.0), kind="stable")


def _cell_centre(cell):
    return (np.asarray(cell, dtype=np.float64) + 0.5) / 16.0   # level 0: N_0 = 16 exactly


def input_a():
    """one cell: 256 copies of one point, gradient rows (n % 64) + 1"""
    p = proc_uniform((1, 3), 3101, 1.0) * 0.02 + _cell_centre((5, -12, 17)).astype(np.float32)
    x = np.repeat(p.astype(np.float32), 256, axis=0)
    g = np.repeat(((np.arange(256) % 64) + 1).astype(np.float32)[:, None], 32, axis=1)
    return _t(x), _t(g)


def input_b():
    """face straddle: 40 points in one cell, 24 in its neighbour across the x face, jitter 1e-3, interleaved"""
    c = np.concatenate([np.repeat(_cell_centre((-3, 8, 2))[None], 40, 0), np.repeat(_cell_centre((-2, 8, 2))[None], 24, 0)])
    x = (c + proc_uniform((64, 3), 3102, 1e-3)).astype(np.float32)[_order(64, 3103)]
    return _t(x), _t(proc_uniform((64, 32), 3104, 1.0))


def input_c():
    """192 points from 8 cells (a 2 x 2 x 2 block, whose corners are shared): ~8 lanes per cell in every wave"""
    cell = (proc_uniform((192,), 3105, 4.0) + 4.0).astype(np.int64).clip(0, 7)
    base = np.array([9, -4, -21])
    cells = base[None] + np.stack([(cell >> 2) & 1, (cell >> 1) & 1, cell & 1], axis=1)
    x = (_cell_centre(cells) + proc_uniform((192, 3), 3106, 0.02)).astype(np.float32)
    return _t(x), _t(proc_uniform((192, 32), 3107, 1.0))


D_SIZES = (1, 63, 65, 257, 1000)


def input_d(n):
    """ragged sizes, uniform in +-3"""
    return _t(proc_uniform((n, 3), 3110 + n, 3.0)), _t(proc_uniform((n, 32), 3120 + n, 1.0))


def input_e():
    """tag conflicts: 128 scattered points, each twice (1e-4 apart), in ONE round of 256 samples: about 1000 distinct table rows per
    level compete for the 1024 direct-mapped LDS rows, so owned rows and rows that fall through to the global atomics feed one table"""
    p = proc_uniform((128, 3), 3130, 3.0)
    x = np.concatenate([p, p + proc_uniform((128, 3), 3131, 1e-4)]).astype(np.float32)[_order(256, 3132)]
    return _t(x), _t(proc_uniform((256, 32), 3133, 1.0))


def tag_conflicts(x):
    """number of (level, round, LDS row) slots that two DIFFERENT table rows of the same 256-sample round map to"""
    idx = O.hash_corner_indices(x)
    n = 0
    for r0 in range(0, x.shape[0], ROUND):
        for l in range(LEVELS):
            ids = torch.unique(idx[l, :, r0:r0 + ROUND])
            rows, per_row = torch.unique(ids % LDS_ROWS, return_counts=True)
            n += int((per_row > 1).sum())
    return n


F_N = 131073   # the smallest N at which a workgroup takes two rounds (512 workgroups x 256 samples = 131072)


def input_f():
    """more than one round per workgroup; workgroup 256 has one live sample, the rest none"""
    return _t(proc_uniform((F_N, 3), 3140, 1.5)), _t(proc_uniform((F_N, 32), 3141, 1.0))


def input_g():
    """exact arithmetic on level 0: x = k / 64 in a 2 x 2 x 2 block of level-0 cells around the origin (weights are multiples of 1/4,
    their products of 1/64), integer gradients |g| <= 8, tangent components in {0, +-1, +-0.5}: every level-0 sum is exact in
    fp32 (< 2^15 with 6 fractional bits; tangent: < 2^21 with 1) and in 2^-40 fixed point"""
    k = (proc_uniform((4096, 3), 3150, 4.0) + 4.0).astype(np.int64).clip(0, 7) - 4
    x = (k.astype(np.float64) / 64.0).astype(np.float32)
    g = np.rint(proc_uniform((4096, 32), 3151, 8.0)).astype(np.float32)
    t = np.array([0.0, 1.0, -1.0, 0.5, -0.5], dtype=np.float32)[(proc_uniform((4096, 3), 3152, 2.5) + 2.5).astype(np.int64).clip(0, 4)]
    return _t(x), _t(g), _t(t)


def tangent_for(n, seed=3160):
    return _t(proc_uniform((n, 3), seed + n % 97, 1.0))


def pad64(x, g, t=None, seed=3170):
    """N padded to a whole number of waves with further uniform points"""
    n = x.shape[0]
    m = (-n) % 64
    if m == 0:
        return (x, g) if t is None else (x, g, t)
    x = torch.cat([x, _t(proc_uniform((m, 3), seed, 1.5))])
    g = torch.cat([g, _t(proc_uniform((m, 32), seed + 1, 1.0))])
    if t is None:
        return x, g
    return x, g, torch.cat([t, _t(proc_uniform((m, 3), seed + 2, 1.0))])


def limits_input():
    """the limits of the fixed-point format on exact integers: 1024 samples ON vertices of the level-0 grid (weight 1 on corner 0, 0 on
    the others), integer gradients.  Sample 0 sits on the origin and carries, in the four level-0 columns,
      2^20 (bypass), 2^22 (bypass), the largest fp32 below 2^20 (stays in the accumulator), 2^19;
    samples 64, 128, ... 704 (one per wave: a wave merges its lanes first, two of them would reach 2^20 and bypass) sit on the origin
    too with 2^19 in column 3: twelve addends, 6291456 < 2^23.  Every other sample adds small integers to the same rows through
    the fixed-point path (column 2: non-positive ones, so that the total stays below 2^20 where 1/16 is representable).
    A wave merges the lanes that share a row BEFORE the threshold is applied, so what meets `|v| < 2^20` is the wave's merged sum:
    the other lanes of wave 0 carry zeros in columns 0 .. 2, and the values above reach the threshold as they are (exactly 2^20
    in column 0: the edge of the comparison).  The small integers come from the other waves -- of the same workgroup, through its
    LDS rows, and of the three other workgroups."""
    n = 1024
    k = (proc_uniform((n, 3), 3180, 1.0) + 1.0).astype(np.int64).clip(0, 1) - 1      # vertices -1/16 and 0 per axis
    k[::64] = 0
    x = (k.astype(np.float64) / 16.0).astype(np.float32)
    g = np.rint(proc_uniform((n, 32), 3181, 8.0)).astype(np.float32)
    g[:, 2] = -np.abs(g[:, 2])
    g[:, 3] = 0.0
    g[1:64, 0:3] = 0.0
    g[0, 0], g[0, 1], g[0, 2] = 2.0 ** 20, 2.0 ** 22, np.nextafter(np.float32(2.0 ** 20), np.float32(0))
    g[0:768:64, 3] = 2.0 ** 19
    return _t(x), _t(g)


@functools.lru_cache(maxsize=None)
def case(name):
    """(x, g, tangent) of a named input: 'A', 'B', 'C', 'D<n>', 'E', 'F', 'G'"""
    if name == "G":
        return input_g()
    x, g = {"A": input_a, "B": input_b, "C": input_c, "E": input_e, "F": input_f}[name]() if name[0] != "D" else input_d(int(name[1:]))
    return x, g, tangent_for(x.shape[0])


@functools.lru_cache(maxsize=None)
def reference(name, tangent):
    """scatter_ref of a named input, computed once per process and shared (callers must not modify it)"""
    x, g, t = case(name)
    return scatter_ref(x, g, t if tangent else None)


CASES = ("A", "B", "C") + tuple(f"D{n}" for n in D_SIZES) + ("E", "F", "G")
