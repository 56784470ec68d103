"""Plain reference of NeRFVoxel's grid lookup (csrc/voxel.hip; src/nerf.py:493-524 of the reference), the error bounds the tests hold
the kernels to, and the inputs they share.  Imported by tests/test_voxel_ref.py (CPU) and tests/test_gpu_voxel.py.

CELL MEMBERSHIP IS PART OF THE OPERATOR'S DEFINITION.  The lower and the upper neighbour of a point come from two independent
floors, so on the planes p = (k + 0.5) voxel_len one ulp decides which pair of cells is read, and the result then moves by the size
of the grid values: the reference's own fp32 and fp64 runs disagree there.  `cells` therefore restates the reference's chain up to
and including xyz in fp32 torch on the CPU, operation by operation in the reference's order
    (-h) + p, h + p  ->  clamp +-grid_radius  ->  / voxel_len  ->  + 1e-10  ->  floor  ->  + 0.5  ->  * voxel_len
    ->  clamp +-(grid_radius - voxel_len / 2)  ->  xyz = (p - centre of corner 0) / voxel_len,  ids = floor(centre / voxel_len + 1e-10) + S / 2
with the Python doubles (voxel_len = grid_radius * 2 / S, ...) cast to fp32 where they meet the fp32 tensor, exactly as in the
reference (tests/test_voxel_ref.py holds ids and xyz to the reference's fp32 ones bit for bit on the g23 fixtures).  Everything behind
xyz -- 1 - x, the weights' products, times the grid values, the sums -- is fp64 here.  A sample with a non-finite xyz (a NaN or Inf
coordinate) is NaN in every output.

THE BOUNDS (derived, not tuned; first order in u = 2^-24).  mag = sum |w_c| |v_c| of an output, NOT |output|: outside the grid the
weights alternate in sign and grow polynomially (3.0e4 at S = 64 at the corner of |p| <= 2.5) while their sum stays 1.

  gather    |got - ref| <= SAMPLE_C u mag,  SAMPLE_C = 12:
            an addend w_c v_c carries 4 fp32 roundings (1 - x, two products of the weight, times v_c), summing 8 addends in any order
            adds at most 7 u mag, and 1 u covers the terms of second order
  scatter   |got - ref| <= (k + SCATTER_C0) u mag  +  [deterministic mode]  (k 2^-40 + u |ref|),  SCATTER_C0 = 4, k = addends of the entry:
            an addend w_c g carries the same 4 roundings, any summation order of k terms adds at most (k - 1) u mag (the LDS rows
            and the global atomics are one such order); the deterministic mode converts every addend to 2^-40 fixed
            point on its own (<= 2^-41 each) and folds the exact integer sum with one rounding to fp32 onto the zeroed output
An entry with bound 0 must be exact.
"""
import functools

import numpy as np
import torch

import oracle as O
from oracle.procedural import proc_uniform

U = 2.0 ** -24
SAMPLE_C = 12.0
SCATTER_C0 = 4.0
TINY = 1e-10       # the reference's additive constant in front of both floors
GRID_RADIUS = 1.3  # NeRFVoxel's default
LDS_ROWS = 1024    # rows of a workgroup's hashed LDS table (VB_ROWS)
ROUND = 256        # samples of one round of a workgroup
F_N = 1048577      # the smallest N at which a workgroup takes two rounds (VB_WG = 4096 workgroups x 256 samples = 1048576)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bit_i(v, bit):
    return (v >> bit) & 1


# ------------------------------------------------------------------------------------------------------------ the lookup
def axis_cells(p, S, grid_radius=GRID_RADIUS):
    """one coordinate p [N] fp32 -> (id of the lower cell, id of the upper cell) int64 and the fraction [N] fp32, every step an fp32
    torch operation in the order of the module docstring (the Python doubles meet the tensor as fp32 scalars)"""
    step = grid_radius * 2 / S
    half = torch.tensor(0.5 * step, dtype=torch.float32)
    last = grid_radius - step / 2          # centre of the outermost cell

    def centre(n):
        cell = torch.floor(n.clamp(-grid_radius, grid_radius) / step + TINY)
        return ((cell + 0.5) * step).clamp(-last, last)

    def index(c):
        i = torch.floor(c / step + TINY) + S / 2
        return torch.where(torch.isnan(i), torch.zeros_like(i), i).long().clamp(0, S - 1)   # (a NaN coordinate: cell 0, fraction NaN)
    lo, hi = centre(p - half), centre(p + half)
    return index(lo), index(hi), (p - lo) / step


def cells(pts, S, grid_radius=GRID_RADIUS):
    """pts [N,3] fp32 -> ids [N,8,3] int64 (corner u takes the upper cell on axis i when bit i of u is set) and xyz [N,3] fp32"""
    assert pts.dtype == torch.float32 and pts.dim() == 2 and pts.shape[1] == 3 and S % 2 == 0
    per_axis = [axis_cells(pts[:, i].contiguous(), S, grid_radius) for i in range(3)]
    ids = torch.stack([torch.stack([per_axis[i][bit_i(u, i)] for i in range(3)], dim=-1) for u in range(8)], dim=1)
    xyz = torch.stack([per_axis[i][2] for i in range(3)], dim=-1)
    assert xyz.dtype == torch.float32
    return ids, xyz


def weights_of(xyz):
    """trilinear_weights (src/nerf.py:363-369) in fp64 from the fp32 xyz: [N,8]; NaN rows where xyz is not finite"""
    x = xyz.double()
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    pick = lambda v, pos: v if pos else 1 - v
    return torch.stack([pick(x[:, 0], bit_i(u, 0)) * pick(x[:, 1], bit_i(u, 1)) * pick(x[:, 2], bit_i(u, 2)) for u in range(8)], dim=-1)


def rows_of(ids, S):
    return (ids[..., 0] * S + ids[..., 1]) * S + ids[..., 2]


def sample_ref(pts, densities, rgb, grid_radius=GRID_RADIUS):
    """pts [N,3] fp32, densities [S,S,S,1], rgb [S,S,S,C] -> raw [N, 1 + C] fp64 = [density | colour parameters] and mag [N, 1 + C] =
    sum over the corners of |w_c| |v_c|"""
    S = densities.shape[0]
    ids, xyz = cells(pts, S, grid_radius)
    w = weights_of(xyz)                                                      # [N,8]
    grid = torch.cat([densities, rgb], dim=-1).double().reshape(S ** 3, -1)  # [S^3, 1 + C]
    v = grid[rows_of(ids, S)]                                                # [N,8,1+C]
    raw = (w[..., None] * v).sum(dim=1)
    mag = (w[..., None] * v).abs().sum(dim=1)
    return raw, mag


def sample_bound(mag):
    return SAMPLE_C * U * mag


def scatter_ref(pts, g_raw, S, grid_radius=GRID_RADIUS):
    """pts [N,3] fp32, g_raw [N, 1 + C] -> ref, mag, cnt [S^3, 1 + C] fp64: the gradient of the grid (column 0: densities), sum |addend|
    per entry, addends per entry"""
    ids, xyz = cells(pts, S, grid_radius)
    w = weights_of(xyz)
    rows = rows_of(ids, S)
    g = g_raw.double().reshape(pts.shape[0], -1)
    ref = torch.zeros(S ** 3, g.shape[1], dtype=torch.float64)
    mag, cnt = torch.zeros_like(ref), torch.zeros_like(ref)
    ones = torch.ones_like(g)
    for u in range(8):
        a = w[:, u, None] * g
        ref.index_add_(0, rows[:, u], a)
        mag.index_add_(0, rows[:, u], a.abs())
        cnt.index_add_(0, rows[:, u], ones)
    return ref, mag, cnt


def scatter_bound(ref, mag, cnt, det):
    """the per-entry bound of the module docstring; the additive constant lives HERE and nowhere else"""
    b = (cnt + SCATTER_C0) * U * mag
    if det:
        b = b + cnt * 2.0 ** -40 + U * ref.abs()
    return b


def worst_ratio(got, ref, bound):
    """max over ALL entries of |got - ref| / bound (bound 0: the entry must be exact -- ratio 0 or inf); NaN where the two disagree about
    NaN, entries that are NaN in both count as equal"""
    got = got.detach().cpu().double().reshape(ref.shape)
    both_nan = torch.isnan(got) & torch.isnan(ref)
    if bool((torch.isnan(got) != torch.isnan(ref)).any()):
        return float("nan")
    err = torch.where(both_nan, torch.zeros_like(ref), (got - ref).abs())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(ratio.max()) if ratio.numel() else 0.0


def composite_ref(raw, ts, rays, act, bg, rand=None):
    """fp64 compositing (the oracle's restatement of src/nerf.py:60-103) of raw [T, *batch, 4] samples over rays [*batch, 6]:
    out [*batch, 3], alpha, weights [T, *batch]"""
    T, batch = raw.shape[0], tuple(rays.shape[:-1])
    raw = raw.double().reshape(T, 1, 1, -1, 4)
    r_d = rays[..., 3:].double().reshape(1, 1, -1, 3)
    alpha, weights = O.alpha_from_density(raw[..., 0], ts.double(), r_d)
    out = O.volumetric_integrate(weights, O.sigmoid(act)(raw[..., 1:]))
    if bg == "white":
        out = out + O.sky_white(weights)
    elif bg == "random":
        out = out + O.sky_random(weights, rand.double().reshape(1, 1, -1, 1))
    return out.reshape(batch + (3,)), alpha.reshape((T,) + batch), weights.reshape((T,) + batch)


def model_ref(g, route_pts=None):
    """(out, alpha, weights) in fp64 of a g23 fixture's case by this file's lookup + composite_ref: positions o + t d formed in fp32"""
    from conftest import golden_params
    p = golden_params(g)
    rays, ts = g["rays"], g["ts"]
    pts = pts_of(rays, ts)
    raw, _ = sample_ref(pts.reshape(-1, 3), p["densities"], p["rgb"], float(g["grid_radius"]))
    return composite_ref(raw.reshape(pts.shape[:-1] + (4,)), ts, rays, str(g["act"]), str(g["bg"]))


# ------------------------------------------------------------------------------------------------------------ inputs
def grid_values(S, seed=4200, C=3):
    """(densities [S,S,S,1], rgb [S,S,S,C]) uniform in +-1"""
    return _t(proc_uniform((S, S, S, 1), seed, 1.0)), _t(proc_uniform((S, S, S, C), seed + 1, 1.0))


def index_grid(S):
    """a grid whose entries encode their own index with exact small integers (row % 251 + 1 in the density, three other residues in the
    colours): a wrong cell is an error of order 1, not of order u"""
    r = np.arange(S ** 3, dtype=np.int64)
    den = ((r % 251) + 1).astype(np.float32).reshape(S, S, S, 1)
    rgb = np.stack([(r % 241) + 1, (r % 239) + 1, (r % 233) + 1], axis=-1).astype(np.float32).reshape(S, S, S, 3)
    return _t(den), _t(rgb)


def uniform_points(n, seed=4300, amp=2.5):
    """(i) uniform in +-2.5: the inside of the grid and the extrapolated region"""
    return _t(proc_uniform((n, 3), seed + n, amp))


def lattice_points(S, grid_radius=GRID_RADIUS, n=256, seed=4400):
    """(ii) the lattice set: per axis k voxel_len and (k + 0.5) voxel_len for k in [-S/2 - 1, S/2 + 1] (products formed in double, cast
    to fp32), `n` seeded combinations, plus the 8 corners +-grid_radius and the origin"""
    voxel_len = grid_radius * 2 / S
    k = np.arange(-S // 2 - 1, S // 2 + 2, dtype=np.float64)
    vals = np.concatenate([k * voxel_len, (k + 0.5) * voxel_len])
    pick = ((proc_uniform((n, 3), seed + S, 0.5) + 0.5) * len(vals)).astype(np.int64).clip(0, len(vals) - 1)
    corners = np.array([[(2 * bit_i(u, i) - 1) * grid_radius for i in range(3)] for u in range(8)], dtype=np.float64)
    return _t(np.concatenate([vals[pick], corners, np.zeros((1, 3))]).astype(np.float32))


def zero_points():
    """(iii) +-1e-11 and +-1e-4 around zero per axis (all 64 combinations): tiny coordinates of both signs.  (The reference's 1e-10 is
    added to n / voxel_len with n = p -+ voxel_len / 2; it could move a floor only for -1e-10 <= n / voxel_len < 0, and the fp32
    difference p - h is 0 or at least an ulp of h away from 0, so at these points -- n = -+h -- and everywhere else it is absorbed.
    The kernels keep the add; this set pins that a tiny coordinate of either sign lands in the cell pair (S/2 - 1, S/2).)"""
    v = np.array([-1e-4, -1e-11, 1e-11, 1e-4], dtype=np.float64)
    i = np.arange(64)
    return _t(np.stack([v[i & 3], v[(i >> 2) & 3], v[(i >> 4) & 3]], axis=-1).astype(np.float32))


def generic_rays(shape, seed=4500):
    """seeded origins on the radius-4 sphere, directions towards the origin with jitter 0.3, normalised: with near 2 / far 6 the first
    samples of every ray lie outside the grid"""
    o = proc_uniform(tuple(shape) + (3,), seed, 1.0).astype(np.float64)
    o = 4.0 * o / np.linalg.norm(o, axis=-1, keepdims=True)
    d = -o / 4.0 + 0.3 * proc_uniform(tuple(shape) + (3,), seed + 1, 1.0)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return _t(np.concatenate([o, d], axis=-1).astype(np.float32))


def pts_of(rays, ts):
    """o + t d as na_compute_pts (and torch) form it in fp32: a multiply, then an add; [T, ..., 3]"""
    return rays[..., :3].unsqueeze(0) + ts.reshape((-1,) + (1,) * (rays.dim() - 1) + (1,)) * rays[..., 3:].unsqueeze(0)


SCATTER_S = 16


def scatter_case(name):
    """(pts [N,3], g_raw [N,4], S, grid_radius) of a named scatter input:
      A      one cell hit by 256 copies of a point, gradient rows (n % 64) + 1
      B      face straddle: 40 points in one cell, 24 in its neighbour across the x face, interleaved
      D<n>   ragged sizes, uniform in +-2.5
      F      F_N samples: a workgroup takes a second round
      L      the lattice set
      G      exact arithmetic: S = 4, grid_radius 1 (voxel_len 0.5), points on multiples of 1/8 in [-0.75, 1] -- xyz multiples of 1/4,
             weights of 1/64 in [0, 1] -- and integer gradients |g| <= 8: every sum of the 4096 samples is exact in fp32 (< 2^15 with 6
             fractional bits) and in 2^-40 fixed point, in any order"""
    S, gr = SCATTER_S, GRID_RADIUS
    vl = gr * 2 / S
    if name == "A":
        p = (np.array([[2.5, -3.5, 0.5]]) * vl + proc_uniform((1, 3), 4601, 0.2 * vl)).astype(np.float32)
        return _t(np.repeat(p, 256, axis=0)), _t(np.repeat(((np.arange(256) % 64) + 1).astype(np.float32)[:, None], 4, axis=1)), S, gr
    if name == "B":
        c = np.concatenate([np.repeat([[-1.0, 2.0, 3.0]], 40, 0), np.repeat([[0.0, 2.0, 3.0]], 24, 0)]) * vl
        order = np.argsort(proc_uniform((64,), 4603, 1.0), kind="stable")
        return _t((c + proc_uniform((64, 3), 4602, 0.05 * vl)).astype(np.float32)[order]), _t(proc_uniform((64, 4), 4604, 1.0)), S, gr
    if name[0] == "D":
        n = int(name[1:])
        return uniform_points(n, 4610), _t(proc_uniform((n, 4), 4620 + n, 1.0)), S, gr
    if name == "F":
        return _t(proc_uniform((F_N, 3), 4640, 1.5)), _t(proc_uniform((F_N, 4), 4641, 1.0)), S, gr
    if name == "L":
        p = lattice_points(S, gr)
        return p, _t(proc_uniform((p.shape[0], 4), 4650, 1.0)), S, gr
    if name == "G":
        k = (proc_uniform((4096, 3), 4660, 7.5) + 7.5).astype(np.int64).clip(0, 14) - 6   # -6 .. 8: below -0.75 the lower border extrapolates
        return _t((k.astype(np.float64) / 8.0).astype(np.float32)), _t(np.rint(proc_uniform((4096, 4), 4661, 8.0)).astype(np.float32)), 4, 1.0
    raise KeyError(name)


D_SIZES = (1, 63, 65, 257, 1000)
SCATTER_CASES = ("A", "B") + tuple(f"D{n}" for n in D_SIZES) + ("F", "L", "G")


@functools.lru_cache(maxsize=None)
def scatter_reference(name):
    """scatter_ref of a named input, computed once per process and shared (callers must not modify it)"""
    p, g, S, gr = scatter_case(name)
    return scatter_ref(p, g, S, gr)
