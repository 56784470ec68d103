"""Plain reference of NeRFVoxel's lookup with the per-voxel pos-linear-view head (csrc/voxel.hip; src/refl.py:265-280 over
src/nerf.py:493-524 of the reference), its scatter, its position gradient and the model, with the error bounds the tests hold the
kernels to.  Imported by tests/test_voxel_plv_ref.py (CPU) and the GPU tests of the head.

Built on tests/voxel_ref.py: cells and xyz are its fp32 chain (cell membership is part of the operator's definition), everything
behind xyz is fp64 here -- the weights, the basis Y_k of the fp32 direction, the products and the sums.  The grid row is
[raw rgb (3) | NK = (K+1)^2 coefficients]; per sample
    raw = [density | 3 colour parameters] (voxel_ref.sample_ref on the leading columns),   s = sum_u w_u sum_k Y_k v_uk.

THE ASSOCIATION of the kernels (csrc/voxel_plv.h): per corner d_u = Y_0 v_u0, then d_u = fma(Y_k, v_uk, d_u) for k = 1 .. NK-1 (NK
roundings), then s = s + w_u * d_u over the corners in order (a product and a sum each).

THE BOUNDS (derived, first order in u = 2^-24, never tuned).  All are relative to a sum of absolute addends, never to the result:
extrapolated samples have sign-alternating weights.  For the SH sum the magnitude is
    mag_s = sum_u sum_k |w_u| Yabs_k |v_uk|,
where Yabs_k >= |Y_k| is Y_k's closed form with every monomial taken in absolute value (YABS below): the fp32 evaluation error of
a basis function that vanishes by cancellation (x^2 - y^2 on a diagonal, 35 z^4 - 30 z^2 + 3 on a cone) is relative to its terms,
not to its value, so a bound relative to |Y_k| alone cannot hold there.  Off those cancellations Yabs_k and |Y_k| are of one size.
  basis      |Y_k(fp32) - Y_k| <= BASIS_C u Yabs_k, BASIS_C = 28: a normalised coordinate carries 4 u (three squares and two sums under
             the root: 3 u, halved by the root, plus the root's and the division's rounding), a monomial of degree <= 4 therefore 16 u,
             the closed forms add at most 10 roundings (products, sums, the fp32 constant), and 2 u covers the second order
  gather s   |got - ref| <= (SH_C0 + NK) u mag_s, SH_C0 = 42: BASIS_C for Y_k, 5 u for w_u (three 1 - x, two products), NK u for the
             fma chain of a corner (each partial sum is bounded by the corner's sum of magnitudes), 1 u for w_u * d_u, 7 u for the sum
             over 8 corners, 1 u for the second order: 28 + 5 + 1 + 7 + 1 = 42.  The four leading outputs are vox_gather's arithmetic
             and keep voxel_ref.sample_bound.
  scatter    SH block, entry (row, 3 + k): the addend is (w_u * g_sh) * Y_k -- 5 u for w_u, one product, one more product, BASIS_C
             for Y_k: 35 u -- and any summation order of cnt addends adds (cnt - 1) u:  (cnt + SH_SCATTER_C0) u mag with SH_SCATTER_C0 =
             35 and mag = sum |w_u g_sh| Yabs_k; the deterministic mode adds cnt 2^-40 + u |ref| like voxel_ref.scatter_bound.  The
             four leading columns keep voxel_ref.scatter_bound.
  positions  g_pts[n, a] = (1 / voxel_len) sum_u (dw_u / da) val_u,  val_u = g_d den_u + sum_c g_c rgb_uc + g_sh d_u:
             |got - ref| <= PTS_C(NK) u (1 / voxel_len) sum_u |dw_u / da| valmag_u, valmag_u the same sum with every term in absolute
             value and Yabs for Y.  PTS_C = 45 + NK: BASIS_C + NK for d_u as above, 1 for g_sh * d_u, 4 for the sum of the five terms
             (their own products are covered by the 1 + NK of the chain being the longest), 3 for dw_u (two 1 - x, a product), 1 for
             the product with val_u, 7 for the corner sum, 1 for the division by voxel_len: 28 + NK + 1 + 4 + 3 + 1 + 7 + 1 = 45 + NK.
An entry with bound 0 must be exact.
"""
import numpy as np
import torch

import voxel_ref as V
from oracle.procedural import proc_uniform

U = V.U
BASIS_C = 28.0
SH_C0 = 42.0
SH_SCATTER_C0 = 35.0
ORDERS = (0, 1, 2, 3, 4)


def nk(order):
    return (order + 1) ** 2


def channels(order):
    return 3 + nk(order)


# closed forms of the real spherical harmonics of degrees 0 .. 4 in the reference's sign convention (src/spherical_harmonics.py:55-106:
# the m < 0 and odd-m terms carry a minus), as (coefficient, [monomials (factor, ex, ey, ez)]) so that Y and Yabs share one table
_P = np.pi
_SH = [
    (0.5 / np.sqrt(_P), [(1, 0, 0, 0)]),
    (-np.sqrt(3 / (4 * _P)), [(1, 0, 1, 0)]),
    (np.sqrt(3 / (4 * _P)), [(1, 0, 0, 1)]),
    (-np.sqrt(3 / (4 * _P)), [(1, 1, 0, 0)]),
    (np.sqrt(15 / _P) / 2, [(1, 1, 1, 0)]),
    (-np.sqrt(15 / _P) / 2, [(1, 0, 1, 1)]),
    (np.sqrt(5 / _P) / 4, [(2, 0, 0, 2), (-1, 2, 0, 0), (-1, 0, 2, 0)]),
    (-np.sqrt(15 / _P) / 2, [(1, 1, 0, 1)]),
    (np.sqrt(15 / _P) / 4, [(1, 2, 0, 0), (-1, 0, 2, 0)]),
    (-np.sqrt(35 / (2 * _P)) / 4, [(3, 2, 1, 0), (-1, 0, 3, 0)]),
    (np.sqrt(105 / _P) / 2, [(1, 1, 1, 1)]),
    (-np.sqrt(21 / (2 * _P)) / 4, [(4, 0, 1, 2), (-1, 2, 1, 0), (-1, 0, 3, 0)]),
    (np.sqrt(7 / _P) / 4, [(2, 0, 0, 3), (-3, 2, 0, 1), (-3, 0, 2, 1)]),
    (-np.sqrt(21 / (2 * _P)) / 4, [(4, 1, 0, 2), (-1, 3, 0, 0), (-1, 1, 2, 0)]),
    (np.sqrt(105 / _P) / 4, [(1, 2, 0, 1), (-1, 0, 2, 1)]),
    (-np.sqrt(35 / (2 * _P)) / 4, [(1, 3, 0, 0), (-3, 1, 2, 0)]),
    (3 * np.sqrt(35 / _P) / 4, [(1, 3, 1, 0), (-1, 1, 3, 0)]),
    (-3 * np.sqrt(35 / (2 * _P)) / 4, [(3, 2, 1, 1), (-1, 0, 3, 1)]),
    (3 * np.sqrt(5 / _P) / 4, [(7, 1, 1, 2), (-1, 1, 1, 0)]),
    (-3 * np.sqrt(5 / (2 * _P)) / 4, [(7, 0, 1, 3), (-3, 0, 1, 1)]),
    (3 / (16 * np.sqrt(_P)), [(35, 0, 0, 4), (-30, 0, 0, 2), (3, 0, 0, 0)]),
    (-3 * np.sqrt(5 / (2 * _P)) / 4, [(7, 1, 0, 3), (-3, 1, 0, 1)]),
    (3 * np.sqrt(5 / _P) / 8, [(7, 2, 0, 2), (-1, 2, 0, 0), (-7, 0, 2, 2), (1, 0, 2, 0)]),
    (-3 * np.sqrt(35 / (2 * _P)) / 4, [(1, 3, 0, 1), (-3, 1, 2, 1)]),
    (3 * np.sqrt(35 / _P) / 16, [(1, 4, 0, 0), (-6, 2, 2, 0), (1, 0, 4, 0)]),
]


def basis(dirs, order):
    """dirs [R,3] fp32 (un-normalised) -> (Y, Yabs) [R, NK] fp64 at F.normalize(dirs, eps 1e-12) formed in fp64 from the fp32 values"""
    d = dirs.double()
    d = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y, Ya = [], []
    for c, terms in _SH[:nk(order)]:
        mono = [f * x ** ex * y ** ey * z ** ez for f, ex, ey, ez in terms]
        Y.append(c * sum(mono))
        Ya.append(abs(c) * sum(m.abs() for m in mono))
    return torch.stack(Y, dim=-1), torch.stack(Ya, dim=-1)


def _ray_rows(n, R):
    return torch.arange(n) % R


# ------------------------------------------------------------------------------------------------------------ the lookup
def sample_ref(pts, dirs, densities, rgb, grid_radius=V.GRID_RADIUS):
    """pts [N,3] fp32 (sample n belongs to ray n % R), dirs [R,3] fp32, densities [S,S,S,1], rgb [S,S,S, 3 + NK] ->
    raw [N,4], mag [N,4] (voxel_ref.sample_ref on the leading columns), s [N], mag_s [N]; all fp64"""
    S, C = densities.shape[0], rgb.shape[-1]
    order = int(round((C - 3) ** 0.5)) - 1
    assert channels(order) == C, C
    raw, mag = V.sample_ref(pts, densities, rgb[..., :3].contiguous(), grid_radius)
    ids, xyz = V.cells(pts, S, grid_radius)
    w = V.weights_of(xyz)                                             # [N,8]
    co = rgb.double().reshape(S ** 3, C)[:, 3:][V.rows_of(ids, S)]   # [N,8,NK]
    Y, Ya = basis(dirs, order)
    r = _ray_rows(pts.shape[0], dirs.shape[0])
    s = (w[..., None] * Y[r][:, None, :] * co).sum(dim=(1, 2))
    mag_s = (w[..., None].abs() * Ya[r][:, None, :] * co.abs()).sum(dim=(1, 2))
    return raw, mag, s, mag_s


def sh_bound(mag_s, order):
    return (SH_C0 + nk(order)) * U * mag_s


def scatter_ref(pts, dirs, g_raw, g_sh, S, order, grid_radius=V.GRID_RADIUS):
    """-> ref, mag, cnt [S^3, 1 + C] fp64: column 0 densities, 1..3 raw rgb, 4.. the coefficients"""
    lead = V.scatter_ref(pts, g_raw, S, grid_radius)
    ids, xyz = V.cells(pts, S, grid_radius)
    w = V.weights_of(xyz)
    rows = V.rows_of(ids, S)
    Y, Ya = basis(dirs, order)
    r = _ray_rows(pts.shape[0], dirs.shape[0])
    gs = g_sh.double().reshape(-1, 1)
    ref = torch.zeros(S ** 3, nk(order), dtype=torch.float64)
    mag, cnt = torch.zeros_like(ref), torch.zeros_like(ref)
    for u in range(8):
        a = w[:, u, None] * gs
        ref.index_add_(0, rows[:, u], a * Y[r])
        mag.index_add_(0, rows[:, u], a.abs() * Ya[r])
        cnt.index_add_(0, rows[:, u], torch.ones_like(Y[r]))
    return tuple(torch.cat([l, t], dim=-1) for l, t in zip(lead, (ref, mag, cnt)))


def scatter_bound(ref, mag, cnt, det):
    lead = V.scatter_bound(ref[:, :4], mag[:, :4], cnt[:, :4], det)
    b = (cnt[:, 4:] + SH_SCATTER_C0) * U * mag[:, 4:]
    if det:
        b = b + cnt[:, 4:] * 2.0 ** -40 + U * ref[:, 4:].abs()
    return torch.cat([lead, b], dim=-1)


def pts_grad_ref(pts, dirs, densities, rgb, g_raw, g_sh, grid_radius=V.GRID_RADIUS):
    """-> g_pts [N,3], bound [N,3] fp64: the derivative of the cell's polynomial (only xyz depends on the position)"""
    S, C = densities.shape[0], rgb.shape[-1]
    order = int(round((C - 3) ** 0.5)) - 1
    vl = grid_radius * 2 / S
    ids, xyz = V.cells(pts, S, grid_radius)
    x = xyz.double()
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    rows = V.rows_of(ids, S)
    grid = torch.cat([densities, rgb], dim=-1).double().reshape(S ** 3, 1 + C)[rows]   # [N,8,1+C]
    Y, Ya = basis(dirs, order)
    r = _ray_rows(pts.shape[0], dirs.shape[0])
    g4, gs = g_raw.double().reshape(-1, 1, 4), g_sh.double().reshape(-1, 1)
    val = (g4 * grid[..., :4]).sum(-1) + gs * (Y[r][:, None, :] * grid[..., 4:]).sum(-1)                  # [N,8]
    vmag = (g4 * grid[..., :4]).abs().sum(-1) + gs.abs() * (Ya[r][:, None, :] * grid[..., 4:].abs()).sum(-1)
    out, bound = [], []
    for a in range(3):
        o = [b for b in range(3) if b != a]
        dw = torch.stack([(1.0 if V.bit_i(u, a) else -1.0)
                          * (x[:, o[0]] if V.bit_i(u, o[0]) else 1 - x[:, o[0]]) * (x[:, o[1]] if V.bit_i(u, o[1]) else 1 - x[:, o[1]])
                          for u in range(8)], dim=-1)
        out.append((dw * val).sum(-1) / vl)
        bound.append((45.0 + nk(order)) * U * (dw.abs() * vmag).sum(-1) / vl)
    return torch.stack(out, dim=-1), torch.stack(bound, dim=-1)


def head_ref(raw, s, act):
    """[density | act(raw rgb) * (sigmoid(s) / 2 + 0.5)] as raw-shaped rows whose colours are FINAL (composite_final)"""
    import oracle as O
    col = O.sigmoid(act)(raw[..., 1:]) * (torch.sigmoid(s)[..., None] / 2 + 0.5)
    return torch.cat([raw[..., :1], col], dim=-1)


def composite_final(rows, ts, rays, bg, rand=None):
    """voxel_ref.composite_ref for rows [T, *batch, 4] = [density | final colours]: no activation in front of the integral"""
    import oracle as O
    T, batch = rows.shape[0], tuple(rays.shape[:-1])
    rows = rows.double().reshape(T, 1, 1, -1, 4)
    r_d = rays[..., 3:].double().reshape(1, 1, -1, 3)
    alpha, weights = O.alpha_from_density(rows[..., 0], ts.double(), r_d)
    out = O.volumetric_integrate(weights, rows[..., 1:])
    if bg == "white":
        out = out + O.sky_white(weights)
    elif bg == "random":
        out = out + O.sky_random(weights, rand.double().reshape(1, 1, -1, 1))
    return out.reshape(batch + (3,)), alpha.reshape((T,) + batch), weights.reshape((T,) + batch)


def render_ref(rays, ts, densities, rgb, act, bg, rand=None, pts=None, grid_radius=V.GRID_RADIUS):
    """fp64 (out, alpha, weights) of the model: positions o + t d in fp32 (or explicit pts [T, ..., 3]), this file's lookup and head,
    composite_final"""
    if pts is None:
        pts = V.pts_of(rays, ts)
    raw, _, s, _ = sample_ref(pts.reshape(-1, 3), rays[..., 3:].reshape(-1, 3), densities, rgb, grid_radius)
    rows = head_ref(raw, s, act).reshape(pts.shape[:-1] + (4,))
    return composite_final(rows, ts, rays, bg, rand)


def model_ref(g):
    """(out, alpha, weights) in fp64 of a g27 fixture's case"""
    from conftest import golden_params
    p = golden_params(g)
    return render_ref(g["rays"], g["ts"], p["densities"], p["rgb"], str(g["act"]), str(g["bg"]), grid_radius=float(g["grid_radius"]))


# ------------------------------------------------------------------------------------------------------------ inputs
def grid_values(S, order, seed=4800):
    """(densities [S,S,S,1], rgb [S,S,S, 3 + NK]) uniform in +-1"""
    return V.grid_values(S, seed, channels(order))


def directions(R, seed=4810):
    """[R,3] un-normalised directions of lengths 0.2 .. 3; row 0 is the zero direction when R > 2 (F.normalize's eps: the basis at
    (0, 0, 0)) and row 1 an axis (most basis functions vanish there)"""
    d = proc_uniform((R, 3), seed + R, 1.0).astype(np.float64)
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * (1.6 + 1.4 * proc_uniform((R, 1), seed + R + 1, 1.0))
    if R > 2:
        d[0] = 0.0
        d[1] = (0.0, 0.0, 2.0)
    return torch.from_numpy(d.astype(np.float32))


def rays_of(dirs, seed=4820):
    """rays [R,6]: seeded origins in +-1 with the given directions"""
    o = torch.from_numpy(proc_uniform((dirs.shape[0], 3), seed + dirs.shape[0], 1.0))
    return torch.cat([o, dirs], dim=-1).contiguous()


def scatter_inputs(name):
    """voxel_ref.scatter_case(name) with directions and the head's extra gradient: (pts, dirs [R,3], g_raw [N,4], g_sh [N], S, grid_radius).
    R = the first of 7, 5, 3, 1 rays that divides N (sample n belongs to ray n % R).  Case G keeps integer g_sh."""
    p, g, S, gr = V.scatter_case(name)
    N = p.shape[0]
    R = next(r for r in (7, 5, 3, 1) if N % r == 0)
    dirs = directions(R, 4830)
    if R == 1:
        dirs = torch.tensor([[0.3, -1.1, 0.7]])
    g_sh = torch.from_numpy(proc_uniform((N,), 4840 + (N % 1000), 1.0))
    if name == "G":
        g_sh = torch.from_numpy(np.rint(proc_uniform((N,), 4841, 8.0)).astype(np.float32))
    return p, dirs, g, g_sh, S, gr
