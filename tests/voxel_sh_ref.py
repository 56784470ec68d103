"""Plain reference of NeRFVoxel's lookup with the per-voxel spherical-harmonic colour head (csrc/voxel.hip; the intended form of
src/refl.py:715-722 over src/nerf.py:493-524 of the reference), its scatter, its position gradient, the head and the model, with the
error bounds the tests hold the kernels to.  Imported by tests/test_voxel_sh_ref.py (CPU) and the GPU tests of the head.

Built on tests/voxel_ref.py (cells and xyz are its fp32 chain: cell membership is part of the operator's definition) and on
voxel_plv_ref.basis / YABS (the basis of the fp32 direction in fp64, and every closed form with its monomials in absolute value); both
are pinned to the reference through the goldens g27 / g28.  Everything behind xyz is fp64 here.  The grid row is 3 channel blocks of
NK = (K+1)^2 coefficients, coefficient k of colour channel c at c NK + k; per sample
    raw = [density | s_0 s_1 s_2],   s_c = sum_u w_u sum_k Y_k v_u[c NK + k],   colour_c = act(s_c).

THE ASSOCIATION of the kernels (csrc/voxel_plv.h, sh_contract_row): per corner and channel d_uc = Y_0 v_u[c NK], then
d_uc = fma(Y_k, v_u[c NK + k], d_uc) for k = 1 .. NK-1 (NK roundings), then s_c = s_c + w_u * d_uc over the corners in order (a product
and a sum each).  It is voxel_plv_ref's association for its one channel, so the counting is the same.

THE BOUNDS (derived as voxel_plv_ref derives its own: first order in u = 2^-24, relative to sums of absolute addends with Yabs, never
tuned).  BASIS_C = 28 is voxel_plv_ref's bound on the fp32 basis, |Y_k(fp32) - Y_k| <= 28 u Yabs_k.
  gather s_c   |got - ref| <= (SH_C0 + NK) u mag_c, mag_c = sum_u sum_k |w_u| Yabs_k |v_u[c NK + k]|, SH_C0 = 42: 28 for Y_k, 5 for w_u
               (three 1 - x, two products), NK for the fma chain of a corner, 1 for w_u * d_uc, 7 for the sum over 8 corners, 1 for the
               second order: 28 + 5 + 1 + 7 + 1 = 42.  The density column is vox_gather's arithmetic and keeps voxel_ref.sample_bound.
  scatter      entry (row, c NK + k): the addend is (w_u * g_c) * Y_k -- 5 u for w_u, one product, one more product, 28 u for Y_k: 35 u
               -- and any summation order of cnt addends adds (cnt - 1) u:  (cnt + SH_SCATTER_C0) u mag, SH_SCATTER_C0 = 35,
               mag = sum |w_u g_c| Yabs_k; the deterministic mode adds cnt 2^-40 + u |ref| like voxel_ref.scatter_bound.  The density
               column keeps voxel_ref.scatter_bound.
  positions    g_pts[n, a] = (1 / voxel_len) sum_u (dw_u / da) val_u,  val_u = g_d den_u + sum_c g_c d_uc:
               |got - ref| <= PTS_C(NK) u (1 / voxel_len) sum_u |dw_u / da| valmag_u, valmag_u the same sum with every term in absolute
               value and Yabs for Y.  PTS_C = 44 + NK: 28 + NK for d_uc as above, 1 for g_c * d_uc, 3 for the sum of the four terms, 3
               for dw_u (two 1 - x, a product), 1 for the product with val_u, 7 for the corner sum, 1 for the division by voxel_len:
               28 + NK + 1 + 3 + 3 + 1 + 7 + 1 = 44 + NK.
An entry with bound 0 must be exact.
"""
import numpy as np
import torch

import voxel_plv_ref as P
import voxel_ref as V
from oracle.procedural import proc_uniform

U = V.U
SH_C0 = P.SH_C0
SH_SCATTER_C0 = P.SH_SCATTER_C0
PTS_C0 = 44.0
ORDERS = P.ORDERS
nk = P.nk


def channels(order):
    return 3 * nk(order)


def _blocks(rgb, order):
    """rgb [S,S,S,3 NK] -> fp64 [S^3, 3, NK]"""
    S = rgb.shape[0]
    assert rgb.shape[-1] == channels(order), (tuple(rgb.shape), order)
    return rgb.double().reshape(S ** 3, 3, nk(order))


def _geometry(pts, dirs, S, order, grid_radius):
    ids, xyz = V.cells(pts, S, grid_radius)
    Y, Ya = P.basis(dirs, order)
    r = torch.arange(pts.shape[0]) % dirs.shape[0]
    return V.weights_of(xyz), V.rows_of(ids, S), xyz, Y[r], Ya[r]


# ------------------------------------------------------------------------------------------------------------ the lookup
def sample_ref(pts, dirs, densities, rgb, order, grid_radius=V.GRID_RADIUS):
    """pts [N,3] fp32 (sample n belongs to ray n % R), dirs [R,3] fp32, densities [S,S,S,1], rgb [S,S,S,3 NK] -> raw [N,4] =
    [density | s_c] and mag [N,4] (column 0: voxel_ref's), fp64"""
    S = densities.shape[0]
    w, rows, _, Y, Ya = _geometry(pts, dirs, S, order, grid_radius)
    den, dmag = V.sample_ref(pts, densities, rgb[..., :3].contiguous(), grid_radius)
    co = _blocks(rgb, order)[rows]                                              # [N,8,3,NK]
    s = (w[:, :, None, None] * Y[:, None, None, :] * co).sum(dim=(1, 3))
    mag = (w[:, :, None, None].abs() * Ya[:, None, None, :] * co.abs()).sum(dim=(1, 3))
    return torch.cat([den[:, :1], s], dim=-1), torch.cat([dmag[:, :1], mag], dim=-1)


def sample_bound(mag, order):
    return torch.cat([V.sample_bound(mag[..., :1]), (SH_C0 + nk(order)) * U * mag[..., 1:]], dim=-1)


def scatter_ref(pts, dirs, g_raw, S, order, grid_radius=V.GRID_RADIUS):
    """-> ref, mag, cnt [S^3, 1 + 3 NK] fp64: column 0 densities, 1 + c NK + k coefficient k of channel c"""
    lead = V.scatter_ref(pts, g_raw, S, grid_radius)
    w, rows, _, Y, Ya = _geometry(pts, dirs, S, order, grid_radius)
    g = g_raw.double().reshape(-1, 4)[:, 1:]
    ref = torch.zeros(S ** 3, 3, nk(order), dtype=torch.float64)
    mag, cnt = torch.zeros_like(ref), torch.zeros_like(ref)
    one = torch.ones(pts.shape[0], 3, nk(order), dtype=torch.float64)
    for u in range(8):
        a = w[:, u, None] * g                                                   # [N,3]
        ref.index_add_(0, rows[:, u], a[:, :, None] * Y[:, None, :])
        mag.index_add_(0, rows[:, u], a.abs()[:, :, None] * Ya[:, None, :])
        cnt.index_add_(0, rows[:, u], one)
    return tuple(torch.cat([l[:, :1], t.reshape(S ** 3, -1)], dim=-1) for l, t in zip(lead, (ref, mag, cnt)))


def scatter_bound(ref, mag, cnt, det):
    lead = V.scatter_bound(ref[:, :1], mag[:, :1], cnt[:, :1], det)
    b = (cnt[:, 1:] + SH_SCATTER_C0) * U * mag[:, 1:]
    if det:
        b = b + cnt[:, 1:] * 2.0 ** -40 + U * ref[:, 1:].abs()
    return torch.cat([lead, b], dim=-1)


def pts_grad_ref(pts, dirs, densities, rgb, g_raw, order, grid_radius=V.GRID_RADIUS):
    """-> g_pts [N,3], bound [N,3] fp64: the derivative of the cell's polynomial (only xyz depends on the position)"""
    S = densities.shape[0]
    vl = grid_radius * 2 / S
    _, rows, xyz, Y, Ya = _geometry(pts, dirs, S, order, grid_radius)
    x = xyz.double()
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    den = densities.double().reshape(S ** 3)[rows]                              # [N,8]
    co = _blocks(rgb, order)[rows]                                              # [N,8,3,NK]
    g4 = g_raw.double().reshape(-1, 1, 4)
    d = (Y[:, None, None, :] * co).sum(-1)                                      # [N,8,3]
    dmag = (Ya[:, None, None, :] * co.abs()).sum(-1)
    val = g4[..., 0] * den + (g4[..., 1:] * d).sum(-1)
    vmag = (g4[..., 0] * den).abs() + (g4[..., 1:].abs() * dmag).sum(-1)
    out, bound = [], []
    for a in range(3):
        o = [b for b in range(3) if b != a]
        dw = torch.stack([(1.0 if V.bit_i(u, a) else -1.0)
                          * (x[:, o[0]] if V.bit_i(u, o[0]) else 1 - x[:, o[0]]) * (x[:, o[1]] if V.bit_i(u, o[1]) else 1 - x[:, o[1]])
                          for u in range(8)], dim=-1)
        out.append((dw * val).sum(-1) / vl)
        bound.append((PTS_C0 + nk(order)) * U * (dw.abs() * vmag).sum(-1) / vl)
    return torch.stack(out, dim=-1), torch.stack(bound, dim=-1)


# ------------------------------------------------------------------------------------------------------------ head and model
def head_ref(raw, act):
    """[density | act(s_c)] as raw-shaped rows whose colours are FINAL (voxel_plv_ref.composite_final)"""
    import oracle as O
    return torch.cat([raw[..., :1], O.sigmoid(act)(raw[..., 1:])], dim=-1)


def render_ref(rays, ts, densities, rgb, order, act, bg, rand=None, pts=None, grid_radius=V.GRID_RADIUS):
    """fp64 (out, alpha, weights) of the model: positions o + t d in fp32 (or explicit pts [T, ..., 3]), this file's lookup and head,
    voxel_plv_ref.composite_final"""
    if pts is None:
        pts = V.pts_of(rays, ts)
    raw, _ = sample_ref(pts.reshape(-1, 3), rays[..., 3:].reshape(-1, 3), densities, rgb, order, grid_radius)
    return P.composite_final(head_ref(raw, act).reshape(pts.shape[:-1] + (4,)), ts, rays, bg, rand)


# ------------------------------------------------------------------------------------------------------------ inputs
def grid_values(S, order, seed=5600):
    """(densities [S,S,S,1], rgb [S,S,S,3 NK]) uniform in +-1"""
    return V.grid_values(S, seed, channels(order))


_Z2 = (30.0 - np.sqrt(480.0)) / 70.0   # a root of 35 z^4 - 30 z^2 + 3 in z^2


def directions(R, seed=5610):
    """voxel_plv_ref.directions (un-normalised; row 0 the zero direction, row 1 an axis when R > 2) with, when R > 4, row 2 on the
    cancellation cone of x^2 - y^2 (|x| = |y|) and row 3 on the one of 35 z^4 - 30 z^2 + 3"""
    d = P.directions(R, seed).clone()
    if R > 4:
        d[2] = torch.tensor([0.7, -0.7, 0.4])
        d[3] = torch.tensor([1.7 * np.sqrt(1.0 - _Z2), 0.0, 1.7 * np.sqrt(_Z2)], dtype=torch.float64).float()
    return d


rays_of = P.rays_of


def scatter_inputs(name):
    """voxel_ref.scatter_case(name) with directions: (pts, dirs [R,3], g_raw [N,4], S, grid_radius), R the first of 7, 5, 3, 1 rays that
    divides N (sample n belongs to ray n % R)"""
    p, g, S, gr = V.scatter_case(name)
    N = p.shape[0]
    R = next(r for r in (7, 5, 3, 1) if N % r == 0)
    dirs = directions(R, 5630) if R > 1 else torch.tensor([[0.3, -1.1, 0.7]])
    return p, dirs, g, S, gr


def grads(n, seed=5640):
    return torch.from_numpy(proc_uniform((n, 4), seed + n, 1.0))
