"""Plain fp64 restatement of DynamicNeRFVoxel's divergence operators (csrc/dyn_voxel_div.hip; runner.py:694-700 and src/utils.py:461-478
of the reference) with the error bounds the tests hold the kernels to.  Imported by tests/test_dyn_voxel_div_ref.py (CPU) and
tests/test_gpu_dyn_voxel_div.py.

Cell membership and xyz come from voxel_ref.cells (the reference's fp32 chain, part of the operators' definition); everything behind xyz
is fp64 here, voxel_len being its fp32 image.  With w_u the trilinear weights of corner u, s_ui = +1 / -1 by bit i of u:
    d_u = v . grad w_u = (v_x s_ux wy wz + v_y wx s_uy wz + v_z wx wy s_uz) / vl         dabs_u = the same sum of ABSOLUTE values
    J_dp v    = sum_k B_k(t) sum_u d_u c_{u,k}
    J_rigid v = s (J_dp v) + dp (s (1 - s)) sum_u d_u r_u,    s = sigmoid(sum_u w_u r_u),   dp = sum_k B_k sum_u w_u c_{u,k}
    value     = v . (J v)

THE BOUNDS (derived from the kernel's order of operations, not tuned; first order in u = 2^-24; every `mag` is a sum of absolute values
of the summed terms, never |result|: outside the grid the weights alternate in sign and grow polynomially).
  d_u      a term v_a (+-)(w w'): 1 - x twice, the product, times v_a: 4 roundings; the sum of three terms 2; the division 1:
               |d_u - ref| <= D_C u dabs_u,  D_C = 7
  tangent  tc_ka = sum_u d_u c_uka in corner order: d_u's D_C, the product 1, eight addends 7, second order 1:
               TAN_C u magt_ka,  TAN_C = 16,  magt_ka = sum_u dabs_u |c_uka|            (likewise trl = sum_u d_u r_u: TAN_C u magtl)
  spline   dyn_voxel_ref's count, 3 (n - 1) + 2 on top:  |j_a - ref| <= JQ_C(n) u magj_a,  JQ_C = TAN_C + 3 (n - 1) + 2,
               magj_a = sum_k B_k magt_ka
  dp form  value = (v_x j_x + v_y j_y) + v_z j_z: a product and two adds:   bound = (JQ_C(n) + 3) u sum_a |v_a| magj_a
  rigid    s and dp carry dyn_voxel_ref.warp_ref's bounds b_s, b_dp.  ss = s (1 - s): |d ss / d s| <= 1 and two roundings:
               b_ss = b_s + 2 u ss;    ds = ss trl: b_ds = b_ss magtl + (TAN_C + 1) u ss magtl
           j'_a = s j_a + dp_a ds, M_a = |s| magj_a + magdp_a ss magtl its magnitude (two products, one add; 2 u second order):
               b_j'_a = |s| b_j_a + b_s magj_a + b_dp_a ss magtl + magdp_a b_ds + 5 u M_a
               bound = sum_a |v_a| (b_j'_a + 3 u M_a)
  scatter  entry (row_u, 3 (k - 1) + a) sums d_u ((g B_k) v_a): d_u D_C, B_k at most 3 (n - 1) + 1, three products: C0 = 3 (n - 1) + 11;
           any summation order of cnt addends adds (cnt - 1) u mag, mag = sum dabs_u |g| B_k |v_a|:
               |got - ref| <= (cnt + C0) u mag  +  [deterministic mode]  (cnt 2^-40 + u |ref|)
  xyz      NOT part of a kernel's bound (kernel and restatement share the fp32 xyz).  Against the reference's own fp64 run the fp32 xyz
           itself is off: the centre fl((k + 0.5) fl(vl)) by 2 u |centre|, p - centre and the division by a rounding each and fl(vl) by
           u: dx <= u (3 |x| + 2 |centre| / vl) <= u (3 |x| + S + 1).  `b_xyz` = sum_i |d value / d x_i| dx_i (the derivative by
           autograd through this file's fp64 arithmetic; per scatter addend analytically), plus u |value| for the factor 1 / fl(vl).
           Only comparisons with a g29 fixture add it.
An entry with bound 0 must be exact.
"""
import numpy as np
import torch

import dyn_voxel_ref as DV
import voxel_ref as V

U = V.U
D_C = 7.0
TAN_C = 16.0


def jq_c(n):
    return TAN_C + 3.0 * (n - 1) + 2.0


def scatter_c0(n):
    return 3.0 * (n - 1) + 11.0


def _sign(u, i):
    return 1.0 if V.bit_i(u, i) else -1.0


def _factors(x):
    """per corner u and axis i the factor of the trilinear weight, [N,8,3], from xyz [N,3] fp64 (NaN rows where xyz is not finite)"""
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    return torch.stack([torch.stack([x[:, i] if V.bit_i(u, i) else 1 - x[:, i] for i in range(3)], dim=-1) for u in range(8)], dim=1)


def dweights(x, v, vl):
    """(w [N,8], d [N,8], dabs [N,8]) of the module docstring from xyz [N,3] fp64 and v [N,3] fp64"""
    f = _factors(x)
    w = f[..., 0] * f[..., 1] * f[..., 2]
    sg = torch.tensor([[_sign(u, i) for i in range(3)] for u in range(8)], dtype=torch.float64)
    prod = torch.stack([f[..., 1] * f[..., 2], f[..., 0] * f[..., 2], f[..., 0] * f[..., 1]], dim=-1)   # [N,8,3]
    terms = v[:, None, :] * sg[None] * prod
    return w, terms.sum(-1) / vl, terms.abs().sum(-1) / vl


def _direction(v, pts):
    return torch.ones(pts.shape, dtype=torch.float64) if v is None else v.double().reshape(pts.shape)


def _value(x, v, t, cv, rv, n, vl):
    """the value and every magnitude of the module docstring as differentiable fp64 functions of xyz"""
    w, d, dabs = dweights(x, v, vl)
    B = DV.bernstein(t, n)[:, 1:, None]
    tc, magt = (d[..., None, None] * cv).sum(1), (dabs[..., None, None] * cv.abs()).sum(1)   # [N,n-1,3]
    j, magj = (B * tc).sum(1), (B * magt).sum(1)                                             # [N,3]
    if rv is None:
        return (v * j).sum(-1), dict(magj=magj)
    cp, magc = (w[..., None, None] * cv).sum(1), (w[..., None, None] * cv).abs().sum(1)
    dp, magdp = (B * cp).sum(1), (B * magc).sum(1)
    logit, magl = (w * rv).sum(1), (w * rv).abs().sum(1)
    trl, magtl = (d * rv).sum(1), (dabs * rv.abs()).sum(1)
    s = torch.sigmoid(logit)
    ss = s * (1 - s)
    jr = s[:, None] * j + dp * (ss * trl)[:, None]
    return (v * jr).sum(-1), dict(magj=magj, magdp=magdp, magl=magl, magtl=magtl, s=s, ss=ss)


def jac_quad_ref(pts, t, ctrl, rig, spline, grid_radius=V.GRID_RADIUS, v=None):
    """pts [N,3] fp32, t [N], ctrl [S,S,S,3(n-1)], rig [S,S,S,1] or None (the dp form), v [N,3] or None (ones) -> dict of fp64 [N]:
    value, bound (the kernel's) and b_xyz (module docstring)"""
    S, n = ctrl.shape[0], spline
    ids, xyz = V.cells(pts, S, grid_radius)
    rows = V.rows_of(ids, S)
    vl = float(np.float32(grid_radius * 2 / S))
    vv = _direction(v, pts)
    cv = ctrl.double().reshape(S ** 3, n - 1, 3)[rows]
    rv = None if rig is None else rig.double().reshape(S ** 3)[rows]
    x = xyz.double().requires_grad_(True)
    with torch.enable_grad():
        value, m = _value(x, vv, t.double(), cv, rv, n, vl)
        finite = torch.isfinite(value)
        gx, = torch.autograd.grad(torch.where(finite, value, torch.zeros_like(value)).sum(), x)
    value, x = value.detach(), x.detach()
    m = {k: a.detach() for k, a in m.items()}
    va = vv.abs()
    if rig is None:
        bound = (jq_c(n) + 3) * U * (va * m["magj"]).sum(-1)
    else:
        s, ss, magj, magdp, magtl = m["s"], m["ss"], m["magj"], m["magdp"], m["magtl"]
        b_s = U * (V.SAMPLE_C / 4 * m["magl"] + DV.SIGMOID_C * s.abs())
        b_dp = DV.spline_c(n) * U * magdp
        b_j = jq_c(n) * U * magj
        b_ds = (b_s + 2 * U * ss) * magtl + (TAN_C + 1) * U * ss * magtl
        M = s.abs()[:, None] * magj + magdp * (ss * magtl)[:, None]
        b_jr = s.abs()[:, None] * b_j + b_s[:, None] * magj + b_dp * (ss * magtl)[:, None] + magdp * b_ds[:, None] + 5 * U * M
        bound = (va * (b_jr + 3 * U * M)).sum(-1)
    dx = U * (3 * x.abs() + S + 1)
    b_xyz = (gx.abs() * dx).sum(-1) + U * value.abs()
    nan = torch.full_like(value, float("nan"))
    return dict(value=value, bound=torch.where(finite, bound, nan), b_xyz=torch.where(finite, b_xyz, nan))


def jac_quad_backward_ref(pts, t, S, spline, g, grid_radius=V.GRID_RADIUS, v=None):
    """the dp form's scatter: ref, mag, cnt, xyz [S^3, 3(n-1)] fp64 -- the gradient of sum_n g[n] value[n] w.r.t. ctrl_pts_grid, the sum of
    |addend|, the addends per entry and the entry's share of the fp32 xyz's own error (module docstring)"""
    n, N = spline, pts.shape[0]
    ids, xyz = V.cells(pts, S, grid_radius)
    rows = V.rows_of(ids, S)
    vl = float(np.float32(grid_radius * 2 / S))
    vv = _direction(v, pts)
    x = xyz.double()
    f = _factors(x)
    _, d, dabs = dweights(x, vv, vl)
    # |d d_u / d x_i| <= sum_{j != i} |v_j| |factor of the third axis| / vl
    dd = torch.stack([sum(vv[:, None, j].abs() * f[..., 3 - i - j].abs() for j in range(3) if j != i) for i in range(3)], dim=-1) / vl
    dx = U * (3 * x.abs() + S + 1)
    dxy = (dd * dx[:, None, :]).sum(-1) + U * dabs                                                     # [N,8]
    B = DV.bernstein(t, n)[:, 1:]
    sv = (g.double().reshape(N, 1, 1) * B[:, :, None] * vv[:, None, :]).reshape(N, -1)                 # [N,W]
    ref = torch.zeros(S ** 3, sv.shape[1], dtype=torch.float64)
    mag, cnt, bx = torch.zeros_like(ref), torch.zeros_like(ref), torch.zeros_like(ref)
    ones = torch.ones_like(sv)
    for u in range(8):
        ref.index_add_(0, rows[:, u], d[:, u, None] * sv)
        mag.index_add_(0, rows[:, u], dabs[:, u, None] * sv.abs())
        bx.index_add_(0, rows[:, u], dxy[:, u, None] * sv.abs())
        cnt.index_add_(0, rows[:, u], ones)
    return ref, mag, cnt, bx


def scatter_bound(ref, mag, cnt, spline, det):
    b = (cnt + scatter_c0(spline)) * U * mag
    if det:
        b = b + cnt * 2.0 ** -40 + U * ref.abs()
    return b


# ------------------------------------------------------------------------------------------------------------ inputs
def directions(n, seed=5100):
    """v [n,3]: a seeded stand-in for the normal draw, uniform in +-2"""
    from oracle.procedural import proc_uniform
    return V._t(proc_uniform((n, 3), seed + n, 2.0))


def face_distance(pts, S, grid_radius=V.GRID_RADIUS):
    """per coordinate the distance, in voxel lengths, to the nearest plane on which the cell pair changes (p = (k + 0.5) voxel_len,
    |k + 0.5| <= S / 2 + 0.5; inf beyond the outermost one)"""
    vl = grid_radius * 2 / S
    q = pts.double() / vl - 0.5
    dist = (q - torch.round(q)).abs()
    return torch.where(q.abs() > S / 2 + 1, torch.full_like(dist, float("inf")), dist)


def fixture_case(g):
    """the tensors of a g29 fixture: pts [N,3], t [N], ctrl, rig, spline, grid_radius, e [N,3]"""
    return dict(pts=g["pts"].reshape(-1, 3), t=g["t"].reshape(-1), ctrl=g["ctrl_pts_grid"], rig=g["rigidity_grid"], spline=int(g["spline"]),
                grid_radius=float(g["grid_radius"]), e=g["e"].reshape(-1, 3))
