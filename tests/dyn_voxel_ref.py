"""Plain reference of DynamicNeRFVoxel's three operators (csrc/dyn_voxel.hip, csrc/voxel.hip; src/nerf.py:1526-1586 of the reference) and
the error bounds the tests hold the kernels to.  Imported by tests/test_dyn_voxel_ref.py (CPU) and tests/test_gpu_dyn_voxel.py.

Cell membership and xyz come from voxel_ref.cells (the reference's fp32 chain, part of the operators' definition); everything behind
xyz is fp64 here.  The scalars that meet fp32 tensors in the reference (voxel_len) are their fp32 images.

THE BOUNDS (derived, not tuned; first order in u = voxel_ref.U = 2^-24; `mag` is always a sum of ABSOLUTE values of the addends, never
|result|: outside the grid the weights alternate in sign and grow polynomially).  t is in [0, 1], so the Bernstein weights B_k(t) are
non-negative and sum to 1.

  warp     control point k, axis a: c_ka = sum_u w_u v_u is voxel_ref's gather: SAMPLE_C u mag_ka, mag_ka = sum_u |w_u| |v_u|.
           dp_a = sum_k B_k c_ka.  de_casteljau runs n - 1 levels of b_j <- b_j (1 - t) + b_{j+1} t: per level a term picks up the
           rounding of 1 - t (once), of its product and of the add, 3 u, and every path's weight is non-negative, so the spline adds
           3 (n - 1) u sum_k B_k |c_ka|; cubic_bezier's coefficients carry at most 4 roundings (1 - t, square, times 3, times t or
           1 - t), the product 1 and the sum of four 3: 8 <= 3 (n - 1) + 2 at n = 4.  With 2 u for second order:
               |dp - ref| <= (SAMPLE_C + 3 (n - 1) + 2) u magdp,   magdp_a = sum_k B_k mag_ka   (>= sum_k B_k |c_ka|)
           rigidity r = sigmoid(l), l = the gather of rigidity_grid (SAMPLE_C u mag_l): |sigmoid'| = r (1 - r) <= 1/4 passes 3 u mag_l
           on; exp to 1 ulp (2 u relative, worth at most 2 u r on r), 1 + e and the division one rounding each, 1 u second order:
               |r - ref| <= u (SAMPLE_C / 4 mag_l + SIGMOID_C |r|),   SIGMOID_C = 5
           warped = p + dp r: the two inputs' errors, the product's rounding u |dp r| and the add's u |warped|, 1 u |dp r| second order:
               |warped - ref| <= |r| bound(dp) + |dp| bound(r) + u (2 |dp r| + |warped|)
  pts grad g_p[a] = (1 / voxel_len) sum_u s_ua d_ua V_u with V_u = g_0 den_u + sum_c g_{1+c} rgb_uc, d_ua the product of the other two
           axes' factors and s_ua = +-1.  V_u: a product and at most 3 adds per term, 4 u Vabs_u (Vabs_u = sum |g| |v|); d_ua: 1 - x twice
           and a product, 3 u; times V_u 1 u; the sum of 8 addends 7 u; the division 1 u; 1 u second order:
               |g_p - ref| <= PTS_C u magp_a / voxel_len,   PTS_C = 17,   magp_a = sum_u |d_ua| Vabs_u
  scatter  with D_a = G_a r + g_dp_a and q = (G . dp + g_r) (r (1 - r)), entry (row, 1 + 3 (k - 1) + a) sums w_u B_k D_a and entry
           (row, 0) sums w_u q over the samples' corners; dp and r are INPUTS (the forward's fp32 outputs), not recomputed.
           An addend w B_k D_a: w and the final product 4 roundings (voxel_ref's count), D_a two (relative to Dabs_a = |G_a| |r| +
           |g_dp_a|: the sum may cancel), B_k at most 3 (n - 1) + 1 (cubic: 4), B_k D_a one: 3 (n - 1) + 8.  An addend w q: G . dp + g_r
           at most 4 per term (relative to qabs = sum_a |G_a dp_a| + |g_r|), r (1 - r) 2, their product 1, w 4: 11 <= 3 (n - 1) + 8 for
           n >= 2.  Any summation order of cnt addends adds (cnt - 1) u mag:
               |got - ref| <= (cnt + 3 (n - 1) + 8) u mag   +  [deterministic mode]  (cnt 2^-40 + u |ref|)
           (every addend rounded to 2^-40 fixed point on its own, <= 2^-41 each, and one rounding when the integer sum is folded).
An entry with bound 0 must be exact.
"""
import numpy as np
import torch

import voxel_ref as V
from oracle.procedural import proc_uniform

U = V.U
SIGMOID_C = 5.0
PTS_C = 17.0
ROUND = 256          # samples of one round of a workgroup
F_N = 4096 * 256 + 1  # the smallest N at which a workgroup takes two rounds (DV_WG = 4096 workgroups x 256 samples)
SPLINES = (2, 4, 5, 11)


def spline_c(n):
    return V.SAMPLE_C + 3.0 * (n - 1) + 2.0


def scatter_c0(n):
    return 3.0 * (n - 1) + 8.0


def bernstein(t, n):
    """B_k(t), k = 0 .. n-1, of degree n - 1 in fp64: [N, n]"""
    t = t.double()
    from math import comb
    return torch.stack([comb(n - 1, k) * t ** k * (1 - t) ** (n - 1 - k) for k in range(n)], dim=-1)


def _lookup(pts, S, grid_radius):
    ids, xyz = V.cells(pts, S, grid_radius)
    return V.rows_of(ids, S), V.weights_of(xyz), xyz


# ------------------------------------------------------------------------------------------------------------ the deformation
def warp_ref(pts, t, ctrl, rig, spline, grid_radius=V.GRID_RADIUS):
    """pts [N,3] fp32, t [N], ctrl [S,S,S,3(n-1)], rig [S,S,S,1] -> dict of fp64 tensors: warped [N,3], dp [N,3], rigidity [N] and
    their bounds b_warped, b_dp, b_rigidity (module docstring)"""
    S, n = rig.shape[0], spline
    rows, w, _ = _lookup(pts, S, grid_radius)
    cv = ctrl.double().reshape(S ** 3, n - 1, 3)[rows]             # [N,8,n-1,3]
    cp = (w[..., None, None] * cv).sum(dim=1)                       # [N,n-1,3]
    mag = (w[..., None, None] * cv).abs().sum(dim=1)
    B = bernstein(t, n)[:, 1:, None]                                # control point 0 is zero
    dp, magdp = (B * cp).sum(dim=1), (B * mag).sum(dim=1)
    rv = rig.double().reshape(S ** 3)[rows]                         # [N,8]
    logit, magl = (w * rv).sum(dim=1), (w * rv).abs().sum(dim=1)
    r = torch.sigmoid(logit)
    warped = pts.double() + dp * r[:, None]
    b_dp = spline_c(n) * U * magdp
    b_r = U * (V.SAMPLE_C / 4 * magl + SIGMOID_C * r.abs())
    b_w = r.abs()[:, None] * b_dp + dp.abs() * b_r[:, None] + U * (2 * (dp * r[:, None]).abs() + warped.abs())
    return dict(warped=warped, dp=dp, rigidity=r, b_warped=b_w, b_dp=b_dp, b_rigidity=b_r)


def warp_backward_ref(pts, t, dp, rigidity, S, spline, grid_radius=V.GRID_RADIUS, g_warped=None, g_dp=None, g_rigidity=None):
    """the scatter of the module docstring: ref, mag, cnt [S^3, 1 + 3(n-1)] fp64 -- column 0 the rigidity grid's gradient, the rest
    ctrl_pts_grid's -- from the forward's dp [N,3] and rigidity [N] as given"""
    n, N = spline, pts.shape[0]
    rows, w, _ = _lookup(pts, S, grid_radius)
    z3, z1 = torch.zeros(N, 3, dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    G = z3 if g_warped is None else g_warped.double().reshape(N, 3)
    gd = z3 if g_dp is None else g_dp.double().reshape(N, 3)
    gr = z1 if g_rigidity is None else g_rigidity.double().reshape(N)
    r, dp = rigidity.double().reshape(N), dp.double().reshape(N, 3)
    D, Dabs = G * r[:, None] + gd, G.abs() * r.abs()[:, None] + gd.abs()
    dr = r * (1 - r)
    q, qabs = ((G * dp).sum(-1) + gr) * dr, ((G * dp).abs().sum(-1) + gr.abs()) * dr.abs()
    B = bernstein(t, n)[:, 1:]                                                                        # [N,n-1]
    sv = torch.cat([q[:, None], (B[:, :, None] * D[:, None, :]).reshape(N, -1)], dim=-1)              # [N,W]
    sabs = torch.cat([qabs[:, None], (B[:, :, None] * Dabs[:, None, :]).reshape(N, -1)], dim=-1)
    ref = torch.zeros(S ** 3, sv.shape[1], dtype=torch.float64)
    mag, cnt = torch.zeros_like(ref), torch.zeros_like(ref)
    ones = torch.ones_like(sv)
    for u in range(8):
        ref.index_add_(0, rows[:, u], w[:, u, None] * sv)
        mag.index_add_(0, rows[:, u], w[:, u, None].abs() * sabs)
        cnt.index_add_(0, rows[:, u], ones)
    return ref, mag, cnt


def scatter_bound(ref, mag, cnt, spline, det):
    b = (cnt + scatter_c0(spline)) * U * mag
    if det:
        b = b + cnt * 2.0 ** -40 + U * ref.abs()
    return b


def split_grids(flat, S):
    """[S^3, W] as warp_backward_ref lays it out -> (ctrl_pts_grid's [S,S,S,W-1], rigidity_grid's [S,S,S,1])"""
    return flat[:, 1:].reshape(S, S, S, -1), flat[:, :1].reshape(S, S, S, 1)


# ------------------------------------------------------------------------------------------------------------ the position gradient
def sample_backward_pts_ref(pts, g_raw, densities, rgb, grid_radius=V.GRID_RADIUS):
    """g_pts [N,3] fp64 of voxel_ref.sample_ref w.r.t. pts and its bound: only xyz depends on p"""
    S = densities.shape[0]
    rows, _, xyz = _lookup(pts, S, grid_radius)
    x = xyz.double()
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    grid = torch.cat([densities, rgb], dim=-1).double().reshape(S ** 3, -1)[rows]      # [N,8,1+C]
    g = g_raw.double().reshape(pts.shape[0], 1, -1)
    Vu, Vabs = (g * grid).sum(-1), (g * grid).abs().sum(-1)                            # [N,8]
    vl = float(np.float32(grid_radius * 2 / S))
    out, mag = [], []
    for a in range(3):
        o1, o2 = [i for i in range(3) if i != a]
        terms, tabs = [], []
        for u in range(8):
            f = lambda i: x[:, i] if V.bit_i(u, i) else 1 - x[:, i]
            d = f(o1) * f(o2)
            terms.append((1.0 if V.bit_i(u, a) else -1.0) * d * Vu[:, u])
            tabs.append(d.abs() * Vabs[:, u])
        out.append(sum(terms) / vl)
        mag.append(sum(tabs) / vl)
    return torch.stack(out, dim=-1), PTS_C * U * torch.stack(mag, dim=-1)


def sample_fp64(pts64, densities, rgb, grid_radius=V.GRID_RADIUS):
    """the lookup as a smooth fp64 function of pts64 [N,3] with the cells FROZEN at the fp32 image of pts64 (central differences inside
    a cell): raw [N, 1 + C]"""
    S = densities.shape[0]
    vl = grid_radius * 2 / S
    ids, _ = V.cells(pts64.float(), S, grid_radius)
    centre0 = (ids[:, 0, :].double() - S / 2 + 0.5) * vl
    x = (pts64 - centre0) / vl
    pick = lambda v, pos: v if pos else 1 - v
    w = torch.stack([pick(x[:, 0], V.bit_i(u, 0)) * pick(x[:, 1], V.bit_i(u, 1)) * pick(x[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    grid = torch.cat([densities, rgb], dim=-1).double().reshape(S ** 3, -1)[V.rows_of(ids, S)]
    return (w[..., None] * grid).sum(dim=1)


# ------------------------------------------------------------------------------------------------------------ inputs
def dyn_grids(S, spline, seed=4700):
    """(ctrl_pts_grid [S,S,S,3(n-1)], rigidity_grid [S,S,S,1]) uniform in +-1 / +-2"""
    return V._t(proc_uniform((S, S, S, 3 * (spline - 1)), seed + spline, 1.0)), V._t(proc_uniform((S, S, S, 1), seed + 50 + spline, 2.0))


def index_dyn_grids(S, spline):
    """grids whose entries encode their own (row, channel) with exact small integers: a wrong cell or channel is an error of order 1"""
    r = np.arange(S ** 3, dtype=np.int64)[:, None]
    ch = np.arange(3 * (spline - 1), dtype=np.int64)[None, :]
    ctrl = (((r * 7 + ch * 13) % 251) - 125).astype(np.float32).reshape(S, S, S, -1) / 64.0
    rig = (((r % 241) - 120).astype(np.float32) / 32.0).reshape(S, S, S, 1)
    return V._t(ctrl), V._t(rig)


def times(n, kind, seed=4800):
    """t [n]: all 0, all 1, or seeded values strictly inside (0, 1)"""
    if kind == "zero":
        return torch.zeros(n)
    if kind == "one":
        return torch.ones(n)
    return V._t((proc_uniform((n,), seed + n, 0.49) + 0.5).astype(np.float32))


def upstream(n, seed=4900):
    """(g_warped [n,3], g_dp [n,3], g_rigidity [n]) uniform in +-1"""
    return (V._t(proc_uniform((n, 3), seed + n, 1.0)), V._t(proc_uniform((n, 3), seed + n + 1, 1.0)), V._t(proc_uniform((n,), seed + n + 2, 1.0)))


def one_cell_points(n, S=16, grid_radius=V.GRID_RADIUS, seed=4950):
    """n points that read the same 8 rows (heavy duplicates in the scatter): within 0.2 voxel_len of a cell corner, so that p -+
    voxel_len / 2 stays strictly inside the two cells around it on every axis"""
    vl = grid_radius * 2 / S
    return V._t((np.array([[3.0, -3.0, 1.0]]) * vl + proc_uniform((n, 3), seed, 0.2 * vl)).astype(np.float32))


def model_ref(g):
    """a g25 fixture's case by this file's operators + voxel_ref's lookup and compositing, fp64: dict(out, alpha, weights, dp, rigidity)"""
    from conftest import golden_params
    p = golden_params(g)
    rays, ts, t = g["rays"], g["ts"], g["times"]
    pts = V.pts_of(rays, ts)                                           # [T,B,H,W,3]
    tt = t[None, :, None, None].expand(pts.shape[:-1])
    gr = float(g["grid_radius"])
    w = warp_ref(pts.reshape(-1, 3), tt.reshape(-1), p["ctrl_pts_grid"], p["rigidity_grid"], int(g["spline"]), gr)
    raw, _ = V.sample_ref(w["warped"].float().reshape(-1, 3), p["canonical.densities"], p["canonical.rgb"], gr)
    out, alpha, weights = V.composite_ref(raw.reshape(pts.shape[:-1] + (4,)), ts, rays, str(g["act"]), str(g["bg"]))
    return dict(out=out, alpha=alpha, weights=weights, dp=w["dp"].reshape(pts.shape), rigidity=w["rigidity"].reshape(pts.shape[:-1] + (1,)))
