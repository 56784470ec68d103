"""tests/voxel_plv_ref.py against the recorded reference (g27 static, g28 dynamic; tools/gen_golden.py) on the CPU: its lookup with the
pos-linear-view head, composited in fp64, reproduces the reference's fp64 out / alpha / weights; its scatter and its position gradient
reproduce the reference's fp64 grid gradients (S <= 16; the dynamic model's control-point gradients exist only through the position
gradient); the kernels' association restated in fp32 torch stays inside the bounds the kernels are held to (worst ratios printed)."""
import pytest
import torch

from conftest import golden_params, load_golden
import voxel_plv_ref as P
import voxel_ref as V

CASES = ("s64_black", "s16_ragged", "s4", "s2")
SMALL = ("s16_ragged", "s4", "s2")
DYN = ("s4_n4", "s16_n2")


def test_the_fixtures_carry_the_reference_heads_layout():
    for name in CASES:
        g = load_golden(f"g27_voxel_plv_{name}")
        p = golden_params(g)
        S = int(g["S"])
        assert sorted(p) == ["densities", "rgb"] and tuple(p["rgb"].shape) == (S, S, S, 28) and tuple(p["densities"].shape) == (S, S, S, 1)


def test_basis_is_orthonormal_and_dominated_by_its_absolute_form():
    """the closed forms integrate to the identity on the sphere (Gauss-Legendre in cos(theta) x uniform in phi: exact for the degree-8
    products) and Yabs >= |Y| everywhere; the zero direction gives the basis at the origin"""
    import numpy as np
    n_p = 32
    nodes, wts = np.polynomial.legendre.leggauss(12)
    ct, wt = torch.from_numpy(nodes), torch.from_numpy(wts)
    ph = (torch.arange(n_p, dtype=torch.float64) + 0.5) * (2 * torch.pi / n_p)
    st = (1 - ct ** 2).sqrt()
    d = torch.stack([(st[:, None] * ph.cos()[None]).reshape(-1), (st[:, None] * ph.sin()[None]).reshape(-1),
                     ct[:, None].expand(-1, n_p).reshape(-1)], dim=-1)
    q = (wt[:, None].expand(-1, n_p) * (2 * torch.pi / n_p)).reshape(-1)
    Y, Ya = P.basis(d.float(), 4)   # (fp32 directions: the normalisation in `basis` takes the rounding out again, up to 1e-7 in angle)
    gram = Y.T @ (Y * q[:, None])
    assert float((gram - torch.eye(25, dtype=torch.float64)).abs().max()) < 1e-5
    assert bool((Ya >= Y.abs() - 1e-15).all())
    Y0, _ = P.basis(torch.zeros(1, 3), 4)
    assert abs(float(Y0[0, 0]) - 0.28209479177387814) < 1e-15 and abs(float(Y0[0, 20]) - 3 * 0.10578554691520431) < 1e-15
    assert float(Y0[0, [1, 2, 3, 4, 5, 7, 8]].abs().max()) == 0.0


@pytest.mark.parametrize("name", CASES)
def test_model_reference_reproduces_the_fixture(name):
    """the reference's fp64 run and this file's (fp32 membership, fp64 behind it) differ by the fp32 rounding of xyz only"""
    g = load_golden(f"g27_voxel_plv_{name}")
    out, alpha, weights = P.model_ref(g)
    for got, key in ((out, "out64"), (alpha, "alpha64"), (weights, "weights64")):
        err = float((got - g[key]).abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


def _fp32_lookup(pts, dirs, den, rgb, S, gr, order):
    """the kernels' association in fp32 torch: per corner the coefficient sum in k order, then the corners in order (plain products and
    sums in place of the fma: one more rounding per term, inside the NK the bound allows)"""
    ids, xyz = V.cells(pts, S, gr)
    pick = lambda v, pos: v if pos else 1 - v
    w = torch.stack([pick(xyz[:, 0], V.bit_i(u, 0)) * pick(xyz[:, 1], V.bit_i(u, 1)) * pick(xyz[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    co = rgb.reshape(S ** 3, -1)[:, 3:][V.rows_of(ids, S)]
    Y = P.basis(dirs, order)[0].float()[torch.arange(pts.shape[0]) % dirs.shape[0]]
    s = torch.zeros(pts.shape[0])
    for u in range(8):
        d = Y[:, 0] * co[:, u, 0]
        for k in range(1, P.nk(order)):
            d = d + Y[:, k] * co[:, u, k]
        s = s + w[:, u] * d
    return s


@pytest.mark.parametrize("name", CASES)
def test_fp32_association_is_inside_the_sh_bound(name):
    g = load_golden(f"g27_voxel_plv_{name}")
    p = golden_params(g)
    S, gr = int(g["S"]), float(g["grid_radius"])
    pts = V.pts_of(g["rays"], g["ts"]).reshape(-1, 3)
    dirs = g["rays"][..., 3:].reshape(-1, 3)
    _, _, s, mag_s = P.sample_ref(pts, dirs, p["densities"], p["rgb"], gr)
    got = _fp32_lookup(pts, dirs, p["densities"], p["rgb"], S, gr, 4)
    ratio = V.worst_ratio(got, s, P.sh_bound(mag_s, 4))
    print(name, "worst |err| / bound", ratio)
    assert ratio <= 1.0


def _grid_grads(g, pts, dirs, ts, rays, p):
    """fp64 autograd through head and compositing gives (g_raw, g_sh); scatter_ref scatters them"""
    S, gr = int(g["S"]), float(g["grid_radius"])
    raw, _, s, _ = P.sample_ref(pts.reshape(-1, 3), dirs, p["densities"], p["rgb"], gr)
    raw, s = raw.requires_grad_(True), s.requires_grad_(True)
    rows = P.head_ref(raw, s, str(g["act"])).reshape(pts.shape[:-1] + (4,))
    out, _, _ = P.composite_final(rows, ts, rays, str(g["bg"]))
    out.square().sum().backward()
    ref, _, cnt = P.scatter_ref(pts.reshape(-1, 3), dirs, raw.grad, s.grad, S, 4, gr)
    assert int(cnt[:, 0].sum()) == 8 * pts.numel() // 3 and int(cnt[:, 28].sum()) == 8 * pts.numel() // 3
    return ref, raw.grad, s.grad


@pytest.mark.parametrize("name", SMALL)
def test_scatter_reference_reproduces_the_fixture_gradients(name):
    g = load_golden(f"g27_voxel_plv_{name}")
    p = golden_params(g)
    rays, ts = g["rays"], g["ts"]
    pts = V.pts_of(rays, ts)
    ref, _, _ = _grid_grads(g, pts, rays[..., 3:].reshape(-1, 3), ts, rays, p)
    for got, key in ((ref[:, 0], "g_densities64"), (ref[:, 1:], "g_rgb64")):
        want = g[key].reshape(got.shape)
        err = float((got - want).abs().max() / want.abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


def _dyn_warp64(g, p):
    """the reference's deformation restated in fp64 over voxel_ref's fp32 cells at the unwarped points: (pts, warped, dp, rigidity)"""
    S, n, gr = int(g["S"]), int(g["spline"]), float(g["grid_radius"])
    rays, ts = g["rays"], g["ts"]
    pts = V.pts_of(rays, ts)
    flat = pts.reshape(-1, 3)
    ids, xyz = V.cells(flat, S, gr)
    w = V.weights_of(xyz)
    rows = V.rows_of(ids, S)
    ctrl = (w[..., None] * p["ctrl_pts_grid"].double().reshape(S ** 3, -1)[rows]).sum(1).reshape(-1, n - 1, 3)
    rig = torch.sigmoid((w * p["rigidity_grid"].double().reshape(S ** 3)[rows]).sum(1))
    t = g["times"].double()[None, :, None, None].expand(pts.shape[:-1]).reshape(-1)
    c = torch.cat([torch.zeros(ctrl.shape[0], 1, 3, dtype=torch.float64), ctrl], dim=1)   # control point 0 is zero
    while c.shape[1] > 1:                                                                  # de Casteljau (equals the cubic form at n = 4)
        c = (1 - t)[:, None, None] * c[:, :-1] + t[:, None, None] * c[:, 1:]
    dp = c[:, 0]
    return pts, flat.double() + dp * rig[:, None], dp, rig


@pytest.mark.parametrize("name", DYN)
def test_dynamic_model_reference_reproduces_the_fixture(name):
    """forward of the voxel D-NeRF over the head: the warped points (fp64) are cast to fp32 for the canonical cells, as the kernels see
    them; dp and rigidity are the fixture's"""
    g = load_golden(f"g28_dyn_voxel_plv_{name}")
    p = golden_params(g)
    pts, warped, dp, rig = _dyn_warp64(g, p)
    assert float((dp.reshape(g["dp64"].shape) - g["dp64"]).abs().max()) <= 1e-5
    assert float((rig.reshape(g["rigidity64"].shape) - g["rigidity64"]).abs().max()) <= 1e-5
    out, alpha, weights = P.render_ref(g["rays"], g["ts"], p["canonical.densities"], p["canonical.rgb"], str(g["act"]), str(g["bg"]),
                                       pts=warped.float().reshape(pts.shape), grid_radius=float(g["grid_radius"]))
    for got, key in ((out, "out64"), (alpha, "alpha64"), (weights, "weights64")):
        err = float((got - g[key]).abs().max())
        print(name, key, err)
        assert err <= 2e-5, (name, key, err)


@pytest.mark.parametrize("name", DYN)
def test_position_gradient_reproduces_the_dynamic_fixture_gradients(name):
    """d sum(out^2) / d ctrl_pts_grid and rigidity_grid reach the deformation grids only through pts_grad_ref: chained by hand through
    warped = pts + dp * rigidity and scattered with the unwarped cells, against the reference's fp64 gradients"""
    g = load_golden(f"g28_dyn_voxel_plv_{name}")
    p = golden_params(g)
    S, n, gr = int(g["S"]), int(g["spline"]), float(g["grid_radius"])
    rays, ts = g["rays"], g["ts"]
    pts, warped, dp, rig = _dyn_warp64(g, p)
    w32 = warped.float()
    dirs = rays[..., 3:].reshape(-1, 3)
    ref, g_raw, g_sh = _grid_grads(g, w32.reshape(pts.shape), dirs, ts, rays, {"densities": p["canonical.densities"], "rgb": p["canonical.rgb"]})
    for got, key in ((ref[:, 0], "grad64.canonical.densities"), (ref[:, 1:], "grad64.canonical.rgb")):
        want = g[key].reshape(got.shape)
        err = float((got - want).abs().max() / want.abs().max())
        print(name, key, err)
        assert err <= 2e-5, (name, key, err)
    gp, _ = P.pts_grad_ref(w32, dirs, p["canonical.densities"], p["canonical.rgb"], g_raw, g_sh, gr)
    # warped = pts + dp r: d/d(dp) = G r, d/d(logit) = (G . dp) r (1 - r); dp = sum_k B_k(t) ctrl_k with Bernstein weights of degree n - 1
    t = g["times"].double()[None, :, None, None].expand(pts.shape[:-1]).reshape(-1)
    import math
    B = torch.stack([math.comb(n - 1, k) * t ** k * (1 - t) ** (n - 1 - k) for k in range(1, n)], dim=-1)      # [N, n-1]
    g_ctrl_s = (B[:, :, None] * (gp * rig[:, None])[:, None, :]).reshape(-1, 3 * (n - 1))
    g_rig_s = ((gp * dp).sum(-1) * rig * (1 - rig))[:, None]
    ids, xyz = V.cells(pts.reshape(-1, 3), S, gr)
    w, rows = V.weights_of(xyz), V.rows_of(ids, S)
    for src, key in ((g_ctrl_s, "grad64.ctrl_pts_grid"), (g_rig_s, "grad64.rigidity_grid")):
        acc = torch.zeros(S ** 3, src.shape[1], dtype=torch.float64)
        for u in range(8):
            acc.index_add_(0, rows[:, u], w[:, u, None] * src)
        want = g[key].reshape(acc.shape)
        err = float((acc - want).abs().max() / want.abs().max())
        print(name, key, err)
        assert err <= 1e-4, (name, key, err)
