"""tests/dyn_voxel_ref.py against the recorded reference (g25, tools/gen_golden.py) on the CPU: the restated deformation, composited in
fp64 through voxel_ref, reproduces the reference's fp64 out / alpha / weights / dp / rigidity and (S <= 16) its fp64 gradients of all
four grids -- the position gradient is the link between the two halves of that chain; the position gradient agrees with central
differences inside a cell; the reference's OWN fp32 dp and rigidity stay inside the bounds the kernels are held to."""
import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
import dyn_voxel_ref as D

CASES = ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11", "s64_n4")
SMALL = CASES[:4]


@pytest.mark.parametrize("name", CASES)
def test_model_reference_reproduces_the_fixture(name):
    """this file's run (fp32 membership, fp64 behind it) against the reference's fp64 run: they differ by the fp32 rounding of xyz and
    of the warped points only, far inside the 1e-4 bar the models are held to"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    got = D.model_ref(g)
    for key in ("out", "alpha", "weights", "dp", "rigidity"):
        err = float((got[key] - g[key + "64"]).abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


@pytest.mark.parametrize("name", CASES)
def test_the_references_fp32_outputs_are_inside_the_bounds(name):
    """a bound that the reference's own fp32 run breaks would be wrong: its dp and rigidity against the restatement, under the bounds of
    the warp (same cells -- the reference's fp32 chain -- and fp32 arithmetic behind them in torch's order)"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    p = golden_params(g)
    pts = V.pts_of(g["rays"], g["ts"])
    tt = g["times"][None, :, None, None].expand(pts.shape[:-1])
    w = D.warp_ref(pts.reshape(-1, 3), tt.reshape(-1), p["ctrl_pts_grid"], p["rigidity_grid"], int(g["spline"]), float(g["grid_radius"]))
    r_dp = V.worst_ratio(g["dp"], w["dp"], w["b_dp"])
    r_rig = V.worst_ratio(g["rigidity"], w["rigidity"], w["b_rigidity"])
    print(name, "worst |err| / bound: dp", r_dp, "rigidity", r_rig)
    assert r_dp <= 1.0 and r_rig <= 1.0


@pytest.mark.parametrize("name", SMALL)
def test_reference_chain_reproduces_the_fixture_gradients(name):
    """d sum(out^2) / d the four grids through the restated operators: fp64 compositing's autograd gives g_raw; voxel_ref.scatter_ref the
    canonical grids' gradients at the warped points; sample_backward_pts_ref g_warped; warp_backward_ref the deformation grids' --
    against the reference's fp64 gradients, within 1e-5 of the largest entry"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    p = golden_params(g)
    S, n, gr, rays, ts = int(g["S"]), int(g["spline"]), float(g["grid_radius"]), g["rays"], g["ts"]
    pts = V.pts_of(rays, ts)
    flat, tt = pts.reshape(-1, 3), g["times"][None, :, None, None].expand(pts.shape[:-1]).reshape(-1)
    w = D.warp_ref(flat, tt, p["ctrl_pts_grid"], p["rigidity_grid"], n, gr)
    warped = w["warped"].float()
    raw, _ = V.sample_ref(warped, p["canonical.densities"], p["canonical.rgb"], gr)
    raw = raw.reshape(pts.shape[:-1] + (4,)).requires_grad_(True)
    out, _, _ = V.composite_ref(raw, ts, rays, str(g["act"]), str(g["bg"]))
    out.square().sum().backward()
    g_raw = raw.grad.reshape(-1, 4)
    canon, _, _ = V.scatter_ref(warped, g_raw, S, gr)
    g_warped, _ = D.sample_backward_pts_ref(warped, g_raw, p["canonical.densities"], p["canonical.rgb"], gr)
    dyn, _, cnt = D.warp_backward_ref(flat, tt, w["dp"], w["rigidity"], S, n, gr, g_warped=g_warped)
    assert int(cnt[:, 0].sum()) == 8 * flat.shape[0]
    print(name, "the reference's own fp32 gradients vs its fp64 ones (g_dev):", g["g_dev"].tolist())
    for got, key in ((canon[:, 0], "canonical.densities"), (canon[:, 1:], "canonical.rgb"), (dyn[:, 1:], "ctrl_pts_grid"), (dyn[:, 0], "rigidity_grid")):
        want = g["grad64." + key].reshape(got.shape)
        err = float((got - want).abs().max() / want.abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


@pytest.mark.parametrize("S", (2, 4, 16))
def test_position_gradient_against_central_differences(S):
    """points strictly inside a cell, inside the grid and in the extrapolated region, with grid_radius 1 and fractions that are
    multiples of 1/32 in [1/8, 7/8]: voxel_len is a power of two and every coordinate, centre and xyz is exact in fp32, so the
    restatement (fp32 xyz, fp32 voxel_len) and the fp64 function differentiated here are the same polynomial.  Step 1e-6 voxel_len
    with the cells frozen: the lookup has degree <= 1 per axis, so the central difference is exact up to fp64 rounding (1e-16 / 1e-6)"""
    import numpy as np
    from oracle.procedural import proc_uniform
    gr = 1.0
    vl = gr * 2 / S
    k = np.floor(proc_uniform((200, 3), 5000 + S, S / 2 + 1.5))
    frac = np.rint((proc_uniform((200, 3), 5001 + S, 0.375) + 0.5) * 32) / 32
    pts = torch.from_numpy(((k + 0.5 + frac) * vl).astype(np.float32))
    assert torch.equal(pts.double(), torch.from_numpy((k + 0.5 + frac) * vl)) and float(pts.abs().max()) > gr
    den, rgb = V.grid_values(S)
    g_raw = torch.from_numpy(proc_uniform((200, 4), 5002 + S, 1.0))
    got, bound = D.sample_backward_pts_ref(pts, g_raw, den, rgb, gr)
    h = 1e-6 * vl
    p64 = pts.double()
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = h
        fd = ((D.sample_fp64(p64 + e, den, rgb, gr) - D.sample_fp64(p64 - e, den, rgb, gr)) * g_raw.double()).sum(-1) / (2 * h)
        err = float((fd - got[:, a]).abs().max() / got.abs().max())
        print(S, "axis", a, "relative to the largest entry:", err)
        assert err <= 1e-8
    assert float(bound.min()) >= 0


def test_bernstein_is_de_casteljau_and_the_cubic_form():
    t = D.times(64, "interior").double()
    for n in D.SPLINES:
        cp = torch.cat([torch.zeros(1, 64, 3, dtype=torch.float64), torch.randn(n - 1, 64, 3, generator=torch.Generator().manual_seed(n), dtype=torch.float64)])
        betas = cp
        for _ in range(1, n):
            betas = betas[:-1] * (1 - t)[None, :, None] + betas[1:] * t[None, :, None]
        want = betas.squeeze(0)
        got = (D.bernstein(t, n).T[:, :, None] * cp).sum(0)
        assert float((got - want).abs().max()) <= 1e-14
    m1t = 1 - t
    k = torch.stack([m1t * m1t * m1t, 3 * m1t * m1t * t, 3 * t * t * m1t, t * t * t], dim=-1)
    assert float((k - D.bernstein(t, 4)).abs().max()) <= 1e-15
