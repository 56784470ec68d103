"""The divergence operators of --dyn-model voxel on the GPU (csrc/dyn_voxel_div.hip): v . (J v) in both forms and the dp form's
scatter-add backward in both accumulation modes, against tests/dyn_voxel_div_ref.py (membership fixed in fp32, everything behind it in
fp64) under that file's derived bounds, and against the recorded reference (g29: the reference's own fp64 autograd), where the fp32 xyz
chain's share `b_xyz` is added to the bound.  No sample and no gradient entry is excluded anywhere."""
import contextlib
import functools

import pytest
import torch

from conftest import load_golden
import voxel_ref as V
import dyn_voxel_ref as D
import dyn_voxel_div_ref as R
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

NA_EWORKSPACE = -5   # include/nerf_atlas_amd.h
GR = V.GRID_RADIUS
CASES = ("s2_n2", "s4_n4", "s4_n5", "s16_n11_ragged")
SIZES = (1, 63, 257, 4099)
DET = pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def mode(det):
    """the deterministic mode is process-wide: always switched off again"""
    from nerf_atlas_amd import config
    if det:
        config.set_deterministic(True)
    try:
        yield
    finally:
        if det:
            config.set_deterministic(False)


@functools.lru_cache(maxsize=None)
def fixture(name):
    g = load_golden("g29_dyn_voxel_div_" + name)
    return g, R.fixture_case(g)


def cu(x):
    return None if x is None else x.cuda()


def run(ops, pts, t, ctrl, rig, n, v=None, gr=GR):
    out = ops.dyn_voxel_jac_quad(cu(pts), cu(t), cu(ctrl), cu(rig), n, gr, cu(v))
    assert out.shape == pts.shape[:-1] and out.dtype == torch.float32
    return out.cpu()


def check(ops, pts, t, ctrl, rig, n, v, what, gr=GR):
    """both forms of one input against the restatement: every sample inside its bound.  Returns (dp form, rigid form)."""
    got = []
    for form, r_grid in (("dp", None), ("rigid", rig)):
        ref = R.jac_quad_ref(pts, t, ctrl, r_grid, n, gr, v)
        out = run(ops, pts, t, ctrl, r_grid, n, v, gr)
        ratio = V.worst_ratio(out, ref["value"], ref["bound"])
        print(f"[dyn_voxel_jac_quad {what} {form}] worst |err| / bound {ratio:.3f}, |value| up to {float(ref['value'].nan_to_num().abs().max()):.3g}")
        assert ratio <= 1.0, (what, form, ratio)
        got.append(out)
    return got


# ------------------------------------------------------------------------------------------------------------ the two forms
@pytest.mark.parametrize("name", CASES)
def test_both_forms_against_the_recorded_reference(ops, name):
    g, c = fixture(name)
    args = (c["pts"], c["t"], c["ctrl"])
    for form, rig, v, want in (("ffjord", c["rig"], c["e"], g["div_approx"]), ("divergence", None, None, g["divergence"])):
        ref = R.jac_quad_ref(*args, rig, c["spline"], c["grid_radius"], v)
        got = run(ops, *args, rig, c["spline"], v, c["grid_radius"])
        r_ref = V.worst_ratio(got, ref["value"], ref["bound"])
        r_fix = V.worst_ratio(got, want.reshape(-1), ref["bound"] + ref["b_xyz"])
        print(f"[g29 {name} {form}] worst |err| / bound: restatement {r_ref:.3f}, the reference's fp64 run {r_fix:.3f}")
        assert r_ref <= 1.0 and r_fix <= 1.0


@pytest.mark.parametrize("n", D.SPLINES)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_uniform_points_at_every_size(ops, S, n):
    """uniform in +-2.5 (the inside and the extrapolated region) at one sample, below a wave, past a workgroup and at 17 workgroups; a
    direction per sample"""
    ctrl, rig = D.dyn_grids(S, n)
    for N in SIZES:
        check(ops, V.uniform_points(N), D.times(N, "interior"), ctrl, rig, n, R.directions(N), f"S={S} n={n} N={N}")


def test_end_points_of_the_spline(ops):
    """t = 0: the spline sits on control point 0 = 0 whatever the grids hold -- exactly 0 in both forms; t = 1: the last control point"""
    for n in (4, 5):
        ctrl, rig = D.dyn_grids(16, n)
        pts, v = V.uniform_points(257), R.directions(257)
        for out in check(ops, pts, D.times(257, "zero"), ctrl, rig, n, v, f"n={n} t=0"):
            assert bool((out == 0).all())
        check(ops, pts, D.times(257, "one"), ctrl, rig, n, v, f"n={n} t=1")


@pytest.mark.parametrize("S", (2, 4, 16))
def test_cell_faces_grid_boundary_and_far_outside(ops, S):
    """the lattice set (every membership plane, the corners +-grid_radius, the origin) and the tiny coordinates of both signs, against the
    restatement with the fp32 cell chain, on random grids and on grids that encode their own row and channel; points up to 50 from the grid"""
    for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points()), ("far", V.uniform_points(257, amp=50.0))):
        N = pts.shape[0]
        for n in (4, 5):
            for gname, (ctrl, rig) in (("random", D.dyn_grids(S, n)), ("index", D.index_dyn_grids(S, n))):
                check(ops, pts, D.times(N, "interior"), ctrl, rig, n, R.directions(N), f"S={S} n={n} {name} {gname} grid")


def test_s2_outside_both_neighbours_are_one_voxel(ops):
    """S = 2, every coordinate beyond the outermost centre by more than half a voxel: the lower and the upper neighbour of each axis are the
    same voxel, the eight rows coincide and sum_u grad w_u = 0 -- the result cancels to 0 within the bound"""
    sign = torch.from_numpy(proc_uniform((257, 3), 5200, 1.0)).sign()
    pts = sign * (2.0 + torch.from_numpy(proc_uniform((257, 3), 5201, 0.5)).abs())
    ids, _ = V.cells(pts, 2, GR)
    assert bool((ids == ids[:, :1]).all())
    for n in (2, 4):
        ctrl, rig = D.dyn_grids(2, n)
        for form, r_grid in (("dp", None), ("rigid", rig)):
            ref = R.jac_quad_ref(pts, D.times(257, "interior"), ctrl, r_grid, n, GR, R.directions(257))
            got = run(ops, pts, D.times(257, "interior"), ctrl, r_grid, n, R.directions(257))
            assert float(ref["value"].abs().max()) <= 1e-9 and bool((got.double().abs() <= ref["bound"]).all()), (n, form)


def test_saturated_rigidity_stays_finite(ops):
    """rigidity logits of +-40 inside the grid (the weights are a convex combination there): s = 1 makes s (1 - s) exactly 0 and the
    rigid form the dp form; s = e^-40 makes the whole term vanish (below 1e-15); both stay finite and inside the bound"""
    n, S, N = 4, 16, 257
    ctrl, _ = D.dyn_grids(S, n)
    pts, t, v = V.uniform_points(N, amp=1.2), D.times(N, "interior"), R.directions(N)
    dp_form = run(ops, pts, t, ctrl, None, n, v)
    for logit in (40.0, -40.0):
        rig = torch.full((S, S, S, 1), logit)
        _, rigid = check(ops, pts, t, ctrl, rig, n, v, f"rigidity logits {logit:+.0f}")
        assert bool(torch.isfinite(rigid).all())
        if logit > 0:
            assert torch.equal(rigid, dp_form)
        else:
            assert float(rigid.abs().max()) < 1e-15 * max(1.0, float(dp_form.abs().max()))


def test_null_direction_is_ones_bit_for_bit(ops):
    for n in (2, 4, 11):
        ctrl, rig = D.dyn_grids(16, n)
        pts, t = V.uniform_points(257), D.times(257, "interior")
        for r_grid in (None, rig):
            a, b = run(ops, pts, t, ctrl, r_grid, n, None), run(ops, pts, t, ctrl, r_grid, n, torch.ones(257, 3))
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def bad_points(n=257):
    pts = V.uniform_points(n).clone()
    bad = {5: (1, float("nan")), 70: (0, float("inf")), 200: (2, float("-inf")), 256: (0, float("nan"))}
    for i, (a, val) in bad.items():
        pts[i, a] = val
    return pts, sorted(bad)


def test_non_finite_coordinates_are_nan_samples_and_nothing_else(ops):
    ctrl, rig = D.dyn_grids(16, 4)
    pts, bad = bad_points()
    t, v = D.times(257, "interior"), R.directions(257)
    clean = check(ops, V.uniform_points(257), t, ctrl, rig, 4, v, "clean")
    got = check(ops, pts, t, ctrl, rig, 4, v, "NaN / Inf coordinates")
    for g, c in zip(got, clean):
        rows = torch.isnan(g)
        assert torch.nonzero(rows).flatten().tolist() == bad
        assert torch.equal(g[~rows].view(torch.int32), c[~rows].view(torch.int32))


def test_no_samples(ops):
    ctrl, rig = (x.cuda() for x in D.dyn_grids(4, 4))
    pts, t = torch.zeros(0, 3).cuda(), torch.zeros(0).cuda()
    for r_grid in (None, rig):
        assert ops.dyn_voxel_jac_quad(pts, t, ctrl, r_grid, 4, GR).shape == (0,)
    g = ops.dyn_voxel_jac_quad_backward(pts, t, 4, 4, GR, torch.zeros(0).cuda())
    assert g.shape == (4, 4, 4, 9) and bool((g == 0).all())


# ------------------------------------------------------------------------------------------------------------ scatter-add
def run_backward(ops, pts, t, S, n, g, v=None, order=None, gr=GR):
    sel = (lambda x: x) if order is None else (lambda x: None if x is None else x[order])
    out = ops.dyn_voxel_jac_quad_backward(cu(sel(pts)), cu(sel(t)), S, n, gr, cu(sel(g)), cu(sel(v)))
    assert out.shape == (S, S, S, 3 * (n - 1))
    return out.reshape(S ** 3, -1).cpu()


def check_backward(ops, pts, t, S, n, det, what, v="directions", gr=GR):
    N = pts.shape[0]
    g = torch.from_numpy(proc_uniform((N,), 5300 + N, 1.0))
    v = R.directions(N) if isinstance(v, str) else v
    ref, mag, cnt, _ = R.jac_quad_backward_ref(pts, t, S, n, g, gr, v)
    with mode(det):
        got = run_backward(ops, pts, t, S, n, g, v, gr=gr)
    ratio = V.worst_ratio(got, ref, R.scatter_bound(ref, mag, cnt, n, det))
    print(f"[dyn_voxel_jac_quad_backward {what} {'det' if det else 'atomic'}] worst |err| / bound {ratio:.3f}, most addends in one entry {int(cnt.max())}")
    assert ratio <= 1.0, (what, det, ratio)
    return got, ref


@DET
@pytest.mark.parametrize("name", CASES)
def test_backward_against_the_recorded_gradient(ops, name, det):
    """d mean(divergence) / d ctrl_pts_grid: g = 1 / N per sample, v = ones"""
    g, c = fixture(name)
    N, S, n = c["pts"].shape[0], int(g["S"]), c["spline"]
    up = torch.full((N,), 1.0 / N)
    ref, mag, cnt, bx = R.jac_quad_backward_ref(c["pts"], c["t"], S, n, up, c["grid_radius"], None)
    with mode(det):
        got = run_backward(ops, c["pts"], c["t"], S, n, up, None, gr=c["grid_radius"])
    bound = R.scatter_bound(ref, mag, cnt, n, det)
    r_ref = V.worst_ratio(got, ref, bound)
    # (1 / N as an fp32 number is off by u relative: u mag on top, for the fixture's exact 1 / N)
    r_fix = V.worst_ratio(got, g["g_ctrl"].reshape(ref.shape), bound + bx + R.U * mag)
    print(f"[g29 {name} backward {'det' if det else 'atomic'}] worst |err| / bound: restatement {r_ref:.3f}, the reference's fp64 gradient {r_fix:.3f}")
    assert r_ref <= 1.0 and r_fix <= 1.0


@DET
@pytest.mark.parametrize("n", D.SPLINES)
def test_backward_every_entry_inside_its_bound(ops, n, det):
    for i, N in enumerate(SIZES):
        S = (2, 4, 16)[(i + n) % 3]
        check_backward(ops, V.uniform_points(N), D.times(N, "interior"), S, n, det, f"S={S} n={n} N={N}")


@DET
def test_backward_all_samples_in_one_cell(ops, det):
    """1000 samples that read the same 8 rows: 1000 addends per entry, all through one slot of the LDS table"""
    for n in (4, 11):
        got, ref = check_backward(ops, D.one_cell_points(1000), D.times(1000, "interior"), 16, n, det, f"one cell n={n}")
        assert int((ref != 0).any(dim=-1).sum()) == 8 and int((got != 0).any(dim=-1).sum()) == 8
    check_backward(ops, D.one_cell_points(1000), D.times(1000, "interior"), 16, 4, det, "one cell, v = ones", v=None)


def test_deterministic_backward_is_independent_of_run_and_sample_order(ops):
    for n, N in ((4, 1000), (11, 4099)):
        pts, t, v = V.uniform_points(N), D.times(N, "interior"), R.directions(N)
        g = torch.from_numpy(proc_uniform((N,), 5300 + N, 1.0))
        order = torch.from_numpy(proc_uniform((N,), 5400, 1.0)).argsort()
        with mode(True):
            a, b, c = (run_backward(ops, pts, t, 16, n, g, v, order=o) for o in (None, None, order))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), n


def test_atomic_mode_is_within_the_bounds_of_the_deterministic_mode(ops):
    N, S, n = 4099, 16, 5
    pts, t, v = V.uniform_points(N), D.times(N, "interior"), R.directions(N)
    g = torch.from_numpy(proc_uniform((N,), 5300 + N, 1.0))
    ref, mag, cnt, _ = R.jac_quad_backward_ref(pts, t, S, n, g, GR, v)
    atomic = run_backward(ops, pts, t, S, n, g, v)
    with mode(True):
        fixed = run_backward(ops, pts, t, S, n, g, v)
    bound = R.scatter_bound(ref, mag, cnt, n, False) + R.scatter_bound(ref, mag, cnt, n, True)
    assert V.worst_ratio(atomic, fixed.double(), bound) <= 1.0


def test_a_too_small_deterministic_workspace_is_refused(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    S, n = 16, 4
    pts, t = V.uniform_points(65).cuda(), D.times(65, "interior").cuda()
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        with pytest.raises(_lib.NaError) as err:
            ops.dyn_voxel_jac_quad_backward(pts, t, S, n, GR, torch.ones(65).cuda())
        assert err.value.code == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 9 * S ** 3} bytes" in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0
    finally:
        config.set_deterministic(False)


# ------------------------------------------------------------------------------------------------------------ the model's methods
def small_model(S=16, n=5, steps=12):
    from nerf_atlas_amd import nerf, refl
    vox = nerf.NeRFVoxel(resolution=S, steps=steps, t_near=2.0, t_far=6.0)
    vox.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    m = nerf.DynamicNeRFVoxel(vox, spline=n)
    ctrl, rig = D.dyn_grids(S, n)
    with torch.no_grad():
        m.ctrl_pts_grid.copy_(ctrl)
        m.rigidity_grid.copy_(rig)
    return m.cuda().train()


def test_sum_jacobian_div_is_linear_in_the_grid_with_the_analytic_gradient(ops):
    """a finite difference of sum_jacobian_div().mean() along one random direction of ctrl_pts_grid against <analytic gradient, direction>.
    The term is linear in the grid, so ONE difference is exact up to rounding: the bound is the restatement's -- the mean of the per-sample
    bounds at both ends (the means are formed in fp64 from the kernel's per-sample values) plus the scatter's bound contracted with
    |direction|."""
    S, n = 16, 5
    m = small_model(S, n)
    torch.manual_seed(7)
    rays = V.generic_rays((2, 3, 5)).cuda()
    m((rays, torch.tensor([0.3, 0.8]).cuda()))
    pts, tt = m.pts.detach().reshape(-1, 3).cpu(), m._tt.reshape(-1).cpu()
    N = pts.shape[0]
    div = m.sum_jacobian_div()
    assert div.shape == m.pts.shape[:-1] + (1,) and div.requires_grad
    div.mean().backward()
    grad = m.ctrl_pts_grid.grad.detach().cpu().double().reshape(S ** 3, -1)
    assert m.rigidity_grid.grad is None and m.canonical.densities.grad is None     # the gradient reaches ctrl_pts_grid only
    theta0 = m.ctrl_pts_grid.detach().cpu().clone()
    delta = torch.from_numpy(proc_uniform(tuple(theta0.shape), 5500, 0.5))
    theta1 = theta0 + delta                                                         # (the fp32 sum IS the second end point)
    step = (theta1.double() - theta0.double()).reshape(S ** 3, -1)
    f0 = div.detach().double().mean().item()
    with torch.no_grad():
        m.ctrl_pts_grid.copy_(theta1)
        f1 = m.sum_jacobian_div().double().mean().item()
    r0 = R.jac_quad_ref(pts, tt, theta0, None, n, m.canonical.grid_radius)
    r1 = R.jac_quad_ref(pts, tt, theta1, None, n, m.canonical.grid_radius)
    ref, mag, cnt, _ = R.jac_quad_backward_ref(pts, tt, S, n, torch.full((N,), 1.0 / N, dtype=torch.float64), m.canonical.grid_radius)
    b_grad = ((R.scatter_bound(ref, mag, cnt, n, False) + R.U * mag) * step.abs()).sum().item()
    bound = r0["bound"].mean().item() + r1["bound"].mean().item() + b_grad
    analytic = (grad * step).sum().item()
    print(f"[finite difference] f1 - f0 = {f1 - f0:.9f}, <grad, step> = {analytic:.9f}, difference {abs(f1 - f0 - analytic):.2e}, bound {bound:.2e}")
    assert abs((f1 - f0) - analytic) <= bound
    assert abs((r1["value"].mean() - r0["value"].mean()).item() - (ref * step).sum().item()) <= 1e-12      # the restatement agrees with itself


def test_ffjord_div_has_the_reference_shape_and_no_graph(ops):
    m = small_model()
    torch.manual_seed(8)
    rays = V.generic_rays((2, 3, 5)).cuda()
    m((rays, torch.tensor([0.3, 0.8]).cuda()))
    e = torch.from_numpy(proc_uniform(tuple(m.pts.shape), 5600, 1.0)).cuda()
    div = m.ffjord_div(e)
    assert div.shape == m.pts.shape[:-1] and not div.requires_grad
    ref = R.jac_quad_ref(m.pts.detach().reshape(-1, 3).cpu(), m._tt.reshape(-1).cpu(), m.ctrl_pts_grid.detach().cpu(), m.rigidity_grid.detach().cpu(),
                         m.spline, m.canonical.grid_radius, e.reshape(-1, 3).cpu())
    assert V.worst_ratio(div.reshape(-1), ref["value"], ref["bound"]) <= 1.0
    m.eval()
    with torch.no_grad():
        m((rays, torch.tensor([0.3, 0.8]).cuda()))
        assert not m.sum_jacobian_div().requires_grad and m.sum_jacobian_div().shape == m.pts.shape[:-1] + (1,)


# ------------------------------------------------------------------------------------------------------------ arguments
def test_argument_checks_and_return_codes(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    S, n = 4, 4
    ctrl, rig = (x.cuda() for x in D.dyn_grids(S, n))
    pts, t = V.uniform_points(8).cuda(), D.times(8, "interior").cuda()
    with pytest.raises(ValueError, match="pts must be a CUDA"):
        ops.dyn_voxel_jac_quad(pts.cpu(), t, ctrl, rig, n, GR)
    with pytest.raises(ValueError, match="v must be float32"):
        ops.dyn_voxel_jac_quad(pts, t, ctrl, rig, n, GR, pts.double())
    with pytest.raises(ValueError, match="one time per sample"):
        ops.dyn_voxel_jac_quad(pts, t[:4], ctrl, rig, n, GR)
    with pytest.raises(ValueError, match="one direction per sample"):
        ops.dyn_voxel_jac_quad(pts, t, ctrl, None, n, GR, pts[:4])
    for r_grid in (None, rig):
        with pytest.raises(ValueError, match="ctrl_pts_grid"):
            ops.dyn_voxel_jac_quad(pts, t, ctrl, r_grid, 5, GR)                              # 9 channels are spline 4
        with pytest.raises(ValueError, match="spline 12"):
            ops.dyn_voxel_jac_quad(pts, t, ctrl, r_grid, 12, GR)
    with pytest.raises(ValueError, match="even"):
        ops.dyn_voxel_jac_quad(pts, t, torch.zeros(3, 3, 3, 9).cuda(), None, n, GR)
    with pytest.raises(ValueError, match="even"):
        ops.dyn_voxel_jac_quad_backward(pts, t, 3, n, GR, t)
    with pytest.raises(ValueError, match="g has 4 elements"):
        ops.dyn_voxel_jac_quad_backward(pts, t, S, n, GR, t[:4])
    with pytest.raises(ValueError, match="spline 1"):
        ops.dyn_voxel_jac_quad_backward(pts, t, S, 1, GR, t)
    # non-contiguous inputs are copied: the same bits
    wide = torch.zeros(8, 6).cuda()
    wide[:, :3] = pts
    assert torch.equal(ops.dyn_voxel_jac_quad(wide[:, :3], t, ctrl, rig, n, GR), ops.dyn_voxel_jac_quad(pts, t, ctrl, rig, n, GR))
    # the raw C ABI
    out, gout = torch.zeros(8).cuda(), torch.zeros_like(ctrl)
    P, st = ops._ptr, ops._stream()
    fwd, bwd = lib.na_dyn_voxel_jac_quad, lib.na_dyn_voxel_jac_quad_backward
    for bad_n in (1, 12):
        assert fwd(P(pts), P(t), 8, P(ctrl), P(rig), S, bad_n, GR, None, P(out), st) == -3 and b"spline" in lib.na_last_error()
        assert bwd(P(pts), P(t), 8, S, bad_n, GR, None, P(t), P(gout), st) == -3 and b"spline" in lib.na_last_error()
    assert fwd(P(pts), P(t), 8, P(ctrl), P(rig), 3, n, GR, None, P(out), st) == -1 and b"resolution 3" in lib.na_last_error()
    assert fwd(P(pts), P(t), -1, P(ctrl), P(rig), S, n, GR, None, P(out), st) == -1
    for k, name in ((0, b"pts"), (1, b"t"), (3, b"ctrl_pts_grid"), (9, b"out")):
        a = [P(pts), P(t), 8, P(ctrl), P(rig), S, n, GR, None, P(out), st]
        a[k] = None
        assert fwd(*a) == -2 and lib.na_last_error().endswith(b"null pointer " + name), lib.na_last_error()
    for k, name in ((0, b"pts"), (1, b"t"), (7, b"g"), (8, b"g_ctrl_pts_grid")):
        a = [P(pts), P(t), 8, S, n, GR, None, P(t), P(gout), st]
        a[k] = None
        assert bwd(*a) == -2 and lib.na_last_error().endswith(b"null pointer " + name), lib.na_last_error()
    assert fwd(None, None, 0, None, None, S, n, GR, None, None, st) == 0 and bwd(None, None, 0, S, n, GR, None, None, None, st) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((gout == 0).all())
