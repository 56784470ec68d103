"""The spline-length operators on the GPU (csrc/spline_len.hip): value, per-spline lengths and gradient of the grid term and of the
per-sample term, in both accumulation modes, against tests/spline_len_ref.py (membership fixed in fp32, everything behind it in fp64)
under that file's derived bounds; the recorded reference (g26) on top."""
import contextlib
import functools

import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
import spline_len_ref as R
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

NA_EUNSUPPORTED = -3   # include/nerf_atlas_amd.h
GR = V.GRID_RADIUS
GRID_K = (1, 63, 65, 257, 4096)
SAMPLE_N = (1, 255, 257)
W_KINDS = ("none", "signed", "zero")
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


def scalar(v):
    return torch.tensor([v], dtype=torch.float32, device="cuda")


WORST = {}   # operator -> the largest |err| / bound of (value, lens, grad) over the module's cases


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    yield
    for name, v in sorted(WORST.items()):
        print(f"\n[{name}] largest |err| / bound over all cases: value {v[0]:.3f} lens {v[1]:.3f} grad {v[2]:.3f}")


def check(what, det, got, r):
    """(value, lens, grad) of an operator pair against a reference dict: every entry inside its bound"""
    value, lens, grad = got
    ratios = [V.worst_ratio(value, r["value"], R.bound(r, "value", det)), V.worst_ratio(lens.reshape(-1), r["lens"], r["b_lens"]),
              V.worst_ratio(grad.reshape(r["grad"].shape), r["grad"], R.bound(r, "grad", det))]
    print(f"[{what} {'det' if det else 'atomic'}] worst |err| / bound: value {ratios[0]:.3f} lens {ratios[1]:.3f} grad {ratios[2]:.3f}")
    assert max(ratios) <= 1.0 and all(x == x for x in ratios), (what, det, ratios)
    name = what.split()[0]
    WORST[name] = [max(a, b) for a, b in zip(WORST.get(name, [0.0] * 3), ratios)]


# ------------------------------------------------------------------------------------------------------------ the grid term
def run_grid(ops, grid, rows, g_up=1.0):
    g, i = grid.cuda(), rows.cuda()
    value, lens = ops.grid_spline_len(g, i, want_lens=True)
    grad = ops.grid_spline_len_backward(g, i, scalar(g_up))
    assert value.shape == () and lens.shape == (rows.numel(),) and grad.shape == grid.shape
    return value.cpu(), lens.cpu(), grad.cpu()


@DET
@pytest.mark.parametrize("m", (1, 3, 4, 10))
def test_grid_term_every_entry_inside_its_bound(ops, m, det):
    """grids of 8 and 64 rows at one index, around the wave and the workgroup size and at 4096 (16 workgroups; far more indices than
    rows: every row is a sum of duplicates); an upstream scalar that is not 1"""
    for rows in (8, 64):
        grid = R.flat_grid(rows, m)
        for K in GRID_K:
            idx = R.indices(K, rows)
            with mode(det):
                got = run_grid(ops, grid, idx, g_up=-0.75)
            check(f"grid_spline_len rows={rows} m={m} K={K}", det, got, R.grid_ref(grid, idx, g_up=-0.75))
            if m == 1:
                assert float(got[0]) == 0.0 and bool((got[1] == 0).all()) and bool((got[2] == 0).all())


@DET
def test_grid_term_all_duplicate_indices(ops, det):
    grid = R.flat_grid(64, 4)
    idx = torch.full((257,), 37, dtype=torch.int64)
    with mode(det):
        got = run_grid(ops, grid, idx)
    r = R.grid_ref(grid, idx)
    check("grid_spline_len 257 copies of one row", det, got, r)
    assert int((got[2] != 0).any(dim=-1).sum()) == 1 and bool((got[1] == got[1][0]).all())


@DET
@pytest.mark.parametrize("m", (1, 3, 4, 10))
def test_grid_term_equal_control_points(ops, m, det):
    """equal control points whose products with t and 1 - t are exact (powers of two): value 0, an all-zero finite gradient -- a
    segment of length 0 adds exactly 0, not 0 / 0"""
    grid = torch.tensor([0.5, -2.0, 1.0]).repeat(8, m)
    idx = R.indices(257, 8)
    with mode(det):
        value, lens, grad = run_grid(ops, grid, idx)
    assert float(value) == 0.0 and bool((lens == 0).all())
    assert bool(torch.isfinite(grad).all()) and bool((grad == 0).all())
    check(f"grid_spline_len equal control points m={m}", det, (value, lens, grad), R.grid_ref(grid, idx))


def test_grid_term_refuses_an_index_outside_the_grid_on_the_host(ops):
    from nerf_atlas_amd import nerf
    grid = R.flat_grid(64, 3).cuda()
    for bad in (64, -1):
        idx = torch.tensor([0, bad, 5], dtype=torch.int64, device="cuda")
        with pytest.raises(ValueError, match="outside the grid"):
            ops.grid_spline_len(grid, idx)
        with pytest.raises(ValueError, match="outside the grid"):
            ops.grid_spline_len_backward(grid, idx, scalar(1.0))
        with pytest.raises(ValueError, match="outside the grid"):
            nerf.arc_len_grid(grid.reshape(4, 4, 4, 9), idxs=idx)


def test_grid_term_clamps_a_trusted_index_and_refuses_other_table_sizes(ops):
    """the kernel's own guard: a trusted index outside the grid reads the nearest row; M outside 2 .. 32 is NA_EUNSUPPORTED"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    grid = R.flat_grid(64, 3).cuda()
    far = torch.tensor([-5, 1 << 40, 7], dtype=torch.int64, device="cuda")
    near = torch.tensor([0, 63, 7], dtype=torch.int64, device="cuda")
    a, b = ops.grid_spline_len(grid, far, trusted=True, want_lens=True), ops.grid_spline_len(grid, near, want_lens=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    assert torch.equal(ops.grid_spline_len_backward(grid, far, scalar(1.0), trusted=True), ops.grid_spline_len_backward(grid, near, scalar(1.0)))
    t = torch.linspace(0, 1, 40).cuda()
    out = torch.zeros(2, device="cuda")
    for M in (1, 33):
        assert lib.na_grid_spline_len(ops._ptr(grid), 64, 3, ops._ptr(near), 3, ops._ptr(t), M, None, ops._ptr(out), ops._stream()) == NA_EUNSUPPORTED
        assert lib.na_grid_spline_len_backward(ops._ptr(grid), 64, 3, ops._ptr(near), 3, ops._ptr(t), M, ops._ptr(scalar(1.0)), ops._ptr(torch.zeros_like(grid)),
                                               ops._stream()) == NA_EUNSUPPORTED
    assert lib.na_grid_spline_len(ops._ptr(grid), 64, 11, ops._ptr(near), 3, ops._ptr(t), 16, None, ops._ptr(out), ops._stream()) == NA_EUNSUPPORTED


def test_arc_len_grid_names_the_references_voxels(ops):
    """nerf.arc_len_grid on a non-cubic grid at explicit flat indices: x = idx % s0 is the slowest axis in memory, as the reference's
    grid[x, y, z] reads it; its gradient arrives through autograd"""
    from nerf_atlas_amd import nerf
    shape = (4, 6, 2)
    grid = R.flat_grid(48, 3).reshape(*shape, 9)
    idx = R.indices(257, 48)
    x, y, z = idx % 4, idx // 4 % 6, idx // 24 % 2
    rows = torch.arange(48).reshape(shape)[x, y, z]
    r = R.grid_ref(grid.reshape(48, 9), rows, g_up=2.0)
    p = grid.cuda().requires_grad_(True)
    value = nerf.arc_len_grid(p, idxs=idx.cuda())
    (2.0 * value).backward()
    check("arc_len_grid 4x6x2", False, (value.detach().cpu(), r["lens"], p.grad.cpu()), r)
    drawn = nerf.arc_len_grid(p.detach(), samples=16 ** 3)
    assert drawn.shape == () and bool(torch.isfinite(drawn))


@pytest.mark.parametrize("name", ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11"))
def test_grid_term_on_the_recorded_reference(ops, name):
    """g26: inside the restatement's bound, and inside twice that of the reference's own fp32 numbers (both sit inside it)"""
    g = load_golden("g26_spline_len_" + name)
    S = int(g["S"])
    ctrl = golden_params(g)["ctrl_pts_grid"].reshape(S ** 3, -1)
    rows = R.rows_of_flat(g["g_idxs"], (S, S, S))
    got = run_grid(ops, ctrl, rows)
    r = R.grid_ref(ctrl, rows)
    check(f"grid_spline_len g26 {name}", False, got, r)
    for k, v in zip(("value", "lens", "grad"), got):
        assert V.worst_ratio(v.reshape(r[k].shape), g["g_" + k].double().reshape(r[k].shape), 2 * r["b_" + k]) <= 1.0, (name, k)


def test_grid_term_deterministic_mode_is_bitwise_reproducible(ops):
    for m, K in ((4, 4096), (10, 257)):
        grid = R.flat_grid(64, m)
        idx = R.indices(K, 64)
        order = torch.from_numpy(proc_uniform((K,), 5970, 1.0)).argsort()
        with mode(True):
            a, b, c = run_grid(ops, grid, idx), run_grid(ops, grid, idx), run_grid(ops, grid, idx[order])
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[2].view(torch.int32), c[2].view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ the per-sample term
def run_dyn(ops, pts, ctrl, n, w, g_up=1.0, order=None):
    sel = (lambda x: x) if order is None else (lambda x: x[order])
    p, c = sel(pts).cuda(), ctrl.cuda()
    wc = None if w is None else sel(w).cuda()
    value, lens = ops.dyn_voxel_spline_len(p, c, n, GR, wc, want_lens=True)
    grad = ops.dyn_voxel_spline_len_backward(p, c, n, GR, scalar(g_up), wc)
    assert value.shape == () and lens.shape == (pts.shape[0],) and grad.shape == ctrl.shape
    return value.cpu(), lens.cpu(), grad.cpu()


@DET
@pytest.mark.parametrize("n", R.SPLINES)
def test_sample_term_every_entry_inside_its_bound(ops, n, det):
    """uniform in +-2.5 -- the inside and the extrapolated region -- at one sample and around the workgroup size; S = 2 (every sample in
    the same 8 rows), 4 and 16; w NULL, signed and all zero cycled over them"""
    for i, S in enumerate((2, 4, 16)):
        ctrl = R.ctrl_grid(S, n)
        for j, N in enumerate(SAMPLE_N):
            kind = W_KINDS[(i + j + n) % 3]
            pts, w = V.uniform_points(N), R.sample_weights(N, kind)
            with mode(det):
                got = run_dyn(ops, pts, ctrl, n, w, g_up=1.5)
            check(f"dyn_voxel_spline_len S={S} n={n} N={N} w={kind}", det, got, R.dyn_ref(pts, ctrl, n, w, g_up=1.5))
            if kind == "zero":
                assert float(got[0]) == 0.0 and bool((got[2] == 0).all()) and bool((got[1] > 0).any())


@DET
def test_sample_term_every_weight_kind_at_one_shape(ops, det):
    ctrl = R.ctrl_grid(16, 4)
    pts = V.uniform_points(257)
    for kind in W_KINDS:
        w = R.sample_weights(257, kind)
        with mode(det):
            got = run_dyn(ops, pts, ctrl, 4, w)
        check(f"dyn_voxel_spline_len S=16 n=4 N=257 w={kind}", det, got, R.dyn_ref(pts, ctrl, 4, w))


@pytest.mark.parametrize("S", (2, 4, 16))
def test_sample_term_on_cell_planes_and_outside_the_grid(ops, S):
    """the membership planes, the corners and the points beyond the grid's border (voxel_ref.lattice_points)"""
    pts = V.lattice_points(S)
    for n in (4, 5):
        ctrl = R.ctrl_grid(S, n)
        w = R.sample_weights(pts.shape[0], "signed")
        check(f"dyn_voxel_spline_len S={S} n={n} lattice", False, run_dyn(ops, pts, ctrl, n, w), R.dyn_ref(pts, ctrl, n, w))


@functools.lru_cache(maxsize=None)
def two_rounds_case():
    """F_N samples, the smallest N at which a workgroup of the backward takes a second round (spline 2: 3 sums per row); computed once"""
    pts = torch.from_numpy(proc_uniform((R.F_N, 3), 5960, 1.5))
    ctrl, w = R.ctrl_grid(16, 2), R.sample_weights(R.F_N, "signed")
    return pts, ctrl, w, R.dyn_ref(pts, ctrl, 2, w)


@DET
def test_sample_term_second_round_of_a_workgroup(ops, det):
    pts, ctrl, w, r = two_rounds_case()
    with mode(det):
        got = run_dyn(ops, pts, ctrl, 2, w)
    check(f"dyn_voxel_spline_len two rounds N={R.F_N}", det, got, r)


def test_sample_term_one_nan_coordinate(ops):
    """a NaN coordinate: that sample's length and the value are not finite; the gradient is finite in every row the sample does not
    touch (its cells are the clamped ones: nothing outside the grid is addressed)"""
    ctrl = R.ctrl_grid(16, 4)
    pts = V.uniform_points(257).clone()
    pts[5, 1] = float("nan")
    w = R.sample_weights(257, "signed")
    r = R.dyn_ref(pts, ctrl, 4, w)
    value, lens, grad = run_dyn(ops, pts, ctrl, 4, w)
    assert not bool(torch.isfinite(value)) and not bool(torch.isfinite(lens[5]))
    assert bool(torch.isfinite(torch.cat([lens[:5], lens[6:]])).all())
    touched = torch.zeros(16 ** 3, dtype=torch.bool)
    touched[r["rows"][5]] = True
    g = grad.reshape(16 ** 3, -1)
    assert bool(torch.isfinite(g[~touched]).all()) and bool(torch.isnan(g[touched]).all())
    check("dyn_voxel_spline_len one NaN coordinate", False, (value, lens, grad), r)


@pytest.mark.parametrize("name", ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11"))
def test_sample_term_on_the_recorded_reference(ops, name):
    """g26: the reference's DynamicNeRFVoxel at one view -- inside the restatement's bound, and inside twice that of the reference's
    own fp32 numbers"""
    g = load_golden("g26_spline_len_" + name)
    S, n = int(g["S"]), int(g["spline"])
    ctrl = golden_params(g)["ctrl_pts_grid"]
    pts, w = R.fixture_points(g), g["s_weights"].reshape(-1)
    assert abs(float(g["grid_radius"]) - GR) < 1e-12
    got = run_dyn(ops, pts, ctrl, n, w)
    r = R.dyn_ref(pts, ctrl, n, w)
    check(f"dyn_voxel_spline_len g26 {name}", False, got, r)
    for k, v in zip(("value", "lens", "grad"), got):
        assert V.worst_ratio(v.reshape(r[k].shape), g["s_" + k].double().reshape(r[k].shape), 2 * r["b_" + k]) <= 1.0, (name, k)


def test_sample_term_deterministic_mode_is_bitwise_reproducible(ops):
    for n, N in ((4, 1000), (11, 1000)):
        ctrl = R.ctrl_grid(16, n)
        pts, w = V.uniform_points(N), R.sample_weights(N, "signed")
        order = torch.from_numpy(proc_uniform((N,), 5980, 1.0)).argsort()
        with mode(True):
            a, b, c = run_dyn(ops, pts, ctrl, n, w), run_dyn(ops, pts, ctrl, n, w), run_dyn(ops, pts, ctrl, n, w, order=order)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), n
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32)) and torch.equal(a[2].view(torch.int32), c[2].view(torch.int32)), n
    pts, ctrl, w, _ = two_rounds_case()
    order = torch.from_numpy(proc_uniform((R.F_N,), 5981, 1.0)).argsort()
    with mode(True):
        a, c = run_dyn(ops, pts, ctrl, 2, w), run_dyn(ops, pts, ctrl, 2, w, order=order)
    assert torch.equal(a[2].view(torch.int32), c[2].view(torch.int32))


def test_lens_are_optional_and_autograd_reaches_the_grid(ops):
    """lens NULL through the wrappers: the same value bits (deterministic mode); DynVoxelSplineLenFn and GridSplineLenFn return what the
    backward operators return, scaled by the upstream gradient on the device"""
    from nerf_atlas_amd import autograd as ag
    ctrl = R.ctrl_grid(16, 5).cuda()
    pts, w = V.uniform_points(257).cuda(), R.sample_weights(257, "signed").cuda()
    with mode(True):
        assert torch.equal(ops.dyn_voxel_spline_len(pts, ctrl, 5, GR, w), ops.dyn_voxel_spline_len(pts, ctrl, 5, GR, w, want_lens=True)[0])
        p = ctrl.clone().requires_grad_(True)
        (3.0 * ag.DynVoxelSplineLenFn.apply(p, pts, w, 5, GR)).backward()
        assert torch.equal(p.grad, ops.dyn_voxel_spline_len_backward(pts, ctrl, 5, GR, scalar(3.0), w))
        idx = R.indices(257, 16 ** 3).cuda()
        q = ctrl.clone().requires_grad_(True)
        (0.5 * ag.GridSplineLenFn.apply(q, idx, False)).backward()
        assert torch.equal(q.grad, ops.grid_spline_len_backward(ctrl, idx, scalar(0.5)))
