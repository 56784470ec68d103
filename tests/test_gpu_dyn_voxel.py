"""--dyn-model voxel on the GPU (csrc/dyn_voxel.hip, na_voxel_sample_backward_pts of csrc/voxel.hip): the one-launch deformation, its
scatter-add backward in both accumulation modes and the lookup's position gradient against tests/dyn_voxel_ref.py (membership fixed
in fp32, everything behind it in fp64) under that file's derived bounds, and the model against the recorded reference (g25) under the
project's 1e-4 bars."""
import contextlib

import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
import dyn_voxel_ref as D
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

NA_EWORKSPACE = -5   # include/nerf_atlas_amd.h
SIZES = (1, 63, 64, 65, 257, 1000)
KINDS = ("zero", "one", "interior")
GR = V.GRID_RADIUS


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


def run_warp(ops, pts, t, ctrl, rig, n, gr=GR):
    return ops.dyn_voxel_warp(pts.cuda(), t.cuda(), ctrl.cuda(), rig.cuda(), n, gr)


def check_warp(ops, pts, t, ctrl, rig, n, what, gr=GR):
    ref = D.warp_ref(pts, t, ctrl, rig, n, gr)
    got = run_warp(ops, pts, t, ctrl, rig, n, gr)
    assert got[0].shape == pts.shape and got[1].shape == pts.shape and got[2].shape == pts.shape[:-1]
    ratios = [V.worst_ratio(g, ref[k], ref["b_" + k]) for g, k in zip(got, ("warped", "dp", "rigidity"))]
    print(f"[dyn_voxel_warp {what}] worst |err| / bound: warped {ratios[0]:.3f} dp {ratios[1]:.3f} rigidity {ratios[2]:.3f}")
    assert max(ratios) <= 1.0 and all(r == r for r in ratios), (what, ratios)
    return got


# ------------------------------------------------------------------------------------------------------------ the deformation
@pytest.mark.parametrize("n", D.SPLINES)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_warp_uniform_points(ops, S, n):
    """uniform in +-2.5 -- the inside and the extrapolated region -- at every ragged size; t = 0, 1 and interior values cycled over them"""
    ctrl, rig = D.dyn_grids(S, n)
    for i, N in enumerate(SIZES):
        check_warp(ops, V.uniform_points(N), D.times(N, KINDS[(i + n) % 3]), ctrl, rig, n, f"S={S} n={n} N={N}")


def test_warp_s64(ops):
    for n in (4, 11):
        ctrl, rig = D.dyn_grids(64, n)
        check_warp(ops, V.uniform_points(1000), D.times(1000, "interior"), ctrl, rig, n, f"S=64 n={n} N=1000")


@pytest.mark.parametrize("S", (2, 4, 16))
def test_warp_lattice_and_zero_sets(ops, S):
    """the membership planes, the corners, the origin and tiny coordinates of both signs, on random grids and on grids whose entries
    encode their own row and channel (a wrong cell or channel is an error of order 1 there); the cubic and the de Casteljau branch"""
    for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points())):
        for n in (4, 5):
            for gname, (ctrl, rig) in (("random", D.dyn_grids(S, n)), ("index", D.index_dyn_grids(S, n))):
                check_warp(ops, pts, D.times(pts.shape[0], "interior"), ctrl, rig, n, f"S={S} n={n} {name} {gname} grid")


def test_warp_optional_outputs_and_end_points(ops):
    """dp / rigidity NULL through the C ABI: warped is the same bits; at t = 0 the spline sits on control point 0 = 0 exactly"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    ctrl, rig = (x.cuda() for x in D.dyn_grids(16, 5))
    pts, t = V.uniform_points(257).cuda(), D.times(257, "interior").cuda()
    full = ops.dyn_voxel_warp(pts, t, ctrl, rig, 5, GR)
    only = torch.empty_like(pts)
    rc = lib.na_dyn_voxel_warp(ops._ptr(pts), ops._ptr(t), 257, ops._ptr(ctrl), ops._ptr(rig), 16, 5, GR, ops._ptr(only), None, None, ops._stream())
    assert rc == 0 and torch.equal(only, full[0])
    for n in (4, 5):
        ctrl, rig = D.dyn_grids(16, n)
        w, dp, _ = ops.dyn_voxel_warp(pts, torch.zeros_like(t), ctrl.cuda(), rig.cuda(), n, GR)
        assert bool((dp == 0).all()) and torch.equal(w, pts)


def bad_points(n=257):
    pts = V.uniform_points(n).clone()
    bad = {5: (1, float("nan")), 70: (0, float("inf")), 200: (2, float("-inf")), 256: (0, float("nan"))}
    for i, (a, v) in bad.items():
        pts[i, a] = v
    return pts, sorted(bad)


def test_warp_non_finite_coordinates_are_nan_rows_and_nothing_else(ops):
    ctrl, rig = D.dyn_grids(16, 4)
    pts, bad = bad_points()
    t = D.times(257, "interior")
    clean = run_warp(ops, V.uniform_points(257), t, ctrl, rig, 4)
    got = check_warp(ops, pts, t, ctrl, rig, 4, "S=16 NaN / Inf coordinates")
    for g, c in zip(got, clean):
        g, c = g.reshape(257, -1).cpu(), c.reshape(257, -1).cpu()
        rows = torch.isnan(g).any(dim=-1)
        assert torch.nonzero(rows).flatten().tolist() == bad and bool(torch.isnan(g[rows]).all())
        assert torch.equal(g[~rows], c[~rows])


# ------------------------------------------------------------------------------------------------------------ scatter-add
def run_backward(ops, pts, t, ctrl, rig, n, S, grads=(True, True, True), order=None, gr=GR, want_ref=True):
    """the forward on the GPU gives dp and rigidity; (got [S^3, W] as the reference lays it out, the reference's (ref, mag, cnt))"""
    N = pts.shape[0]
    up = [g if on else None for g, on in zip(D.upstream(N), grads)]
    _, dp, r = run_warp(ops, pts, t, ctrl, rig, n, gr)
    ref = D.warp_backward_ref(pts, t, dp.cpu(), r.cpu(), S, n, gr, *up) if want_ref else None
    sel = (lambda x: x) if order is None else (lambda x: None if x is None else x[order])
    cu = lambda x: None if x is None else sel(x).cuda()
    gc, gg = ops.dyn_voxel_warp_backward(cu(pts), cu(t), sel(dp), sel(r), S, n, gr, *[cu(g) for g in up])
    assert gc.shape == (S, S, S, 3 * (n - 1)) and gg.shape == (S, S, S, 1)
    return torch.cat([gg, gc], dim=-1).reshape(S ** 3, -1).cpu(), ref


def check_backward(ops, pts, t, n, S, det, what, **kw):
    ctrl, rig = D.dyn_grids(S, n)
    with mode(det):
        got, (ref, mag, cnt) = run_backward(ops, pts, t, ctrl, rig, n, S, **kw)
    ratio = V.worst_ratio(got, ref, D.scatter_bound(ref, mag, cnt, n, det))
    print(f"[dyn_voxel_warp_backward {what} {'det' if det else 'atomic'}] worst |err| / bound {ratio:.3f}, most addends in one entry {int(cnt.max())}")
    assert ratio <= 1.0, (what, det, ratio)
    return got, ref


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("n", D.SPLINES)
def test_backward_every_entry_inside_its_bound(ops, n, det):
    """ragged sizes (one and several workgroups), S = 2 (every sample in the same 8 rows), 4 and 16; the three upstream gradients
    together"""
    for i, N in enumerate(SIZES):
        S = (2, 4, 16)[i % 3]
        check_backward(ops, V.uniform_points(N), D.times(N, KINDS[(i + n) % 3]), n, S, det, f"S={S} n={n} N={N}")


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_backward_duplicates_lattice_and_two_rounds(ops, det):
    """all samples in one cell (256 and 1000 addends per entry); the lattice set; F_N samples, the smallest N at which a workgroup takes a
    second round (spline 2: 4 sums per row)"""
    for N in (256, 1000):
        got, ref = check_backward(ops, D.one_cell_points(N), D.times(N, "interior"), 4, 16, det, f"one cell N={N}")
        assert int((ref != 0).any(dim=-1).sum()) == 8
    lat = V.lattice_points(16)
    check_backward(ops, lat, D.times(lat.shape[0], "interior"), 5, 16, det, "lattice")
    pts = torch.from_numpy(proc_uniform((D.F_N, 3), 4960, 1.5))
    check_backward(ops, pts, D.times(D.F_N, "interior"), 2, 16, det, f"two rounds N={D.F_N}")


@pytest.mark.parametrize("grads", ((True, False, False), (False, True, False), (False, False, True), (False, False, False)))
def test_backward_each_upstream_gradient_alone(ops, grads):
    got, ref = check_backward(ops, V.uniform_points(257), D.times(257, "interior"), 4, 16, False, f"upstream {grads}", grads=grads)
    if grads == (False, True, False):
        assert bool((got[:, 0] == 0).all())            # g_dp alone does not reach the rigidity grid
    if grads == (False, False, True):
        assert bool((got[:, 1:] == 0).all())           # g_rigidity alone does not reach the control points
    if not any(grads):
        assert bool((got == 0).all())


def test_deterministic_backward_is_independent_of_run_and_sample_order(ops):
    for n, N in ((4, 1000), (11, 1000), (2, D.F_N)):
        ctrl, rig = D.dyn_grids(16, n)
        pts = V.uniform_points(N) if N <= 1000 else torch.from_numpy(proc_uniform((N, 3), 4960, 1.5))
        t = D.times(N, "interior")
        order = torch.from_numpy(proc_uniform((N,), 4970, 1.0)).argsort()
        with mode(True):
            a, b, c = (run_backward(ops, pts, t, ctrl, rig, n, 16, order=o, want_ref=False)[0] for o in (None, None, order))
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), n
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), n


def test_a_too_small_deterministic_workspace_is_refused(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    S, n = 16, 4
    ctrl, rig = D.dyn_grids(S, n)
    pts, t = V.uniform_points(65).cuda(), D.times(65, "interior").cuda()
    _, dp, r = ops.dyn_voxel_warp(pts, t, ctrl.cuda(), rig.cuda(), n, GR)
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        with pytest.raises(_lib.NaError) as err:
            ops.dyn_voxel_warp_backward(pts, t, dp, r, S, n, GR, g_warped=torch.ones_like(pts))
        assert err.value.code == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 10 * S ** 3} bytes" in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0
    finally:
        config.set_deterministic(False)


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_backward_non_finite_coordinates(ops, det):
    """a NaN / Inf coordinate makes NaN exactly the entries the reference's clamped ids name -- at most 8 grid rows per bad sample in
    each gradient -- and every other entry stays inside its bound"""
    S, n = 16, 4
    pts, bad = bad_points()
    got, ref = check_backward(ops, pts, D.times(257, "interior"), n, S, det, "NaN / Inf coordinates")
    for cols in (got[:, :1], got[:, 1:]):
        assert 0 < int(torch.isnan(cols).any(dim=-1).sum()) <= 8 * len(bad)


# ------------------------------------------------------------------------------------------------------------ the position gradient
def check_pts_grad(ops, pts, den, rgb, what, gr=GR):
    N = pts.shape[0]
    g_raw = torch.from_numpy(proc_uniform((N, 4), 4980 + N, 1.0))
    ref, bound = D.sample_backward_pts_ref(pts, g_raw, den, rgb, gr)
    got = ops.voxel_sample_backward_pts(g_raw.cuda(), pts.cuda(), den.cuda(), rgb.cuda(), gr)
    assert got.shape == pts.shape
    ratio = V.worst_ratio(got, ref, bound)
    print(f"[voxel_sample_backward_pts {what}] worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return got


@pytest.mark.parametrize("S", (2, 4, 16, 64))
def test_position_gradient(ops, S):
    """uniform points at every ragged size; the lattice set (on the membership planes the derivative is the one of the cell pair the
    fp32 chain picked: a wrong one-sided derivative is an error of order 1 / voxel_len) and the zero set, on a random and on the
    index-encoding grid"""
    den, rgb = V.grid_values(S)
    for N in SIZES:
        check_pts_grad(ops, V.uniform_points(N), den, rgb, f"S={S} N={N}")
    for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points())):
        for gname, grids in (("random", (den, rgb)), ("index", V.index_grid(S))):
            check_pts_grad(ops, pts, *grids, f"S={S} {name} {gname} grid")


def test_position_gradient_non_finite_and_exact_points(ops):
    den, rgb = V.grid_values(16)
    pts, bad = bad_points()
    got = check_pts_grad(ops, pts, den, rgb, "NaN / Inf coordinates").cpu()
    clean = check_pts_grad(ops, V.uniform_points(257), den, rgb, "clean").cpu()
    rows = torch.isnan(got).any(dim=-1)
    assert torch.nonzero(rows).flatten().tolist() == bad and bool(torch.isnan(got[rows]).all()) and torch.equal(got[~rows], clean[~rows])
    p, _, S, gr = V.scatter_case("G")   # voxel_len 0.5, points on multiples of 1/8
    check_pts_grad(ops, p, *V.index_grid(S), "S=4 radius 1 exact points", gr=gr)


def test_autograd_returns_the_position_gradient_only_when_asked(ops):
    from nerf_atlas_amd import autograd as ag
    den, rgb = (x.cuda().requires_grad_(True) for x in V.grid_values(4))
    pts = V.uniform_points(65).cuda()
    g = torch.from_numpy(proc_uniform((65, 4), 4990, 1.0)).cuda()
    with mode(True):   # (fixed-point sums: the two scatters can be compared bit for bit)
        ag.VoxelSampleFn.apply(den, rgb, GR, pts, None, None).backward(g)
        plain = (den.grad.clone(), rgb.grad.clone())
        den.grad = rgb.grad = None
        p = pts.clone().requires_grad_(True)
        ag.VoxelSampleFn.apply(den, rgb, GR, p, None, None).backward(g)
    assert torch.equal(den.grad, plain[0]) and torch.equal(rgb.grad, plain[1])
    assert torch.equal(p.grad, ops.voxel_sample_backward_pts(g, pts, den.detach(), rgb.detach(), GR))


# ------------------------------------------------------------------------------------------------------------ arguments
def test_argument_checks_and_return_codes(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    S, n = 4, 4
    ctrl, rig = (x.cuda() for x in D.dyn_grids(S, n))
    den, rgb = (x.cuda() for x in V.grid_values(S))
    pts, t = V.uniform_points(8).cuda(), D.times(8, "interior").cuda()
    with pytest.raises(ValueError):
        ops.dyn_voxel_warp(pts.cpu(), t, ctrl, rig, n, GR)                                   # host tensors
    with pytest.raises(ValueError, match="float32"):
        ops.dyn_voxel_warp(pts.double(), t, ctrl, rig, n, GR)
    with pytest.raises(ValueError, match="one time per sample"):
        ops.dyn_voxel_warp(pts, t[:4], ctrl, rig, n, GR)
    with pytest.raises(ValueError, match="ctrl_pts_grid"):
        ops.dyn_voxel_warp(pts, t, ctrl, rig, 5, GR)                                         # 9 channels are spline 4
    with pytest.raises(ValueError, match="spline"):
        ops.dyn_voxel_warp(pts, t, ctrl, rig, 12, GR)
    with pytest.raises(ValueError, match="even"):
        ops.dyn_voxel_warp(pts, t, torch.zeros(3, 3, 3, 9).cuda(), torch.zeros(3, 3, 3, 1).cuda(), n, GR)
    w, dp, r = ops.dyn_voxel_warp(pts, t, ctrl, rig, n, GR)
    with pytest.raises(ValueError, match="even"):
        ops.dyn_voxel_warp_backward(pts, t, dp, r, 3, n, GR, g_warped=w)
    with pytest.raises(ValueError, match="g_dp"):
        ops.dyn_voxel_warp_backward(pts, t, dp, r, S, n, GR, g_dp=dp[:4])
    with pytest.raises(ValueError, match="rigidity"):
        ops.dyn_voxel_warp_backward(pts, t, dp, r[:4], S, n, GR, g_dp=dp)
    with pytest.raises(ValueError, match="g_raw"):
        ops.voxel_sample_backward_pts(torch.zeros(8, 3).cuda(), pts, den, rgb, GR)
    # non-contiguous inputs are copied, a gradient at an odd storage offset too: the same bits
    wide = torch.zeros(8, 6).cuda()
    wide[:, :3] = pts
    assert torch.equal(ops.dyn_voxel_warp(wide[:, :3], t, ctrl, rig, n, GR)[0], w)
    g = torch.from_numpy(proc_uniform((8, 4), 4991, 1.0)).cuda()
    flat = torch.zeros(33).cuda()
    flat[1:] = g.reshape(-1)
    assert torch.equal(ops.voxel_sample_backward_pts(flat[1:].reshape(8, 4), pts, den, rgb, GR), ops.voxel_sample_backward_pts(g, pts, den, rgb, GR))
    # the raw C ABI
    out = torch.zeros(8, 3).cuda()
    P, st = ops._ptr, ops._stream()
    for bad_n in (1, 12):
        assert lib.na_dyn_voxel_warp(P(pts), P(t), 8, P(ctrl), P(rig), S, bad_n, GR, P(out), None, None, st) == -3 and b"spline" in lib.na_last_error()
        assert lib.na_dyn_voxel_warp_backward(P(pts), P(t), 8, P(dp), P(r), P(w), None, None, S, bad_n, GR, P(ctrl), P(rig), st) == -3
    assert lib.na_dyn_voxel_warp(P(pts), P(t), 8, P(ctrl), P(rig), 3, n, GR, P(out), None, None, st) == -1 and b"resolution 3" in lib.na_last_error()
    assert lib.na_dyn_voxel_warp(P(pts), P(t), 8, P(ctrl), P(rig), 1026, n, GR, P(out), None, None, st) == -1
    assert lib.na_dyn_voxel_warp(P(pts), None, 8, P(ctrl), P(rig), S, n, GR, P(out), None, None, st) == -2
    assert lib.na_dyn_voxel_warp(P(pts), P(t), 8, P(ctrl), P(rig), S, n, GR, None, None, None, st) == -2
    assert lib.na_dyn_voxel_warp(P(pts), P(t), -1, P(ctrl), P(rig), S, n, GR, P(out), None, None, st) == -1
    assert lib.na_dyn_voxel_warp(None, None, 0, None, None, S, n, GR, None, None, None, st) == 0          # nothing to do
    assert lib.na_dyn_voxel_warp_backward(P(pts), P(t), 8, None, P(r), P(w), None, None, S, n, GR, P(ctrl), P(rig), st) == -2
    assert lib.na_dyn_voxel_warp_backward(P(pts), P(t), 8, P(dp), P(r), None, None, None, S, n, GR, None, None, st) == 0   # no upstream gradient
    assert lib.na_voxel_sample_backward_pts(P(pts), 8, P(den), P(rgb), P(g), 3, 3, GR, P(out), st) == -1
    assert lib.na_voxel_sample_backward_pts(P(pts), 8, P(den), P(rgb), P(g), S, 5, GR, P(out), st) == -3
    assert lib.na_voxel_sample_backward_pts(P(pts), 8, P(den), None, P(g), S, 3, GR, P(out), st) == -2
    torch.cuda.synchronize()
    assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------------------ model vs the reference
def build_model(g, device="cuda"):
    from nerf_atlas_amd import nerf, refl
    c = nerf.NeRFVoxel(resolution=int(g["S"]), t_near=float(g["near"]), t_far=float(g["far"]), steps=int(g["steps"]), bg=str(g["bg"]))
    c.set_refl(refl.Positional(act=str(g["act"]), latent_size=0, out_features=3))
    m = nerf.DynamicNeRFVoxel(c, spline=int(g["spline"]))
    m.load_state_dict(golden_params(g), strict=True)
    return m.to(device).eval()


class Spy:
    NAMES = ("dyn_voxel_warp", "dyn_voxel_warp_backward", "voxel_render", "voxel_sample", "voxel_sample_backward", "voxel_sample_backward_pts",
             "composite")

    def __init__(self, monkeypatch, ops):
        self.calls = {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, n, fn):
        def f(*a, **k):
            self.calls[n] += 1
            return fn(*a, **k)
        return f

    def used(self):
        return {k: v for k, v in self.calls.items() if v}


def close(got, g, what, tol=1e-4):
    for key, x in got.items():
        err = float((x.detach().cpu().double() - g[key + "64"]).abs().max())
        print(f"[{what}] {key} max |err| {err:.2e}")
        assert x.shape == g[key + "64"].shape and err <= tol, (what, key, err)


@pytest.mark.parametrize("name", ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11", "s64_n4"))
def test_model_matches_the_reference_on_both_routes(ops, monkeypatch, name):
    g = load_golden(f"g25_dyn_voxel_{name}")
    m = build_model(g)
    rays, t = g["rays"].cuda(), g["times"].cuda()
    spy = Spy(monkeypatch, ops)
    with torch.no_grad():
        out = m((rays, t))
    assert spy.used() == {"dyn_voxel_warp": 1, "voxel_render": 1}          # the eval route: warp + render
    assert torch.equal(m.ts.cpu(), g["ts"]) and m.rigid_dp.shape == m.dp.shape
    state = lambda o: dict(out=o, alpha=m.canonical.alpha, weights=m.canonical.weights, dp=m.dp, rigidity=m.rigidity)
    close(state(out), g, f"{name} eval route")
    spy.calls = {k: 0 for k in spy.calls}
    out_t = m((rays, t))                                                    # the operator route: gradients wanted
    assert spy.used() == {"dyn_voxel_warp": 1, "voxel_sample": 1, "composite": 1} and out_t.requires_grad
    close(state(out_t), g, f"{name} operator route")
    out_t.square().sum().backward()
    assert spy.calls["dyn_voxel_warp_backward"] == 1 and spy.calls["voxel_sample_backward_pts"] == 1 and spy.calls["voxel_sample_backward"] == 1
    if "g_dev" in g:
        # the project's 1e-4 bar, relative to the largest entry of the reference's fp64 gradient; the reference's own fp32 gradients'
        # distance from them (`g_dev`) is printed next to this build's
        params = dict(m.named_parameters())
        for i, key in enumerate(("canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid")):
            want, got = g["grad64." + key], params[key].grad
            err = float((got.cpu().double() - want).abs().max() / want.abs().max())
            print(f"[{name}] {key}: max |err| / largest entry {err:.2e} (the reference's own fp32: {float(g['g_dev'][i]):.2e})")
            assert got.shape == want.shape and err <= 1e-4, (name, key, err)


def test_offset_regularisers_reach_both_deformation_grids(ops):
    """--delta-x-decay and --offset-decay read model.dp / model.rigidity (train.py): their gradient enters DynVoxelWarpFn through its dp
    and rigidity outputs.  Against the restatement: the same two terms in fp64 torch on the model's dp / rigidity / weights give g_dp and
    g_rigidity, warp_backward_ref scatters them; within 1e-4 of the largest entry (the fp32 loss arithmetic in front of the kernel is
    torch's, so the project's model bar and not the scatter's bound)"""
    from nerf_atlas_amd import train
    g = load_golden("g25_dyn_voxel_s4_n4")
    m = build_model(g)
    m((g["rays"].cuda(), g["times"].cuda()))
    loss = 0.7 * m.dp.norm(dim=-1).mean() + 0.3 * train.offset_decay_term(m, 0.5)
    loss.backward()
    assert m.densities.grad is None and m.rgb.grad is None                 # neither term touches the canonical grids
    dp = m.dp.detach().cpu().double().requires_grad_(True)
    r = m.rigidity.detach().cpu().double().requires_grad_(True)
    w = m.canonical.weights.detach().cpu().double()
    reg = w[None, ..., None] * (torch.linalg.vector_norm(dp, dim=-1, keepdim=True).pow(2 - r) + 3e-3 * r)
    (0.7 * dp.norm(dim=-1).mean() + 0.3 * (1 / 100) ** 0.5 * reg.mean()).backward()
    pts = V.pts_of(g["rays"], g["ts"])
    tt = g["times"][None, :, None, None].expand(pts.shape[:-1]).reshape(-1)
    ref, _, _ = D.warp_backward_ref(pts.reshape(-1, 3), tt, m.dp.detach().cpu(), m.rigidity.detach().cpu(), 4, 4, float(g["grid_radius"]),
                                    g_dp=dp.grad, g_rigidity=r.grad)
    want_c, want_r = D.split_grids(ref, 4)
    for got, want, key in ((m.ctrl_pts_grid.grad, want_c, "ctrl_pts_grid"), (m.rigidity_grid.grad, want_r, "rigidity_grid")):
        err = float((got.cpu().double() - want).abs().max() / want.abs().max())
        print(f"[offset regularisers] {key}: max |err| / largest entry {err:.2e}")
        assert float(want.abs().max()) > 0 and err <= 1e-4, (key, err)


def test_a_training_step_lowers_the_loss(ops):
    """load_model -> NaAdam on the four grids: 20 steps on one batch of rays at two times towards a constant image; every grid
    receives a gradient"""
    from nerf_atlas_amd import train
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4", "--near", "2", "--far", "6",
                                 "--steps", "16"])
    torch.manual_seed(0)
    m = train.load_model(args, is_dyn=True).train()
    opt = train.NaAdam(m.parameters(), lr=5e-2)
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    t = torch.tensor([0.0, 1.0], device="cuda")
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (m((rays, t)) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("[dyn voxel train] loss", losses[0], "->", losses[-1])
    # a descent check, not a convergence claim: the loss falls, stays finite, and all four grids receive a gradient
    assert losses[-1] < losses[0] and all(l == l for l in losses)
    assert all(float(p.grad.abs().max()) > 0 for p in m.parameters())
