"""--model voxel on the GPU (csrc/voxel.hip): the gather, its scatter-add backward in both accumulation modes and the one-launch eval
route against tests/voxel_ref.py (membership fixed in fp32, everything behind it in fp64), and the model against the recorded
reference (g23).  Bounds: voxel_ref's derived ones for the two operators, the project's 1e-4 for everything composited."""
import contextlib

import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
from oracle.procedural import proc_param, proc_uniform

pytestmark = pytest.mark.gpu

NA_EWORKSPACE = -5   # include/nerf_atlas_amd.h
RESOLUTIONS = (2, 4, 16, 64)
SAMPLE_N = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 257: (1, 257), 1000: (8, 125)}   # N: (T, R) of the rays x ts form


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


def check_sample(ops, pts, den, rgb, what, grid_radius=V.GRID_RADIUS, **form):
    ref, mag = V.sample_ref(pts.reshape(-1, 3), den, rgb, grid_radius)
    got = ops.voxel_sample(den.cuda(), rgb.cuda(), grid_radius, **({"pts": pts.cuda()} if not form else {k: v.cuda() for k, v in form.items()}))
    assert got.shape[-1] == 4 and got.numel() == ref.numel()
    ratio = V.worst_ratio(got, ref, V.sample_bound(mag))
    print(f"[voxel_sample {what}] worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("S", RESOLUTIONS)
def test_sample_uniform_points_both_position_forms(ops, S):
    """(i) uniform in +-2.5 -- the inside and the extrapolated region -- at every ragged size, as explicit points and as rays x ts"""
    den, rgb = V.grid_values(S)
    for N, (T, R) in SAMPLE_N.items():
        check_sample(ops, V.uniform_points(N), den, rgb, f"S={S} N={N} pts")
        rays = torch.from_numpy(proc_uniform((R, 6), 4700 + N, 1.0))
        ts = torch.linspace(0.0, 2.5, T) if T > 1 else torch.tensor([1.25])
        pts = V.pts_of(rays, ts)
        assert pts.shape == (T, R, 3)
        check_sample(ops, pts, den, rgb, f"S={S} N={N} rays x ts", rays=rays, ts=ts)


@pytest.mark.parametrize("S", RESOLUTIONS)
def test_sample_lattice_and_zero_sets(ops, S):
    """(ii) the membership planes, the corners, the origin and (iii) tiny coordinates of both signs, on a random grid and on a grid whose
    entries encode their own index (a wrong cell is an error of order 1 there)"""
    for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points())):
        for gname, (den, rgb) in (("random", V.grid_values(S)), ("index", V.index_grid(S))):
            check_sample(ops, pts, den, rgb, f"S={S} {name} {gname} grid")


def test_sample_on_power_of_two_voxels(ops):
    """voxel_len = 0.5: every point of scatter case G sits exactly on a plane or a quarter of a cell -- exact arithmetic in the chain"""
    p, _, S, gr = V.scatter_case("G")
    den, rgb = V.index_grid(S)
    check_sample(ops, p, den, rgb, "S=4 radius 1 exact points", grid_radius=gr)


def test_sample_non_finite_coordinates_are_nan_rows_and_nothing_else(ops):
    S = 16
    den, rgb = V.grid_values(S)
    pts = V.uniform_points(257).clone()
    bad = {5: (1, float("nan")), 70: (0, float("inf")), 200: (2, float("-inf")), 256: (0, float("nan"))}
    for n, (a, v) in bad.items():
        pts[n, a] = v
    got = ops.voxel_sample(den.cuda(), rgb.cuda(), V.GRID_RADIUS, pts=pts.cuda()).cpu()
    nan_rows = torch.isnan(got).any(dim=-1)
    assert sorted(torch.nonzero(nan_rows).flatten().tolist()) == sorted(bad) and bool(torch.isnan(got[nan_rows]).all())
    check_sample(ops, pts, den, rgb, "S=16 NaN / Inf coordinates")


def test_sample_argument_checks(ops):
    from nerf_atlas_amd import _lib
    den, rgb = V.grid_values(4)
    pts = V.uniform_points(8).cuda()
    with pytest.raises(ValueError):
        ops.voxel_sample(den, rgb, 1.3, pts=pts.cpu())                             # host tensors
    with pytest.raises(ValueError, match="even"):
        ops.voxel_sample(torch.zeros(3, 3, 3, 1).cuda(), torch.zeros(3, 3, 3, 3).cuda(), 1.3, pts=pts)
    with pytest.raises(_lib.NaError) as err:
        ops.voxel_sample(den.cuda(), torch.zeros(4, 4, 4, 5).cuda(), 1.3, pts=pts)  # C = 5: no kernel
    assert err.value.code == -3
    lib = _lib.load()
    raw = torch.zeros(8, 4).cuda()
    rc = lib.na_voxel_sample(ops._ptr(pts), None, 8, None, 1, ops._ptr(den.cuda()), ops._ptr(rgb.cuda()), 3, 3, 1.3, ops._ptr(raw), ops._stream())
    assert rc == -1 and b"resolution 3" in lib.na_last_error()
    rc = lib.na_voxel_sample(None, None, 8, None, 1, ops._ptr(den.cuda()), ops._ptr(rgb.cuda()), 4, 3, 1.3, ops._ptr(raw), ops._stream())
    assert rc == -2


# ------------------------------------------------------------------------------------------------------------ scatter
def scatter(ops, name, order=None):
    p, g, S, gr = V.scatter_case(name)
    if order is not None:
        p, g = p[order], g[order]
    gd, gc = ops.voxel_sample_backward(g.cuda(), S, gr, pts=p.cuda())
    assert gd.shape == (S, S, S, 1) and gc.shape == (S, S, S, 3)
    return torch.cat([gd, gc], dim=-1).reshape(S ** 3, 4).cpu()


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("name", V.SCATTER_CASES)
def test_scatter_every_entry_inside_its_bound(ops, name, det):
    ref, mag, cnt = V.scatter_reference(name)
    with mode(det):
        got = scatter(ops, name)
    ratio = V.worst_ratio(got, ref, V.scatter_bound(ref, mag, cnt, det))
    print(f"[voxel scatter {name} {'det' if det else 'atomic'}] worst |err| / bound {ratio:.3f}, most addends in one entry {int(cnt.max())}")
    assert ratio <= 1.0, (name, det, ratio)
    if name == "G":   # exact arithmetic: bitwise the fp64 sum
        assert torch.equal(got.double(), ref)


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_scatter_rays_form_and_non_finite_coordinates(ops, det):
    """positions formed in the kernel; a NaN and an Inf coordinate make exactly the entries NaN that the reference's clamped ids name"""
    S, T, R = 16, 9, 29
    rays = torch.from_numpy(proc_uniform((R, 6), 4710, 1.0)).clone()
    rays[3, 1], rays[17, 5] = float("nan"), float("inf")
    ts = torch.linspace(0.1, 2.5, T)
    g = torch.from_numpy(proc_uniform((T, R, 4), 4711, 1.0))
    pts = V.pts_of(rays, ts).reshape(-1, 3)
    ref, mag, cnt = V.scatter_ref(pts, g.reshape(-1, 4), S)
    with mode(det):
        gd, gc = ops.voxel_sample_backward(g.cuda(), S, V.GRID_RADIUS, rays=rays.cuda(), ts=ts.cuda())
    got = torch.cat([gd, gc], dim=-1).reshape(S ** 3, 4).cpu()
    assert 0 < int(torch.isnan(ref[:, 0]).sum()) < S ** 3 // 8
    assert V.worst_ratio(got, ref, V.scatter_bound(ref, mag, cnt, det)) <= 1.0


def test_scatter_takes_a_gradient_at_an_odd_storage_offset(ops):
    """g_raw as a contiguous view one float into its storage (not 16-byte aligned): ops copies it, the result is the aligned one's"""
    p, g, S, gr = V.scatter_case("D257")
    flat = torch.zeros(g.numel() + 1).cuda()
    flat[1:] = g.reshape(-1).cuda()
    view = flat[1:].reshape(g.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    with mode(True):
        a = ops.voxel_sample_backward(g.cuda(), S, gr, pts=p.cuda())
        b = ops.voxel_sample_backward(view, S, gr, pts=p.cuda())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        ops.voxel_sample_backward(g.cuda()[:-1], S, gr, pts=p.cuda())


def test_deterministic_scatter_is_independent_of_run_and_sample_order(ops):
    for name in ("D1000", "L", "F"):
        n = V.scatter_case(name)[0].shape[0]
        order = torch.from_numpy(proc_uniform((n,), 4720, 1.0)).argsort()
        with mode(True):
            a, b, c = scatter(ops, name), scatter(ops, name), scatter(ops, name, order)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name


def test_a_too_small_deterministic_workspace_is_refused(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    p, g, S, gr = V.scatter_case("D65")
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        with pytest.raises(_lib.NaError) as err:
            ops.voxel_sample_backward(g.cuda(), S, gr, pts=p.cuda())
        assert err.value.code == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 4 * S ** 3} bytes" in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0
    finally:
        config.set_deterministic(False)


# ------------------------------------------------------------------------------------------------------------ fused render
RENDER_T = (1, 2, 63, 64, 65, 130)
RENDER_R = {1: (1,), 63: (3, 3, 7), 65: (65,), 257: (257,)}
ACTS = ("upshifted", "thin", "leaky_relu")
BGS = ("black", "white", "random")


def render_ref(rays, ts, den, rgb, act, bg, rand=None):
    pts = V.pts_of(rays, ts)
    raw, _ = V.sample_ref(pts.reshape(-1, 3), den, rgb)
    return V.composite_ref(raw.reshape(pts.shape[:-1] + (4,)), ts, rays, act, bg, rand)


def close(got, ref, what, tol=1e-4):
    for g, r, n in zip(got, ref, ("out", "alpha", "weights")):
        err = float((g.detach().cpu().double() - r).abs().max())
        print(f"[{what}] {n} max |err| {err:.2e}")
        assert g.shape == r.shape and err <= tol, (what, n, err)


@pytest.mark.parametrize("T", RENDER_T)
def test_render_one_launch(ops, T):
    """every ray count (one as a [B,H,W] batch) x the three backgrounds x the three activations, cycled so that each T sees all of them;
    explicit points give the same bits as points formed in the kernel"""
    S = 16 if T != 64 else 64
    den, rgb = V.grid_values(S)
    dc, rc = den.cuda(), rgb.cuda()
    ts = torch.linspace(2.0, 6.0, T) if T > 1 else torch.tensor([4.0])
    for i, (R, shape) in enumerate(RENDER_R.items()):
        act, bg = ACTS[(i + T) % 3], BGS[(i + T // 2) % 3]
        rays = V.generic_rays(shape, 4730 + R)
        rand = torch.from_numpy(proc_uniform(shape + (1,), 4740 + R, 0.5)) + 0.5 if bg == "random" else None
        ref = render_ref(rays, ts, den, rgb, act, bg, rand)
        got = ops.voxel_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, "black" if bg == "random" else bg)
        viapts = ops.voxel_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, "black" if bg == "random" else bg, pts=V.pts_of(rays, ts).cuda())
        for a, b in zip(got, viapts):
            assert torch.equal(a, b)
        if bg == "random":
            ops.sky_random(got[2], rand.cuda(), got[0])
        close(got, ref, f"voxel_render S={S} T={T} R={R} {act} {bg}")
        # the operator route (what training runs) on the same shapes, the same bar
        raw = ops.voxel_sample(dc, rc, V.GRID_RADIUS, rays=rays.cuda(), ts=ts.cuda())
        via_ops = ops.composite(raw[..., 0].contiguous(), ops.sigmoid(raw[..., 1:].contiguous(), act), ts.cuda(), rays.cuda(), bg=bg,
                                rand=None if rand is None else rand.cuda())
        close(via_ops, ref, f"operator route S={S} T={T} R={R} {act} {bg}")
    out_only = ops.voxel_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, "white", want_weights=False)
    assert out_only[1] is None and out_only[2] is None and out_only[0].shape == shape + (3,)


def build_model(g, device="cuda"):
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=int(g["S"]), t_near=float(g["near"]), t_far=float(g["far"]), steps=int(g["steps"]), bg=str(g["bg"]))
    m.set_refl(refl.Positional(act=str(g["act"]), latent_size=0, out_features=3))
    m.load_state_dict(golden_params(g), strict=True)
    return m.to(device).eval()


class Spy:
    def __init__(self, monkeypatch, ops, names=("voxel_render", "voxel_sample", "voxel_sample_backward", "composite")):
        self.calls = {n: 0 for n in names}
        for n in names:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, n, fn):
        def f(*a, **k):
            self.calls[n] += 1
            return fn(*a, **k)
        return f


# ------------------------------------------------------------------------------------------------------------ model vs the reference
@pytest.mark.parametrize("name", ("s64_black", "s64_white", "s16_ragged", "s4", "s2"))
def test_model_matches_the_reference_on_both_routes(ops, monkeypatch, name):
    g = load_golden(f"g23_voxel_{name}")
    m = build_model(g)
    rays = g["rays"].cuda()
    ref = (g["out64"], g["alpha64"], g["weights64"])
    spy = Spy(monkeypatch, ops)
    with torch.no_grad():
        out = m(rays)
    assert spy.calls == {"voxel_render": 1, "voxel_sample": 0, "voxel_sample_backward": 0, "composite": 0}
    assert torch.equal(m.ts.cpu(), g["ts"])
    close((out, m.alpha, m.weights), ref, f"{name} eval route")
    # explicit positions through from_pts: the same launch
    with torch.no_grad():
        pts = V.pts_of(g["rays"], g["ts"]).cuda()
        out_p = m.from_pts(pts, m.ts, rays[..., :3], rays[..., 3:], rays=rays)
    assert torch.equal(out_p, out) and spy.calls["voxel_render"] == 2
    # the operator route: gradients wanted
    spy.calls = {k: 0 for k in spy.calls}
    out_t = m(rays)
    assert spy.calls == {"voxel_render": 0, "voxel_sample": 1, "voxel_sample_backward": 0, "composite": 1} and out_t.requires_grad
    close((out_t, m.alpha, m.weights), ref, f"{name} operator route")
    out_t.square().sum().backward()
    assert spy.calls["voxel_sample_backward"] == 1
    if "g_densities64" in g:
        # the project's 1e-4 bar, relative to the largest entry of the reference's fp64 gradient (the reference's own fp32 gradients are
        # up to 2.0e-6 off them: `g_dev` in the fixture, printed next to this build's)
        for got, key in ((m.densities.grad, "g_densities64"), (m.rgb.grad, "g_rgb64")):
            want = g[key]
            err = float((got.cpu().double() - want).abs().max() / want.abs().max())
            print(f"[{name}] {key}: max |err| / largest entry {err:.2e} (the reference's own fp32: {g['g_dev'].tolist()})")
            assert got.shape == want.shape and err <= 1e-4, (name, key, err)


def test_model_random_background_and_training_mode(ops, monkeypatch):
    """bg random: the one-launch route composites against black and adds the sky behind it (two launches), like the operator route does in
    its compositing kernel; training mode draws stratified steps and takes the operator route even without gradients"""
    from nerf_atlas_amd import render
    g = load_golden("g23_voxel_s16_ragged")
    m = build_model(g)
    m.set_bg("random")
    p = golden_params(g)
    rays = g["rays"]
    spy = Spy(monkeypatch, ops)
    with torch.no_grad():
        out = m(rays.cuda())
    assert spy.calls["voxel_render"] == 1 and spy.calls["composite"] == 0
    ref = render_ref(rays, g["ts"], p["densities"], p["rgb"], str(g["act"]), "random", m.bg_rand.cpu())
    close((out, m.alpha, m.weights), ref, "bg random, eval route")
    out_t = m(rays.cuda())
    ref = render_ref(rays, g["ts"], p["densities"], p["rgb"], str(g["act"]), "random", m.bg_rand.cpu())
    close((out_t, m.alpha, m.weights), ref, "bg random, operator route")
    assert render.depth_map(m).shape == rays.shape[:-1] + (1,) and render.alpha_map(m).shape == rays.shape[:-1] + (1,)
    m.train()
    spy.calls = {k: 0 for k in spy.calls}
    m.set_bg("black")
    with torch.no_grad():
        out_n = m(rays.cuda())
    assert spy.calls["voxel_render"] == 0 and spy.calls["voxel_sample"] == 1 and not torch.equal(m.ts.cpu(), g["ts"])
    ref = render_ref(rays, m.ts.cpu(), p["densities"], p["rgb"], str(g["act"]), "black")
    close((out_n, m.alpha, m.weights), ref, "training mode, stratified steps")


def test_a_training_step_lowers_the_loss(ops):
    """load_model -> NaAdam on the two grids: 20 steps on one batch of rays towards a constant image"""
    from nerf_atlas_amd import train
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos", "--near", "2", "--far", "6", "--steps", "16"])
    torch.manual_seed(0)
    m = train.load_model(args).train()
    opt = train.NaAdam(m.parameters(), lr=5e-2)
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (m(rays) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("[voxel train] loss", losses[0], "->", losses[-1])
    assert losses[-1] < 0.5 * losses[0] and all(l == l for l in losses)


# ------------------------------------------------------------------------------------------------------------ training against the reference
def test_training_tracks_the_reference(tmp_path):
    """tests/golden/train_parity_voxel.json: the reference's runner.main on the analytic scene (tools/ref_train_fixture.py voxel), replayed
    through this build's loaders, kernels and training loop with the reference's random stream.  The recipe is not chaotic (the
    reference's own 8- and 2-thread runs differ by 1.5e-8 in the worst loss and 1e-6 dB): the strict bars of tests/test_gpu_train.py --
    first 10 losses within 2e-4, the smoothed curve within 0.1 of its maximum, every test view within 0.01 dB (there is no GEMM in this
    model: the exact-fp32 bar)."""
    import json
    import os
    import numpy as np
    from conftest import GOLDEN
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_voxel.json")))
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")])
    assert args.epochs == len(fx["losses"]) == 200 and args.model == "voxel"

    def procedural_init(model):
        with torch.no_grad():
            for k, v in model.state_dict().items():
                v.copy_(torch.from_numpy(proc_param(k, tuple(v.shape))))
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        res = T.fit(args, replay_reference_rng=True, init=procedural_init)
    finally:
        config.set_deterministic(False)
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    sm = lambda v: np.convolve(v, np.ones(20) / 20, mode="valid")
    dev = np.abs(sm(got) - sm(ref)).max() / sm(ref).max()
    print(f"[voxel parity] |loss - ref| first 10 {np.abs(got[:10] - ref[:10]).max():.2e}, all 200 {np.abs(got - ref).max():.2e}; smoothed "
          f"curve {dev:.2e}; test PSNR {np.round(res['test_psnr'], 4).tolist()} vs {np.round(fx['test_psnr'], 4).tolist()} ({d.max():.5f} dB)")
    assert np.abs(got[:10] - ref[:10]).max() <= 2e-4 and dev <= 0.1 and d.max() <= 0.01
    assert ref[-20:].mean() < 0.5 * ref[:20].mean(), "the recipe must actually learn"


def test_runner_cli_trains_and_writes_results(tmp_path):
    """python -m nerf_atlas_amd.runner --model voxel --refl-kind pos (`make voxel` with the head that has a voxel form)"""
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2", "--steps", "24",
                       "--epochs", "12", "--quiet", "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2", "--outdir", str(out),
                       "--save", str(tmp_path / "m.pt")])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12
    sd = torch.load(tmp_path / "m.pt")
    assert sorted(sd) == ["densities", "rgb"] and tuple(sd["rgb"].shape) == (64, 64, 64, 3)
