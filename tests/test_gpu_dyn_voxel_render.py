"""The voxel D-NeRF's one-launch test renderer on the GPU (csrc/dyn_voxel_render.hip, na_dyn_voxel_render): bit for bit against the launches
it replaces (na_compute_pts -> na_dyn_voxel_warp -> na_voxel_render(pts = warped) -> na_integrate x 4), its optional outputs, a
non-finite ray, its argument checks, tests/dyn_voxel_maps_ref.py's fp64 restatement under that file's derived bounds, the recorded
reference (g25) under the project's 1e-4 bar, the routes through render.py and the command line."""
import itertools

import numpy as np
import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
import dyn_voxel_ref as D
import dyn_voxel_maps_ref as M

pytestmark = pytest.mark.gpu

GR = V.GRID_RADIUS
SIZES = (1, 63, 64, 65, 257, 1000)
STEPS = (1, 2, 7, 24)          # 1: the 1e10 step alone; 2, 7 and 24: no multiples of the chunk of steps gathered ahead (16)
ACTS = ("upshifted", "thin")
OPTIONAL = ("depth", "acc", "flow", "rigidity", "alpha", "weights")
NA_EINVAL, NA_ENULL, NA_EUNSUPPORTED = -1, -2, -3   # include/nerf_atlas_amd.h


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def build_model(g, device="cuda"):
    """the g25 fixture's model with its recorded parameters, in eval mode"""
    from nerf_atlas_amd import nerf, refl
    c = nerf.NeRFVoxel(resolution=int(g["S"]), t_near=float(g["near"]), t_far=float(g["far"]), steps=int(g["steps"]), bg=str(g["bg"]))
    c.set_refl(refl.Positional(act=str(g["act"]), latent_size=0, out_features=3))
    m = nerf.DynamicNeRFVoxel(c, spline=int(g["spline"]))
    m.load_state_dict(golden_params(g), strict=True)
    return m.to(device).eval()


def rays_of(R, seed=4500):
    """voxel_ref.generic_rays (the first samples of every ray outside the grid), every third ray turned round: it walks away from the
    grid, through the extrapolated region only"""
    rays = V.generic_rays((R,), seed + R).clone()
    rays[2::3, 3:] = -rays[2::3, 3:]
    return rays


def times_of(R):
    """one launch holds rays at t = 0, t = 1 and interior times"""
    t = D.times(R, "interior").clone()
    t[0::3] = 0.0
    t[1::3] = 1.0
    return t


def steps_of(T, lo=2.0, hi=6.0):
    return torch.linspace(lo, hi, T) if T > 1 else torch.tensor([lo])


def grids_of(S, n, index=False):
    """(densities, rgb, ctrl_pts_grid, rigidity_grid) on the GPU"""
    canon = V.index_grid(S) if index else V.grid_values(S)
    dyn = D.index_dyn_grids(S, n) if index else D.dyn_grids(S, n)
    return tuple(x.cuda() for x in canon + dyn)


def composition(ops, rays, t, ts, grids, n, act, bg, gr=GR):
    """the launches the kernel replaces, as DynamicNeRFVoxel.forward + render.depth_map / alpha_map / flow_map / rigidity_map run them"""
    den, rgb, ctrl, rig = grids
    T, R = ts.shape[0], rays.shape[0]
    pts = ops.compute_pts(rays, ts)
    warped, dp, r = ops.dyn_voxel_warp(pts, t[None, :].expand(T, R).contiguous(), ctrl, rig, n, gr)
    out, alpha, weights = ops.voxel_render(rays, ts, den, rgb, gr, act, bg, True, pts=warped)
    ones = torch.ones(T, R, 1, device="cuda")
    ones[-1] = 0
    return dict(rgb=out, alpha=alpha, weights=weights, depth=ops.integrate(weights, ts[:, None, None].expand(T, R, 1).contiguous()),
                acc=ops.integrate(weights, ones), flow=ops.integrate(weights, (dp * r[..., None]).contiguous()),
                rigidity=ops.integrate(weights, r[..., None].contiguous()))


def fused(ops, rays, t, ts, grids, n, act, bg, gr=GR, want=OPTIONAL):
    den, rgb, ctrl, rig = grids
    return ops.dyn_voxel_render(rays, t, ts, den, rgb, ctrl, rig, n, gr, act, bg, want=want)


def assert_same_bits(got, ref, what):
    assert set(got) == set(ref) == set(M.OUTPUTS)
    for k in M.OUTPUTS:
        assert not bool(torch.isnan(ref[k]).any()), (what, k)
        assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (what, k, float((got[k] - ref[k]).abs().max()))


# ------------------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("n", D.SPLINES)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_bit_for_bit_against_the_launches_it_replaces(ops, S, n):
    grids = grids_of(S, n)
    for i, T in enumerate(STEPS):
        R = SIZES[(i + n + S) % len(SIZES)]
        act, bg = ACTS[(i + n) % 2], ("black", "white")[(i + S // 2) % 2]
        rays, t, ts = rays_of(R).cuda(), times_of(R).cuda(), steps_of(T).cuda()
        assert_same_bits(fused(ops, rays, t, ts, grids, n, act, bg), composition(ops, rays, t, ts, grids, n, act, bg),
                         f"S={S} n={n} T={T} R={R} {act} {bg}")


def test_every_ragged_size_and_both_backgrounds(ops):
    """every R of the list at one grid, T = 7 (half a chunk of steps), both backgrounds and both activation kinds"""
    grids = grids_of(4, 4)
    ts = steps_of(7).cuda()
    for R, act, bg in itertools.product(SIZES, ACTS, ("black", "white")):
        rays, t = rays_of(R).cuda(), times_of(R).cuda()
        assert_same_bits(fused(ops, rays, t, ts, grids, 4, act, bg), composition(ops, rays, t, ts, grids, 4, act, bg), f"R={R} {act} {bg}")


def test_bit_for_bit_at_the_recipes_shape(ops):
    """make dyn_voxel: S 64, spline 4, 80 steps; 1000 rays"""
    grids = grids_of(64, 4)
    rays, t, ts = rays_of(1000).cuda(), times_of(1000).cuda(), steps_of(80).cuda()
    assert_same_bits(fused(ops, rays, t, ts, grids, 4, "upshifted", "black"), composition(ops, rays, t, ts, grids, 4, "upshifted", "black"),
                     "S=64 n=4 T=80 R=1000")


# ------------------------------------------------------------------------------------------------------------ optional outputs
def call_abi(ops, rays, t, ts, grids, S, n, bufs, act="upshifted", bg="black", C=3, T=None, R=None, gr=GR):
    """the raw C entry point; bufs: name -> tensor or None for `out` and the six optional outputs"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    P = ops._ptr
    den, rgb, ctrl, rig = grids
    return lib.na_dyn_voxel_render(P(rays), P(t), rays.shape[0] if R is None else R, P(ts), ts.shape[0] if T is None else T, P(den), P(rgb),
                                   P(ctrl), P(rig), S, C, n, gr, ops.SIGMOID[act], ops.BG[bg], P(bufs.get("rgb")),
                                   *(P(bufs.get(k)) for k in OPTIONAL), ops._stream())


def test_every_pattern_of_null_optional_outputs(ops):
    S, n, R, T = 16, 5, 257, 7
    grids = grids_of(S, n)
    rays, t, ts = rays_of(R).cuda(), times_of(R).cuda(), steps_of(T).cuda()
    full = fused(ops, rays, t, ts, grids, n, "upshifted", "white")
    for mask in range(64):
        names = [k for i, k in enumerate(OPTIONAL) if mask >> i & 1]
        bufs = {k: torch.full_like(full[k], -7.0) for k in names + ["rgb"]}
        assert call_abi(ops, rays, t, ts, grids, S, n, bufs, bg="white") == 0
        for k, v in bufs.items():
            assert torch.equal(v, full[k]), (mask, k)


# ------------------------------------------------------------------------------------------------------------ a non-finite ray
@pytest.mark.parametrize("value", (float("inf"), float("nan")))
def test_a_non_finite_ray_is_nan_and_touches_nothing_else(ops, value):
    S, n, T = 16, 4, 7
    grids = grids_of(S, n)
    rays, t, ts = rays_of(65).cuda(), times_of(65).cuda(), steps_of(T).cuda()
    rays[40, 1] = value
    keep = torch.tensor([i for i in range(65) if i != 40], device="cuda")
    got = fused(ops, rays, t, ts, grids, n, "upshifted", "white")
    clean = fused(ops, rays[keep].contiguous(), t[keep].contiguous(), ts, grids, n, "upshifted", "white")
    for k in M.OUTPUTS:
        g, c = (got[k].movedim(1, 0), clean[k].movedim(1, 0)) if k in M.PER_SAMPLE else (got[k], clean[k])
        assert bool(torch.isnan(g[40]).all()), k
        assert torch.equal(g[keep], c), k


# ------------------------------------------------------------------------------------------------------------ arguments
def test_argument_checks_and_return_codes(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    S, n, R, T = 4, 4, 8, 3
    grids = grids_of(S, n)
    rays, t, ts = rays_of(R).cuda(), times_of(R).cuda(), steps_of(T).cuda()
    out = torch.zeros(R, 3, device="cuda")
    bufs = dict(rgb=out)
    err = lambda: lib.na_last_error().decode()
    for bad_n in (1, 12):
        assert call_abi(ops, rays, t, ts, grids, S, bad_n, bufs) == NA_EUNSUPPORTED and f"n_ctrl {bad_n}" in err()
    assert call_abi(ops, rays, t, ts, grids, 3, n, bufs) == NA_EINVAL and "na_dyn_voxel_render: resolution 3" in err()
    assert call_abi(ops, rays, t, ts, grids, 1026, n, bufs) == NA_EINVAL and "resolution 1026" in err()
    assert call_abi(ops, rays, t, ts, grids, S, n, bufs, C=4) == NA_EUNSUPPORTED and "C = 4" in err()
    assert call_abi(ops, rays, t, ts, grids, S, n, bufs, T=0) == NA_EINVAL and "T=0" in err()
    assert call_abi(ops, rays, t, ts, grids, S, n, bufs, R=-1) == NA_EINVAL and "R=-1" in err()
    for i, name in enumerate(("densities", "rgb", "ctrl_pts_grid", "rigidity_grid")):
        g = list(grids)
        g[i] = None
        assert call_abi(ops, rays, t, ts, g, S, n, bufs) == NA_ENULL and f"null pointer {name}" in err()
    assert call_abi(ops, None, t, ts, grids, S, n, bufs, R=R) == NA_ENULL and "null pointer rays" in err()
    assert call_abi(ops, rays, None, ts, grids, S, n, bufs) == NA_ENULL and "null pointer t_ray" in err()
    assert call_abi(ops, rays, t, None, grids, S, n, bufs, T=T) == NA_ENULL and "null pointer ts" in err()
    assert call_abi(ops, rays, t, ts, grids, S, n, {}) == NA_ENULL and "null pointer out" in err()
    assert call_abi(ops, None, None, None, (None,) * 4, S, n, {}, R=0, T=T) == 0                       # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    # the Python layer: shapes, dtypes, devices, names
    den, rgb, ctrl, rig = grids
    run = lambda **kw: ops.dyn_voxel_render(**dict(dict(rays=rays, t=t, ts=ts, densities=den, rgb=rgb, ctrl_pts_grid=ctrl, rigidity_grid=rig,
                                                        spline=n, grid_radius=GR), **kw))
    with pytest.raises(ValueError):
        run(rays=rays.cpu())
    with pytest.raises(ValueError, match="float32"):
        run(t=t.double())
    with pytest.raises(ValueError, match="one time per ray"):
        run(t=t[:4])
    with pytest.raises(ValueError, match="ctrl_pts_grid"):
        run(spline=5)
    with pytest.raises(ValueError, match="deformation grids"):
        run(ctrl_pts_grid=torch.zeros(2, 2, 2, 9, device="cuda"), rigidity_grid=torch.zeros(2, 2, 2, 1, device="cuda"))
    with pytest.raises(ValueError, match="normals"):
        run(want=("depth", "normals"))
    with pytest.raises(NotImplementedError):
        run(bg="random")
    res = run(want=())
    assert set(res) == {"rgb"}
    wide = torch.zeros(R, 8, device="cuda")
    wide[:, :6] = rays
    assert torch.equal(run(rays=wide[:, :6], want=())["rgb"], res["rgb"])                               # a non-contiguous view is copied


# ------------------------------------------------------------------------------------------------------------ against fp64
def check_fp64(ops, rays, t, ts, S, n, index, act, bg, what):
    grids = grids_of(S, n, index)
    ref = M.render_ref(rays, t, ts, *(x.cpu() for x in grids), n, GR, act, bg)
    got = fused(ops, rays.cuda(), t.cuda(), ts.cuda(), grids, n, act, bg)
    ratios = {k: V.worst_ratio(got[k], ref[k], ref["b_" + k]) for k in M.OUTPUTS}
    print(f"[dyn_voxel_render {what}] worst |err| / bound:", {k: round(v, 3) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), (what, ratios)


@pytest.mark.parametrize("S", (2, 4, 16))
def test_inside_the_fp64_bounds(ops, S):
    """ts starts at 0, so the first sample of every ray IS its origin: uniform origins (the inside and the extrapolated region) and the
    lattice set (the membership planes of the deformation lookup; at t = 0 the warped point is the same lattice point and the canonical
    lookup sits on them too), on random grids and on the index-encoding grids, where a wrong cell or channel is an error of order 1"""
    ts = torch.linspace(0.0, 1.5, 7)
    for name, o in (("uniform", V.uniform_points(257)), ("lattice", V.lattice_points(S))):
        R = o.shape[0]
        rays = torch.cat([o, V.generic_rays((R,), 4520 + S)[:, 3:]], dim=-1)
        for n, index, act, bg in ((4, False, "upshifted", "white"), (5, True, "thin", "black"), (11, False, "thin", "white"), (2, True, "upshifted", "black")):
            check_fp64(ops, rays, times_of(R), ts, S, n, index, act, bg, f"S={S} n={n} {name} origins, {'index' if index else 'random'} grids")


# ------------------------------------------------------------------------------------------------------------ the recorded reference
@pytest.mark.parametrize("name", ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11", "s64_n4"))
def test_forward_maps_matches_the_recorded_reference(ops, name):
    """rgb within 1e-4 of the reference's fp64 out; every map within 1e-4 of the reference's fp64 maps, its own volumetric_integrate of the
    fixture's fp64 arrays"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    m = build_model(g)
    with torch.no_grad():
        got = m.forward_maps((g["rays"].cuda(), g["times"].cuda()), acc=True)
    want = dict(M.reference_maps(g["weights64"], g["ts"], g["dp64"], g["rigidity64"]), rgb=g["out64"])
    assert set(got) == set(want)
    for k, x in got.items():
        err = float((x.cpu().double() - want[k]).abs().max())
        print(f"[forward_maps {name}] {k} max |err| {err:.2e}")
        assert x.shape == want[k].shape and err <= 1e-4, (name, k, err)


# ------------------------------------------------------------------------------------------------------------ routes
class Spy:
    NAMES = ("dyn_voxel_render", "dyn_voxel_warp", "voxel_render", "integrate", "compute_pts")

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
        used = {k: v for k, v in self.calls.items() if v}
        self.calls = {k: 0 for k in self.calls}
        return used


def camera():
    from nerf_atlas_amd import cameras
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 4.0]]])
    return cameras.NeRFCamera(cam_to_world=c2w, focal=14.0).cuda()


def test_render_frame_maps_equals_the_generic_route(ops, monkeypatch):
    """a 12 x 12 frame in 5-pixel tiles (ragged last tiles): one launch per tile against render() + the four map functions, bit for bit"""
    from nerf_atlas_amd import render
    m, cam = build_model(load_golden("g25_dyn_voxel_s16_n11")), camera()
    t = torch.tensor([0.35], device="cuda")
    spy = Spy(monkeypatch, ops)
    want = ("depth", "flow", "rigidity", "acc")
    one = render.render_frame_maps(m, cam, 12, 5, t, want)
    assert spy.used() == {"dyn_voxel_render": 9}
    gen = render.render_frame_maps(m, cam, 12, 5, t, want, generic=True)
    assert spy.used() == {"compute_pts": 9, "dyn_voxel_warp": 9, "voxel_render": 9, "integrate": 36}
    assert set(one) == set(gen) == {"rgb"} | set(want)
    for k in one:
        assert one[k].shape == (12, 12, render.MAP_CHANNELS.get(k, 3)) and torch.equal(one[k], gen[k]), k
    assert float(one["acc"].max()) > 0 and float(one["flow"].abs().max()) > 0
    sub = render.render_frame_maps(m, cam, 12, 5, t, ("depth",))
    assert set(sub) == {"rgb", "depth"} and torch.equal(sub["depth"], one["depth"]) and torch.equal(sub["rgb"], one["rgb"])
    static = render.render_frame_maps(m.canonical, cam, 12, 5, None, want)          # a static model has no flow or rigidity: omitted
    assert set(static) == {"rgb", "depth", "acc"}


def test_render_over_time_equals_the_generic_route(ops, monkeypatch):
    from nerf_atlas_amd import render
    m, cam = build_model(load_golden("g25_dyn_voxel_s4_n4")), camera()
    times = torch.tensor([0.0, 0.5, 1.0])
    spy = Spy(monkeypatch, ops)
    one = render.render_over_time(m, cam, 12, 5, times, with_alpha=True)
    assert spy.used() == {"dyn_voxel_render": 27}
    gen = render.render_over_time(m, cam, 12, 5, times, with_alpha=True, generic=True)
    assert [i for i, _ in one] == [i for i, _ in gen] == [0, 1, 2]
    for (_, a), (_, b) in zip(one, gen):
        assert a.shape == (12, 12, 4) and torch.equal(a, b)
    rgb = render.render_over_time(m, cam, 12, 5, times[:1])
    assert rgb[0][1].shape == (12, 12, 3) and torch.equal(rgb[0][1], one[0][1][..., :3])


def test_forward_is_untouched_by_forward_maps(ops):
    g = load_golden("g25_dyn_voxel_s16_n5_ragged")
    m = build_model(g)
    rays, t = g["rays"].cuda(), g["times"].cuda()
    with torch.no_grad():
        before = m((rays, t))
        kept = dict(alpha=m.canonical.alpha, weights=m.canonical.weights, dp=m.dp, rigidity=m.rigidity, pts=m.pts)
        bits = {k: v.clone() for k, v in kept.items()}
        maps = m.forward_maps((rays, t), acc=True)
        for k, v in kept.items():
            now = getattr(m.canonical, k) if k in ("alpha", "weights") else getattr(m, k)
            assert now is v and torch.equal(v, bits[k]), k
        after = m((rays, t))
    assert torch.equal(before, after) and torch.equal(maps["rgb"], before)
    for k in ("alpha", "weights"):
        assert torch.equal(getattr(m.canonical, k), bits[k]), k
    assert torch.equal(m.dp, bits["dp"]) and torch.equal(m.rigidity, bits["rigidity"])
    from nerf_atlas_amd import render
    assert torch.equal(maps["depth"], render.depth_map(m)) and torch.equal(maps["flow"], render.flow_map(m))
    assert torch.equal(maps["rigidity"], render.rigidity_map(m)) and torch.equal(maps["acc"], render.alpha_map(m))


def test_forward_maps_random_background_and_refusals(ops):
    g = load_golden("g25_dyn_voxel_s4_n4")
    m = build_model(g)
    rays, t = g["rays"].cuda(), g["times"].cuda()
    m.set_bg("black")
    with torch.no_grad():
        black = m.forward_maps((rays, t), acc=True)
        m.set_bg("random")
        rand = m.forward_maps((rays, t), acc=True)
    c = m.canonical
    assert c.weights is None and set(rand) == set(black)                       # no forward yet: still nothing per sample
    want = black["rgb"] + c.bg_rand * (1 - black["acc"])
    assert float((rand["rgb"] - want).abs().max()) <= 1e-6 and float(c.bg_rand.min()) >= 0
    for k in ("depth", "acc", "flow", "rigidity"):
        assert torch.equal(rand[k], black[k]), k
    with pytest.raises(RuntimeError, match="forward_maps"):
        m.forward_maps((rays, t))                                              # gradients are being recorded
    with torch.no_grad(), pytest.raises(RuntimeError, match="forward_maps"):
        m.train().forward_maps((rays, t))


# ------------------------------------------------------------------------------------------------------------ command line
def test_runner_cli_writes_the_panels_and_the_time_sweep(tmp_path):
    from PIL import Image
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2, dynamic=True) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--data-kind", "dnerf", "--size", "32", "--crop-size", "16", "--test-crop-size", "20", "--batch-size", "2",
                       "--steps", "24", "--epochs", "2", "--quiet", "--model", "voxel", "--dyn-model", "voxel", "--spline", "4", "--refl-kind", "pos",
                       "-lr", "1e-2", "--depth-images", "--flow-map", "--rigidity-map", "--render-over-time", "0", "--render-over-time-steps", "4",
                       "--with-alpha", "--outdir", str(out)])
    txt = (out / "results.txt").read_text().split("\n")
    assert txt[0].startswith("[Summary") and len(txt) == 6 + 2 and all(l.startswith(f"[{i:03}]: L2 ") and " PSNR " in l for i, l in enumerate(txt[6:]))
    assert len(res["maps"]) == 2 and len(res["frames"]) == 2
    for maps in res["maps"]:
        assert {k: tuple(v.shape) for k, v in maps.items()} == {"depth": (32, 32, 1), "flow": (32, 32, 3), "rigidity": (32, 32, 1)}
        assert all(bool(torch.isfinite(v).all()) for v in maps.values())
    for i in range(2):
        img = np.asarray(Image.open(out / f"test_{i:03}.png"))
        assert img.shape == (32, 5 * 32, 3)                                     # label | got | depth | flow | rigidity
    for i in range(4):
        img = np.asarray(Image.open(out / f"time_{i:03}.png"))
        assert img.shape == (32, 32, 4)
    assert not (out / "time_004.png").exists()
