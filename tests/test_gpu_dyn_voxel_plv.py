"""The voxel D-NeRF over the pos-linear-view voxel head on the GPU: the dynamic model against the recorded reference (g28) forward and in
all four grid gradients -- the deformation grids' arrive through na_voxel_plv_sample_backward_pts --, and the one-launch test renderer
(na_dyn_voxel_plv_render) bit for bit against the launches it replaces, through the kernel entry, forward_maps, render_frame_maps and
render_over_time."""
import itertools

import pytest
import torch

from conftest import golden_params, load_golden
import voxel_plv_ref as P
import voxel_ref as V
import dyn_voxel_ref as D
import dyn_voxel_maps_ref as M

pytestmark = pytest.mark.gpu

GR = V.GRID_RADIUS
OPTIONAL = ("depth", "acc", "flow", "rigidity", "alpha", "weights")
GRADS = ("canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def build_model(g, device="cuda"):
    from nerf_atlas_amd import nerf, refl
    c = nerf.NeRFVoxel(resolution=int(g["S"]), t_near=float(g["near"]), t_far=float(g["far"]), steps=int(g["steps"]), bg=str(g["bg"]))
    c.set_refl(refl.PosLinearView(act=str(g["act"]), latent_size=0, out_features=3, voxel_order=4))
    m = nerf.DynamicNeRFVoxel(c, spline=int(g["spline"]))
    m.load_state_dict(golden_params(g), strict=True)
    return m.to(device).eval()


# ------------------------------------------------------------------------------------------------------------ the model vs the reference
@pytest.mark.parametrize("name", ("s4_n4", "s16_n2"))
def test_dynamic_model_matches_the_reference(ops, name):
    """g28: out, alpha, weights, dp, rigidity on the eval and the operator route within the project's 1e-4; the fp64 gradients of the four
    grids within 1e-4 of their largest entry (the bars of tests/test_gpu_dyn_voxel.py for g25)"""
    g = load_golden(f"g28_dyn_voxel_plv_{name}")
    m = build_model(g)
    rays, t = g["rays"].cuda(), g["times"].cuda()

    def check(out, what):
        got = dict(out=out, alpha=m.canonical.alpha, weights=m.canonical.weights, dp=m.dp, rigidity=m.rigidity)
        for k, x in got.items():
            err = float((x.detach().cpu().double() - g[k + "64"]).abs().max())
            print(f"[dyn voxel plv {name} {what}] {k} max |err| {err:.2e}")
            assert x.shape == g[k + "64"].shape and err <= 1e-4, (name, what, k, err)
    with torch.no_grad():
        check(m((rays, t)), "eval route")
    out = m((rays, t))
    assert out.requires_grad
    check(out, "operator route")
    out.square().sum().backward()
    params = dict(m.named_parameters())
    for i, k in enumerate(GRADS):
        want = g["grad64." + k]
        err = float((params[k].grad.cpu().double() - want).abs().max() / want.abs().max())
        print(f"[dyn voxel plv {name}] grad {k}: max |err| / largest entry {err:.2e} (the reference's own fp32: {float(g['g_dev'][i]):.2e})")
        assert params[k].grad.shape == want.shape and err <= 1e-4, (name, k, err)


@pytest.mark.parametrize("name", ("s4_n4", "s16_n2"))
def test_forward_maps_matches_the_recorded_reference(ops, name):
    g = load_golden(f"g28_dyn_voxel_plv_{name}")
    m = build_model(g)
    with torch.no_grad():
        got = m.forward_maps((g["rays"].cuda(), g["times"].cuda()), acc=True)
    want = dict(M.reference_maps(g["weights64"], g["ts"], g["dp64"], g["rigidity64"]), rgb=g["out64"])
    assert set(got) == set(want)
    for k, x in got.items():
        err = float((x.cpu().double() - want[k]).abs().max())
        print(f"[forward_maps plv {name}] {k} max |err| {err:.2e}")
        assert x.shape == want[k].shape and err <= 1e-4, (name, k, err)


# ------------------------------------------------------------------------------------------------------------ one launch, bit for bit
def rays_of(R, seed=4500):
    rays = V.generic_rays((R,), seed + R).clone()
    rays[2::3, 3:] = -rays[2::3, 3:]
    return rays


def times_of(R):
    t = D.times(R, "interior").clone()
    t[0::3] = 0.0
    t[1::3] = 1.0
    return t


def composition(ops, rays, t, ts, grids, n, act, bg):
    den, rgb, ctrl, rig = grids
    T, R = ts.shape[0], rays.shape[0]
    pts = ops.compute_pts(rays, ts)
    warped, dp, r = ops.dyn_voxel_warp(pts, t[None, :].expand(T, R).contiguous(), ctrl, rig, n, GR)
    out, alpha, weights = ops.voxel_plv_render(rays, ts, den, rgb, GR, act, bg, True, pts=warped)
    ones = torch.ones(T, R, 1, device="cuda")
    ones[-1] = 0
    return dict(rgb=out, alpha=alpha, weights=weights, depth=ops.integrate(weights, ts[:, None, None].expand(T, R, 1).contiguous()),
                acc=ops.integrate(weights, ones), flow=ops.integrate(weights, (dp * r[..., None]).contiguous()),
                rigidity=ops.integrate(weights, r[..., None].contiguous()))


@pytest.mark.parametrize("T", (1, 17, 80))
def test_bit_for_bit_against_the_launches_it_replaces(ops, T):
    """T = 1, 17 (one step past a chunk of 16) and the recipe's 80; 1, 35 and 257 rays; order 4 at S = 16 and 64 with the recipe's spline 4,
    the unaligned order 1 with spline 2; rays at t = 0, t = 1 and interior times, every third ray walking away from the grid"""
    ts = torch.linspace(2.0, 6.0, T).cuda() if T > 1 else torch.tensor([2.0]).cuda()
    for (R, (S, order, n)), act, bg in zip(itertools.product((1, 35, 257), ((16, 4, 4), (4, 1, 2), (64, 4, 4))),
                                           itertools.cycle(("upshifted", "thin")), itertools.cycle(("black", "white", "white"))):
        if S == 64 and R != 257:
            continue
        den, rgb = P.grid_values(S, order)
        grids = (den.cuda(), rgb.cuda()) + tuple(x.cuda() for x in D.dyn_grids(S, n))
        rays, t = rays_of(R).cuda(), times_of(R).cuda()
        got = ops.dyn_voxel_render(rays, t, ts, *grids, n, GR, act, bg, want=OPTIONAL, plv=True)
        ref = composition(ops, rays, t, ts, grids, n, act, bg)
        assert set(got) == set(ref)
        for k in ref:
            assert not bool(torch.isnan(ref[k]).any()), k
            assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (T, R, S, order, k, float((got[k] - ref[k]).abs().max()))
        # the bits of an output do not depend on which others are asked for
        few = ops.dyn_voxel_render(rays, t, ts, *grids, n, GR, act, bg, want=("flow",), plv=True)
        assert set(few) == {"rgb", "flow"} and torch.equal(few["rgb"], got["rgb"]) and torch.equal(few["flow"], got["flow"])


def camera():
    from nerf_atlas_amd import cameras
    c2w = torch.tensor([[[1.0, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 4.0]]])
    return cameras.NeRFCamera(cam_to_world=c2w, focal=14.0).cuda()


class Spy:
    NAMES = ("dyn_voxel_render", "dyn_voxel_warp", "voxel_plv_render", "voxel_render", "integrate")

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


def test_render_frame_maps_equals_the_generic_route_for_every_subset_of_maps(ops, monkeypatch):
    """a 12 x 12 frame in 5-pixel tiles (ragged last tiles): one launch per tile against render() + the map functions, bit for bit, for
    every subset of the four maps"""
    from nerf_atlas_amd import render
    m, cam = build_model(load_golden("g28_dyn_voxel_plv_s16_n2")), camera()
    t = torch.tensor([0.35], device="cuda")
    spy = Spy(monkeypatch, ops)
    names = ("depth", "flow", "rigidity", "acc")
    gen = render.render_frame_maps(m, cam, 12, 5, t, names, generic=True)
    assert spy.used() == {"dyn_voxel_warp": 9, "voxel_plv_render": 9, "integrate": 36}
    for k in range(len(names) + 1):
        for want in itertools.combinations(names, k):
            one = render.render_frame_maps(m, cam, 12, 5, t, want)
            assert spy.used() == {"dyn_voxel_render": 9}
            assert set(one) == {"rgb"} | set(want)
            for key in one:
                assert one[key].shape == (12, 12, render.MAP_CHANNELS.get(key, 3)) and torch.equal(one[key], gen[key]), (want, key)
    assert float(gen["acc"].max()) > 0 and float(gen["flow"].abs().max()) > 0


def test_render_over_time_with_alpha_equals_the_generic_route(ops, monkeypatch):
    from nerf_atlas_amd import render
    m, cam = build_model(load_golden("g28_dyn_voxel_plv_s4_n4")), camera()
    times = torch.tensor([0.0, 0.5, 1.0])
    spy = Spy(monkeypatch, ops)
    one = render.render_over_time(m, cam, 12, 5, times, with_alpha=True)
    assert spy.used() == {"dyn_voxel_render": 27}
    gen = render.render_over_time(m, cam, 12, 5, times, with_alpha=True, generic=True)
    assert "dyn_voxel_render" not in spy.used()
    for (_, a), (_, b) in zip(one, gen):
        assert a.shape == (12, 12, 4) and torch.equal(a, b)


def test_forward_maps_still_refuses_a_canonical_model_without_a_one_launch_route(ops):
    """unchanged behaviour: an activation passed as a callable (no named kernel activation) has no one-launch route"""
    g = load_golden("g28_dyn_voxel_plv_s4_n4")
    m = build_model(g)
    m.canonical._head.act_kind = None
    with torch.no_grad(), pytest.raises(RuntimeError, match="one-launch route"):
        m.forward_maps((g["rays"].cuda(), g["times"].cuda()))


def test_argument_checks(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    den, rgb = P.grid_values(4, 4)
    grids = (den.cuda(), rgb.cuda()) + tuple(x.cuda() for x in D.dyn_grids(4, 4))
    rays, t, ts, out = rays_of(8).cuda(), times_of(8).cuda(), torch.linspace(2, 6, 5).cuda(), torch.zeros(8, 3).cuda()
    p = ops._ptr
    call = lambda **k: lib.na_dyn_voxel_plv_render(p(rays), k.get("t", p(t)), k.get("R", 8), p(ts), 5, p(grids[0]), k.get("rgb", p(grids[1])),
                                                   p(grids[2]), p(grids[3]), 4, k.get("order", 4), k.get("n", 4), 1.3, 4, 0, p(out), None, None,
                                                   None, None, None, None, ops._stream())
    assert call() == 0 and call(R=0) == 0
    assert call(order=5) == -1 and b"order 5" in lib.na_last_error()
    assert call(n=12) == -3
    assert call(t=None) == -2 and b"t_ray" in lib.na_last_error()
    off = torch.zeros(64 * 28 + 1).cuda()[1:]
    assert call(rgb=p(off)) == -1 and b"16-byte" in lib.na_last_error()
    torch.cuda.synchronize()
