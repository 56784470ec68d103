"""The voxel D-NeRF over the spherical-harmonic voxel head on the GPU: the one-launch test renderer (na_dyn_voxel_sh_render) bit for bit
against the launches it replaces, for every subset of maps, and the gradients of all four grids of DynamicNeRFVoxel -- the deformation
grids' arrive through na_voxel_sh_sample_backward_pts -- against an fp64 autograd restatement (tests/dyn_voxel_ref.py's warp, the lookup
and head of tests/voxel_sh_ref.py with the cells frozen at the fp32 warped points)."""
import itertools

import pytest
import torch

import dyn_voxel_ref as D
import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

pytestmark = pytest.mark.gpu

GR = V.GRID_RADIUS
OPTIONAL = ("depth", "acc", "flow", "rigidity", "alpha", "weights")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def rays_of(R, seed=4500):
    rays = V.generic_rays((R,), seed + R).clone()
    rays[2::3, 3:] = -rays[2::3, 3:]
    return rays


def times_of(R):
    t = D.times(R, "interior").clone()
    t[0::3] = 0.0
    t[1::3] = 1.0
    return t


def composition(ops, rays, t, ts, grids, order, n, act, bg):
    den, rgb, ctrl, rig = grids
    T, R = ts.shape[0], rays.shape[0]
    pts = ops.compute_pts(rays, ts)
    warped, dp, r = ops.dyn_voxel_warp(pts, t[None, :].expand(T, R).contiguous(), ctrl, rig, n, GR)
    out, alpha, weights = ops.voxel_sh_render(rays, ts, den, rgb, order, GR, act, bg, True, pts=warped)
    ones = torch.ones(T, R, 1, device="cuda")
    ones[-1] = 0
    return dict(rgb=out, alpha=alpha, weights=weights, depth=ops.integrate(weights, ts[:, None, None].expand(T, R, 1).contiguous()),
                acc=ops.integrate(weights, ones), flow=ops.integrate(weights, (dp * r[..., None]).contiguous()),
                rigidity=ops.integrate(weights, r[..., None].contiguous()))


@pytest.mark.parametrize("T", (1, 17, 80))
def test_bit_for_bit_against_the_launches_it_replaces(ops, T):
    """T = 1, 17 (one step past a chunk of 16) and 80; 1, 35 and 257 rays; spline 2 and 4; every order (the aligned ones, 1 and 3, among
    them); rays at t = 0, t = 1 and interior times, every third ray walking away from the grid; every subset of the optional outputs"""
    ts = torch.linspace(2.0, 6.0, T).cuda() if T > 1 else torch.tensor([2.0]).cuda()
    cases = zip(itertools.product((1, 35, 257), (2, 4)), itertools.cycle(H.ORDERS), itertools.cycle((16, 4)),
                itertools.cycle(("upshifted", "thin", "leaky_relu")), itertools.cycle(("black", "white", "white")))
    for (R, n), order, S, act, bg in cases:
        den, rgb = H.grid_values(S, order)
        grids = (den.cuda(), rgb.cuda()) + tuple(x.cuda() for x in D.dyn_grids(S, n))
        rays, t = rays_of(R).cuda(), times_of(R).cuda()
        got = ops.dyn_voxel_render(rays, t, ts, *grids, n, GR, act, bg, want=OPTIONAL, sh_order=order)
        ref = composition(ops, rays, t, ts, grids, order, n, act, bg)
        assert set(got) == set(ref)
        for k in ref:
            assert not bool(torch.isnan(ref[k]).any()), k
            assert got[k].shape == ref[k].shape and torch.equal(got[k], ref[k]), (T, R, S, order, n, k, float((got[k] - ref[k]).abs().max()))
        if R != 35:
            continue
        for size in range(len(OPTIONAL)):   # the bits of an output do not depend on which others are asked for
            for want in itertools.combinations(OPTIONAL, size):
                few = ops.dyn_voxel_render(rays, t, ts, *grids, n, GR, act, bg, want=want, sh_order=order)
                assert set(few) == {"rgb"} | set(want) and all(torch.equal(few[k], got[k]) for k in few), (T, n, want)


def fp64_model(rays, t, ts, den, rgb, ctrl, rig, order, n, act):
    """out [B,H,W,3] as an fp64 autograd function of the four grids; the cells of both lookups are the fp32 chain's"""
    S = den.shape[0]
    vl = GR * 2 / S
    T = ts.shape[0]
    pts = V.pts_of(rays, ts)
    tt = t.reshape((1, -1) + (1,) * (rays.dim() - 2)).expand(pts.shape[:-1])
    warped = D.warp_ref(pts.reshape(-1, 3), tt.reshape(-1), ctrl, rig, n)["warped"]
    w32 = warped.detach().float()
    ids, xyz = V.cells(w32, S)
    rows = V.rows_of(ids, S)
    x = xyz.double() + (warped - w32.double()) / vl       # (xyz as a function of the fp64 warped point inside the frozen cell)
    pick = lambda v, pos: v if pos else 1 - v
    w = torch.stack([pick(x[:, 0], V.bit_i(u, 0)) * pick(x[:, 1], V.bit_i(u, 1)) * pick(x[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    dirs = rays[..., 3:].reshape(-1, 3)
    Y = P.basis(dirs, order)[0][torch.arange(w.shape[0]) % dirs.shape[0]]
    density = (w * den.reshape(-1)[rows]).sum(-1, keepdim=True)
    s = (w[:, :, None, None] * Y[:, None, None, :] * rgb.reshape(S ** 3, 3, H.nk(order))[rows]).sum(dim=(1, 3))
    rows4 = H.head_ref(torch.cat([density, s], dim=-1), act).reshape((T,) + tuple(rays.shape[:-1]) + (4,))
    return P.composite_final(rows4, ts, rays, "black")[0]


@pytest.mark.parametrize("S,n,order", ((4, 4, 4), (16, 2, 3)))
def test_dynamic_model_gradients_of_all_four_grids(ops, S, n, order):
    """the bar of the pos-linear-view tests: every gradient within 1e-4 of the largest entry of the fp64 one"""
    from nerf_atlas_amd import nerf, refl
    c = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=9)
    c.set_refl(refl.SphericalHarmonic(act="upshifted", latent_size=0, out_features=3, voxel_order=order))
    m = nerf.DynamicNeRFVoxel(c, spline=n)
    den, rgb = H.grid_values(S, order)
    ctrl, rig = D.dyn_grids(S, n)
    m.load_state_dict({"canonical.densities": den, "canonical.rgb": rgb, "ctrl_pts_grid": ctrl * 0.2, "rigidity_grid": rig}, strict=True)
    m = m.cuda().eval()
    rays, t = V.generic_rays((2, 3, 3), 4760), D.times(2, "interior")
    out = m((rays.cuda(), t.cuda()))
    assert out.requires_grad
    out.square().sum().backward()
    g64 = [x.double().requires_grad_(True) for x in (den, rgb, ctrl * 0.2, rig)]
    ref = fp64_model(rays, t, m.canonical.ts.cpu(), *g64, order, n, "upshifted")
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"[dyn voxel sh S={S} n={n} K={order}] out max |err| {err:.2e}")
    assert err <= 1e-4
    ref.square().sum().backward()
    params = dict(m.named_parameters())
    for k, want in zip(("canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid"), g64):
        rel = float((params[k].grad.cpu().double() - want.grad).abs().max() / want.grad.abs().max())
        print(f"[dyn voxel sh S={S} n={n} K={order}] grad {k}: max |err| / largest entry {rel:.2e}")
        assert params[k].grad.shape == want.grad.shape and rel <= 1e-4, (k, rel)


def test_forward_maps_takes_the_one_launch_renderer(ops, monkeypatch):
    from nerf_atlas_amd import nerf, refl
    c = nerf.NeRFVoxel(resolution=4, t_near=2.0, t_far=6.0, steps=17)
    c.set_refl(refl.SphericalHarmonic(act="upshifted", latent_size=0, out_features=3, voxel_order=2))
    m = nerf.DynamicNeRFVoxel(c, spline=4).cuda().eval()
    calls = []
    monkeypatch.setattr(ops, "dyn_voxel_render", (lambda fn: lambda *a, **k: (calls.append(k.get("sh_order")), fn(*a, **k))[1])(ops.dyn_voxel_render))
    rays, t = V.generic_rays((2, 3, 3), 4761).cuda(), D.times(2, "interior").cuda()
    with torch.no_grad():
        maps = m.forward_maps((rays, t), acc=True)
        out = m((rays, t))
    assert calls == [2] and set(maps) == {"rgb", "depth", "acc", "flow", "rigidity"} and torch.equal(maps["rgb"], out)


def test_argument_checks(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    den, rgb = H.grid_values(4, 3)
    grids = (den.cuda(), rgb.cuda()) + tuple(x.cuda() for x in D.dyn_grids(4, 4))
    rays, t, ts, out = rays_of(8).cuda(), times_of(8).cuda(), torch.linspace(2, 6, 5).cuda(), torch.full((8, 3), 5.0).cuda()
    p = ops._ptr
    call = lambda **k: lib.na_dyn_voxel_sh_render(p(rays), k.get("t", p(t)), k.get("R", 8), p(ts), 5, p(grids[0]), k.get("rgb", p(grids[1])),
                                                  p(grids[2]), p(grids[3]), 4, k.get("C", 48), k.get("order", 3), k.get("n", 4), 1.3, 4, 0, p(out),
                                                  None, None, None, None, None, None, ops._stream())
    assert call(R=0) == 0
    assert call(order=5) == -1 and b"order 5" in lib.na_last_error()
    assert call(C=19) == -1 and call(C=75) == -1 and call(order=2) == -1   # C names another head, or another order
    assert call(n=12) == -3
    assert call(t=None) == -2 and b"t_ray" in lib.na_last_error()
    off = torch.zeros(64 * 48 + 1).cuda()[1:]
    assert call(rgb=p(off)) == -1 and b"16-byte" in lib.na_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call() == 0
    with pytest.raises(ValueError, match="two different heads"):
        ops.dyn_voxel_render(rays, t, ts, *grids, 4, GR, plv=True, sh_order=3)
    torch.cuda.synchronize()
