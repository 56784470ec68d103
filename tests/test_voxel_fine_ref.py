"""tests/voxel_fine_ref.py against itself and against the modules it is built from (CPU): at a shared row the fine pass is the shared-step
model of every head, and the proposal is its alpha / weights; the gradient reference restates autograd entry by entry."""
import pytest
import torch

import voxel_fine_ref as F
import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

GR = V.GRID_RADIUS


def grids(head, order, S=4):
    return V.grid_values(S) if head == "rgb" else P.grid_values(S, order) if head == "plv" else H.grid_values(S, order)


def shared_model(head, order, rays, ts, den, rgb, act, bg):
    if head == "rgb":
        pts = V.pts_of(rays, ts)
        raw, _ = V.sample_ref(pts.reshape(-1, 3), den, rgb, GR)
        return V.composite_ref(raw.reshape(pts.shape[:-1] + (4,)), ts, rays, act, bg)
    if head == "plv":
        return P.render_ref(rays, ts, den, rgb, act, bg)
    return H.render_ref(rays, ts, den, rgb, order, act, bg)


@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 0), ("plv", 4), ("sh", 0), ("sh", 4)))
def test_fine_pass_at_a_shared_row_is_the_shared_step_model(head, order):
    R, T = 9, 7
    rays = V.generic_rays((R,), 7100)
    ts = torch.linspace(2.0, 6.0, T)
    den, rgb = grids(head, order)
    for act, bg in (("upshifted", "black"), ("thin", "white")):
        f = F.fine_ref(rays, ts.expand(R, T).contiguous(), den, rgb, head, order, act, bg)
        want = shared_model(head, order, rays, ts, den, rgb, act, bg)
        for got, ref in zip((f["comp"]["out"], f["comp"]["alpha"], f["comp"]["weights"]), want):
            assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-13
        prop, _ = F.proposal_ref(rays, ts, den)
        assert torch.equal(prop["alpha"], f["comp"]["alpha"]) and torch.equal(prop["weights"], f["comp"]["weights"])
        b = F.fine_bounds(f)
        assert all(bool((b[k] > 0).all()) and bool(torch.isfinite(b[k]).all()) for k in ("alpha", "weights", "out"))


def test_positions_are_formed_in_fp32_from_each_rays_own_row():
    rays = V.generic_rays((5,), 7110)
    ts_ray = torch.sort(2.0 + 4.0 * torch.rand(5, 6, generator=torch.Generator().manual_seed(1)), dim=1).values
    pts = F.pts_rayts(rays, ts_ray)
    assert pts.dtype == torch.float32 and pts.shape == (6, 5, 3)
    for r in range(5):
        assert torch.equal(pts[:, r], V.pts_of(rays[r:r + 1], ts_ray[r])[:, 0])


@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 1), ("sh", 1)))
def test_gradient_reference_restates_autograd_and_the_proposal_has_none(head, order):
    R, M = 6, 5
    rays = V.generic_rays((R,), 7120)
    ts_ray = torch.sort(2.0 + 4.0 * torch.rand(R, M, generator=torch.Generator().manual_seed(2)), dim=1).values
    ts_ray[:, 2] = ts_ray[:, 1]   # a duplicate step: the 1e-5 clamp
    den, rgb = grids(head, order)
    for det in (False, True):
        ref, bound = F.fine_grads(rays, ts_ray, den, rgb, head, order, "upshifted", "white", det)   # (asserts the restatement inside)
        assert ref.shape == (4 ** 3, 1 + F.channels(head, order)) and bool((bound >= 0).all()) and bool(torch.isfinite(bound).all())
        assert bool((bound[ref != 0] > 0).all())
