"""The routes of a voxel model's eval render agree bit for bit (every renderer forms a step's colour with csrc/voxel_plv.h's
vox_colour and a ray's own position with vox_ray_point): the one-launch renderer over a shared row, the per-ray-step renderer with every row equal to it,
the sparse renderer with a table of ones over both kinds of row, and the density-only proposal -- for every head, both backgrounds, a ray
count that leaves a workgroup part empty (5 rays, 4 to a workgroup at 16 lanes) and a row of 17 steps (a whole chunk of 16 and one more).
Then the table is emptied except for the cells of ONE ray: the others are exactly 0, that ray is untouched.  Inputs are seeded and
finite; NaN and edge cases are the per-route tests' (test_gpu_voxel*.py)."""
import pytest
import torch

import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

pytestmark = pytest.mark.gpu

GR = V.GRID_RADIUS
S, R, T = 4, 5, 17
KEPT = 3   # the ray whose cells stay live: with this seed no other ray has a sample in one of them (asserted below)
HEADS = (("rgb", -1), ("plv", 0), ("plv", 4), ("sh", 0), ("sh", 4))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def scene(ops):
    """rays from outside through the grid, ray 1 turned round (it never meets the grid: every sample is extrapolated); the shared row;
    the table that holds the lower cells of KEPT's samples only"""
    rays = V.generic_rays((R,), 9703).clone()
    rays[1, 3:] = -rays[1, 3:]
    rays, ts = rays.cuda(), torch.linspace(2.0, 6.0, T).cuda()
    pts = ops.compute_pts(rays, ts).reshape(T, R, 3).cpu()
    low = torch.stack([V.cells(pts[:, r].contiguous(), S)[0][:, 0] for r in range(R)])   # [R, T, 3]: corner 0 is the lower cell
    key = (low[..., 0] * S + low[..., 1]) * S + low[..., 2]
    assert not set(key[KEPT].tolist()) & set(key[[r for r in range(R) if r != KEPT]].flatten().tolist())
    one = torch.zeros(S ** 3, dtype=torch.uint8)
    one[key[KEPT]] = 1
    return rays, ts, one.reshape(S, S, S).cuda()


def same(a, b, what):
    for x, y, n in zip(a, b, ("out", "alpha", "weights")):
        assert torch.equal(x, y), (what, n)


@pytest.mark.parametrize("bg", ("black", "white"))
@pytest.mark.parametrize("head,order", HEADS, ids=[f"{h}{'' if k < 0 else k}" for h, k in HEADS])
def test_every_route_gives_the_same_bits(ops, scene, head, order, bg):
    rays, ts, one = scene
    den, rgb = (t.cuda() for t in (V.grid_values(S) if head == "rgb" else P.grid_values(S, order) if head == "plv" else H.grid_values(S, order)))
    rows = ts.expand(R, T).contiguous()
    o = () if head != "sh" else (order,)
    family = {"rgb": "voxel", "plv": "voxel_plv", "sh": "voxel_sh"}[head]
    dense = getattr(ops, family + "_render")(rays, ts, den, rgb, *o, GR, "upshifted", bg)
    assert all(bool(torch.isfinite(t).all()) for t in dense) and bool((dense[2] != 0).any())
    same(getattr(ops, family + "_render_rayts")(rays, rows, den, rgb, *o, GR, "upshifted", bg), dense, "per-ray steps")
    ones = torch.ones(S, S, S, dtype=torch.uint8, device="cuda")
    sparse = lambda row, live: ops.voxel_sparse_render(head, rays, row, den, rgb, live, GR, order, "upshifted", bg)
    same(sparse(ts, ones), dense, "sparse, shared row")
    same(sparse(rows, ones), dense, "sparse, per-ray rows")
    alpha, weights = ops.voxel_proposal(rays, ts, den, GR)
    assert torch.equal(alpha, dense[1]) and torch.equal(weights, dense[2])
    others = [r for r in range(R) if r != KEPT]
    for row in (ts, rows):
        out, a, w = sparse(row, one)
        assert bool((a[:, others] == 0).all()) and bool((w[:, others] == 0).all())
        assert torch.equal(out[KEPT], dense[0][KEPT]) and torch.equal(a[:, KEPT], dense[1][:, KEPT]) and torch.equal(w[:, KEPT], dense[2][:, KEPT])
