"""tests/voxel_ref.py against the recorded reference (g23, tools/gen_golden.py) on the CPU: on the lattice point set its cell ids and xyz
are the reference's fp32 ones bit for bit; its samples, composited in fp64, reproduce the reference's fp64 out / alpha / weights and
(S <= 16) its fp64 grid gradients; the fp32 restatement of the lookup stays inside the bounds the kernels are held to."""
import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V

CASES = ("s64_black", "s64_white", "s16_ragged", "s4", "s2")
SMALL = ("s16_ragged", "s4", "s2")


@pytest.mark.parametrize("name", SMALL)
def test_membership_is_the_references_bit_for_bit(name):
    g = load_golden(f"g23_voxel_{name}")
    S = int(g["S"])
    assert torch.equal(g["lat_pts"], V.lattice_points(S, float(g["grid_radius"])))   # the fixture carries the set this file defines
    ids, xyz = V.cells(g["lat_pts"], S, float(g["grid_radius"]))
    assert torch.equal(ids, g["lat_ids"])
    assert torch.equal(xyz.view(torch.int32), g["lat_xyz"].view(torch.int32))


def test_lattice_set_is_what_it_claims():
    """it contains the membership planes (fp32 and fp64 floors disagree on some of them), extrapolated points, the corners and the origin"""
    for S in (2, 4, 16, 64):
        p = V.lattice_points(S)
        vl = V.GRID_RADIUS * 2 / S
        on_plane = ((p.double() / vl * 2).round() - p.double() / vl * 2).abs().max()
        assert float(on_plane) < 1e-5 and float(p.abs().max()) > V.GRID_RADIUS and bool((p[-1] == 0).all())
        ids, xyz = V.cells(p, S)
        assert int(ids.min()) == 0 and int(ids.max()) == S - 1
        assert float(xyz.min()) < 0 and float(xyz.max()) > 1                          # extrapolation happens
    z = V.zero_points()
    ids, _ = V.cells(z, 4)
    assert bool((ids[:, 0] == 1).all()) and bool((ids[:, 7] == 2).all())              # tiny coordinates of either sign: cells S/2 - 1 and S/2


@pytest.mark.parametrize("name", CASES)
def test_model_reference_reproduces_the_fixture(name):
    """the reference's fp64 run and this file's (fp32 membership, fp64 behind it) differ by the fp32 rounding of xyz only: far inside
    the 1e-4 bar the models are held to; the bound printed is the one the gather is held to"""
    g = load_golden(f"g23_voxel_{name}")
    out, alpha, weights = V.model_ref(g)
    for got, key in ((out, "out64"), (alpha, "alpha64"), (weights, "weights64")):
        err = float((got - g[key]).abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


@pytest.mark.parametrize("name", CASES)
def test_fp32_lookup_is_inside_the_gather_bound(name):
    """the lookup restated wholly in fp32 torch (what the kernel computes, in another summation order) stays inside SAMPLE_C u mag"""
    g = load_golden(f"g23_voxel_{name}")
    p = golden_params(g)
    S = int(g["S"])
    pts = V.pts_of(g["rays"], g["ts"]).reshape(-1, 3)
    ref, mag = V.sample_ref(pts, p["densities"], p["rgb"], float(g["grid_radius"]))
    ids, xyz = V.cells(pts, S, float(g["grid_radius"]))
    pick = lambda v, pos: v if pos else 1 - v
    w32 = torch.stack([pick(xyz[:, 0], V.bit_i(u, 0)) * pick(xyz[:, 1], V.bit_i(u, 1)) * pick(xyz[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    grid = torch.cat([p["densities"], p["rgb"]], dim=-1).reshape(S ** 3, 4)
    got = (w32[..., None] * grid[V.rows_of(ids, S)]).sum(dim=1)
    ratio = V.worst_ratio(got, ref, V.sample_bound(mag))
    print(name, "worst |err| / bound", ratio, "largest |weight|", float(w32.abs().max()))
    assert ratio <= 1.0


@pytest.mark.parametrize("name", SMALL)
def test_scatter_reference_reproduces_the_fixture_gradients(name):
    """d sum(out^2) / d grids: the fp64 compositing's autograd gives g_raw, scatter_ref scatters it -- against the reference's fp64
    gradients, within 1e-5 of the largest entry (the two differ by the fp32 rounding of xyz, as above)"""
    g = load_golden(f"g23_voxel_{name}")
    p = golden_params(g)
    S, rays, ts = int(g["S"]), g["rays"], g["ts"]
    pts = V.pts_of(rays, ts)
    raw, _ = V.sample_ref(pts.reshape(-1, 3), p["densities"], p["rgb"], float(g["grid_radius"]))
    raw = raw.reshape(pts.shape[:-1] + (4,)).requires_grad_(True)
    out, _, _ = V.composite_ref(raw, ts, rays, str(g["act"]), str(g["bg"]))
    out.square().sum().backward()
    ref, _, cnt = V.scatter_ref(pts.reshape(-1, 3), raw.grad.reshape(-1, 4), S, float(g["grid_radius"]))
    assert int(cnt[:, 0].sum()) == 8 * pts.numel() // 3
    for got, key in ((ref[:, 0], "g_densities64"), (ref[:, 1:], "g_rgb64")):
        want = g[key].reshape(got.shape)
        err = float((got - want).abs().max() / want.abs().max())
        print(name, key, err)
        assert err <= 1e-5, (name, key, err)


def test_exact_case_is_exact():
    """scatter case G: every addend is a multiple of 1/64 and every partial sum fits 24 bits, so fp32 summation in any order is exact"""
    p, gr, S, rad = V.scatter_case("G")
    _, xyz = V.cells(p, S, rad)
    assert torch.equal(xyz * 4, (xyz * 4).round()) and float(xyz.min()) >= 0 and float(xyz.max()) <= 1
    ref, mag, _ = V.scatter_reference("G")
    assert torch.equal(ref * 64, (ref * 64).round()) and float(mag.max()) < 2.0 ** 15
    assert torch.equal(ref.float().double(), ref)
