"""tests/dyn_voxel_maps_ref.py against the recorded reference (g25, tools/gen_golden.py) on the CPU.  The reference's maps are its own
volumetric_integrate of the fixture's arrays (runner.py:894-916): sum(weights[..., None] * other, 0) with other = ts, dp * rigidity,
rigidity, and weights[:-1].sum(0).  g25's rule holds: a case counts only where the reference agrees with itself -- its fp32 maps lie
within 1e-5 of its fp64 ones -- and all five cases do (the largest distance is 2.9e-6, depth of s64_n4), so none may be skipped."""
import pytest
import torch

from conftest import load_golden
import dyn_voxel_maps_ref as M
import voxel_ref as V

CASES = ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11", "s64_n4")
SELF_BAR = 1e-5


def fixture_maps(g, suffix):
    return M.reference_maps(g["weights" + suffix], g["ts"], g["dp" + suffix], g["rigidity" + suffix])


def self_distance(g):
    m32, m64 = fixture_maps(g, ""), fixture_maps(g, "64")
    return {k: float((m32[k].double() - m64[k]).abs().max()) for k in M.MAPS}


def test_every_fixture_counts():
    """the reference's fp32 maps against its fp64 ones: every case inside 1e-5, none skipped"""
    counted = []
    for name in CASES:
        dist = self_distance(load_golden(f"g25_dyn_voxel_{name}"))
        print(name, "the reference's fp32 maps vs its fp64 maps:", dist)
        if max(dist.values()) <= SELF_BAR:
            counted.append(name)
    assert tuple(counted) == CASES


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_references_maps(name):
    """fp32 membership + fp64 behind it against the reference's fp64 run: rgb, alpha, weights and the four maps within 1e-5 (they
    differ by the fp32 rounding of xyz and of the warped points only)"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    assert max(self_distance(g).values()) <= SELF_BAR
    got = M.fixture_ref(g)
    want = dict(fixture_maps(g, "64"), rgb=g["out64"], alpha=g["alpha64"], weights=g["weights64"])
    for key in M.OUTPUTS:
        err = float((got[key] - want[key]).abs().max())
        print(name, key, err)
        assert got[key].shape == want[key].shape and err <= 1e-5, (name, key, err)


@pytest.mark.parametrize("name", CASES)
def test_the_references_fp32_run_is_inside_the_bounds(name):
    """a bound the reference's own fp32 run breaks would be wrong: its fp32 out / alpha / weights and the fp32 maps formed from its fp32
    arrays against the restatement, under the bounds the kernel is held to.  (torch sums the T addends pairwise and its softplus / exp
    are libm's: both inside forward_bounds' any-order, 1-ulp terms.)"""
    g = load_golden(f"g25_dyn_voxel_{name}")
    ref = M.fixture_ref(g)
    got = dict(fixture_maps(g, ""), rgb=g["out"], alpha=g["alpha"], weights=g["weights"])
    ratios = {k: V.worst_ratio(got[k], ref[k], ref["b_" + k]) for k in M.OUTPUTS}
    print(name, "worst |err| / bound:", {k: round(v, 3) for k, v in ratios.items()})
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert all(float(ref["b_" + k].min()) >= 0 for k in M.OUTPUTS)


def test_bounds_follow_the_conditioning():
    """the bounds are per element and follow the conditioning of the lookup: a ray whose samples stay where the weights are of order 1
    (S = 2: voxel_len 1.3, every sample within a few cells of the grid) is bounded near 1e-5, while the rays of the S = 64 case walk
    through the extrapolated region, where the weights alternate in sign and reach 3e4 (voxel_ref's docstring) and the logit's bound
    with them -- there the bit-for-bit comparison with the composition, not this bound, is the sharp check"""
    small = M.fixture_ref(load_golden("g25_dyn_voxel_s2_n2"))
    worst = {k: float(small["b_" + k].max()) for k in M.OUTPUTS}
    print("S = 2, largest bound per output:", worst)
    assert max(worst.values()) <= 1e-4 and float(small["b_alpha"].max()) <= 1e-5


def test_a_non_finite_ray_is_nan_in_every_output_and_nowhere_else():
    import dyn_voxel_ref as D
    rays = V.generic_rays((5,), 4510).clone()
    t, ts = D.times(5, "interior"), torch.linspace(2, 6, 7)
    den, rgb = V.grid_values(4)
    ctrl, rig = D.dyn_grids(4, 4)
    clean = M.render_ref(rays, t, ts, den, rgb, ctrl, rig, 4)
    rays[2, 0] = float("inf")
    got = M.render_ref(rays, t, ts, den, rgb, ctrl, rig, 4)
    keep = torch.tensor([0, 1, 3, 4])
    for k in M.OUTPUTS:
        a, b = (got[k], clean[k]) if k not in M.PER_SAMPLE else (got[k].movedim(1, 0), clean[k].movedim(1, 0))
        assert bool(torch.isnan(a[2]).all()) and torch.equal(a[keep], b[keep]), k
