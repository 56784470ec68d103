"""tests/dyn_voxel_div_ref.py (the fp64 restatement the GPU tests hold csrc/dyn_voxel_div.hip to) against the recorded reference: the g29
fixtures are the reference's own fp64 autograd of DynamicNeRFVoxel.forward w.r.t. the sample positions, in training mode.  Every sample
and every gradient entry is compared -- the fixtures keep their samples 1e-3 voxel lengths off the cell faces -- inside the restatement's
own derived bounds (the kernel's bound plus the fp32 xyz chain's share, `b_xyz`)."""
import pytest
import torch

from conftest import load_golden
import dyn_voxel_div_ref as R
import voxel_ref as V

CASES = ("s2_n2", "s4_n4", "s4_n5", "s16_n11_ragged")


@pytest.fixture(scope="module", params=CASES)
def case(request):
    g = load_golden("g29_dyn_voxel_div_" + request.param)
    return request.param, g, R.fixture_case(g)


def test_fixture_keeps_its_promises(case):
    name, g, c = case
    S, n = int(g["S"]), c["spline"]
    assert (S, n) == {"s2_n2": (2, 2), "s4_n4": (4, 4), "s4_n5": (4, 5), "s16_n11_ragged": (16, 11)}[name]
    assert c["ctrl"].shape == (S, S, S, 3 * (n - 1)) and c["rig"].shape == (S, S, S, 1)
    assert float(R.face_distance(c["pts"], S, c["grid_radius"]).min()) >= 1e-3
    inside = float((c["pts"].abs() <= c["grid_radius"]).all(dim=-1).float().mean())
    assert 1 / 3 <= inside <= 2 / 3
    assert g["div_approx"].dtype == torch.float64 and g["g_ctrl"].dtype == torch.float64 and float(g["g_ctrl"].abs().max()) > 0
    if name == "s16_n11_ragged":
        assert c["pts"].shape[0] % 64 != 0


def test_ffjord_form_matches_the_reference(case):
    name, g, c = case
    r = R.jac_quad_ref(c["pts"], c["t"], c["ctrl"], c["rig"], c["spline"], c["grid_radius"], c["e"])
    ratio = V.worst_ratio(r["value"], g["div_approx"].reshape(-1), r["bound"] + r["b_xyz"])
    print(f"[{name}] e . J_rigid e: worst |err| / bound {ratio:.3f}, values up to {float(g['div_approx'].abs().max()):.3g}")
    assert ratio <= 1.0


def test_divergence_form_matches_the_reference(case):
    name, g, c = case
    r = R.jac_quad_ref(c["pts"], c["t"], c["ctrl"], None, c["spline"], c["grid_radius"], None)
    ratio = V.worst_ratio(r["value"], g["divergence"].reshape(-1), r["bound"] + r["b_xyz"])
    print(f"[{name}] 1 . J_dp 1: worst |err| / bound {ratio:.3f}, values up to {float(g['divergence'].abs().max()):.3g}")
    assert ratio <= 1.0


def test_gradient_matches_the_reference(case):
    name, g, c = case
    N, S = c["pts"].shape[0], int(g["S"])
    ref, mag, cnt, bx = R.jac_quad_backward_ref(c["pts"], c["t"], S, c["spline"], torch.full((N,), 1.0 / N, dtype=torch.float64),
                                                c["grid_radius"], None)
    want = g["g_ctrl"].reshape(ref.shape)
    # the restatement is fp64: only the fp32 xyz's share (and fp64's own rounding of a sum of cnt terms) stands between the two
    ratio = V.worst_ratio(ref, want, bx + 2.0 ** -50 * (cnt + 8) * mag)
    print(f"[{name}] d mean(divergence) / d ctrl_pts_grid: worst |err| / bound {ratio:.3f}, {int((want != 0).sum())} non-zero entries")
    assert ratio <= 1.0
    assert bool((want[cnt == 0] == 0).all())


def test_dp_form_with_unit_direction_is_the_sum_of_the_jacobian():
    """value(v = ones) equals the sum of the three value(v = e_i) plus the cross terms: the form is quadratic -- checked through its
    polarisation on one fixture, which pins that v enters both sides of v . (J v)"""
    g = load_golden("g29_dyn_voxel_div_s4_n4")
    c = R.fixture_case(g)
    args = (c["pts"], c["t"], c["ctrl"], None, c["spline"], c["grid_radius"])
    eye = torch.eye(3)
    J = torch.zeros(c["pts"].shape[0], 3, 3, dtype=torch.float64)
    for i in range(3):
        J[:, i, i] = R.jac_quad_ref(*args, eye[i].expand(c["pts"].shape))["value"]
    for i in range(3):
        for j in range(i + 1, 3):
            both = R.jac_quad_ref(*args, (eye[i] + eye[j]).expand(c["pts"].shape))["value"]
            J[:, i, j] = both - J[:, i, i] - J[:, j, j]   # J_ij + J_ji
    total = J.sum(dim=(1, 2))
    ones = R.jac_quad_ref(*args, None)["value"]
    assert float((total - ones).abs().max()) <= 1e-12 * float(ones.abs().max())
