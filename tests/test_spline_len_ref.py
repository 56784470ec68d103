"""tests/spline_len_ref.py against the recorded reference (g26: the real arc_len, runner.py:784-796) and against itself, on the CPU."""
import numpy as np
import pytest
import torch

from conftest import golden_params, load_golden
import voxel_ref as V
import spline_len_ref as R

CASES = ("s2_n2", "s4_n4", "s16_n5_ragged", "s16_n11")


def fixture(name):
    g = load_golden("g26_spline_len_" + name)
    S, n = int(g["S"]), int(g["spline"])
    return g, S, n, golden_params(g)["ctrl_pts_grid"]


def test_the_table_is_linspaces_own():
    """torch.linspace steps by fp32(1 / 15) = 0.06666667014... from either end, so j / 15 formed in fp32 is an ulp or more away at
    j = 3, 6 .. 10 (0.20000001788 against 0.20000000298): the table is carried, not formed"""
    assert R.T_TABLE.dtype == torch.float32 and float(R.T_TABLE[0]) == 0.0 and float(R.T_TABLE[-1]) == 1.0
    assert float(R.T_TABLE[1]) == float(np.float32(0.06666667014360428)) and float(R.T_TABLE[3]) == float(np.float32(0.20000001788139343))
    formed = np.arange(16, dtype=np.float32) / np.float32(15.0)
    assert [j for j in range(16) if float(R.T_TABLE[j]) != float(formed[j])] == [3, 6, 7, 8, 9, 10]


@pytest.mark.parametrize("name", CASES)
def test_grid_term_reproduces_the_reference(name):
    g, S, n, ctrl = fixture(name)
    rows = R.rows_of_flat(g["g_idxs"], ctrl.shape)
    r = R.grid_ref(ctrl.reshape(S ** 3, -1), rows)
    for suffix in ("", "64"):
        ratios = [V.worst_ratio(g["g_lens" + suffix], r["lens"], r["b_lens"]),
                  V.worst_ratio(g["g_value" + suffix], r["value"], r["b_value"]),
                  V.worst_ratio(g["g_grad" + suffix].reshape(S ** 3, -1), r["grad"], r["b_grad"])]
        print(f"[g26 {name} grid term, reference in fp{suffix or '32'}] worst |err| / bound: lens {ratios[0]:.3f} value {ratios[1]:.3f} grad {ratios[2]:.3f}")
        assert max(ratios) <= 1.0 and all(x == x for x in ratios), (name, suffix, ratios)
    if n == 2:  # one control point per voxel: a point, not a curve
        assert bool((r["lens"] == 0).all()) and float(r["value"]) == 0.0 and bool((r["grad"] == 0).all()) and bool((r["b_grad"] == 0).all())
        assert bool((g["g_lens"] == 0).all()) and bool((g["g_grad"] == 0).all())


@pytest.mark.parametrize("name", CASES)
def test_sample_term_reproduces_the_reference(name):
    """the reference's own fp32 run follows the same fp32 membership and xyz chain as the restatement and is held to the derived
    bounds; its `.double()` run forms xyz in fp64 (outside the bounds' premises: voxel_ref's module docstring -- the extrapolated
    first samples of every ray amplify the last bit of xyz) and its lengths are held to the project's 1e-4 bar"""
    g, S, n, ctrl = fixture(name)
    pts = R.fixture_points(g)
    r = R.dyn_ref(pts, ctrl, n, g["s_weights"].reshape(-1), grid_radius=float(g["grid_radius"]))
    ratios = [V.worst_ratio(g["s_lens"].reshape(-1), r["lens"], r["b_lens"]), V.worst_ratio(g["s_value"], r["value"], r["b_value"]),
              V.worst_ratio(g["s_grad"].reshape(S ** 3, -1), r["grad"], r["b_grad"])]
    print(f"[g26 {name} sample term] worst |err| / bound: lens {ratios[0]:.3f} value {ratios[1]:.3f} grad {ratios[2]:.3f}")
    assert max(ratios) <= 1.0 and all(x == x for x in ratios), (name, ratios)
    dev = float((g["s_lens64"].reshape(-1) - r["lens"]).abs().max())
    print(f"[g26 {name} sample term] the reference's fp64 lengths are up to {dev:.2e} away (fp64 xyz; its own fp32 run: "
          f"{float((g['s_lens'].double() - g['s_lens64']).abs().max()):.2e})")
    assert dev <= 1e-4


def test_equal_control_points_have_length_zero_and_gradient_exactly_zero():
    """control points that are equal powers of two (their products with t and 1 - t are exact): every point of the spline is that
    control point, bit for bit, every segment has length 0 and the rule dir = 0 at length 0 gives a gradient of exactly 0"""
    for m in (1, 3, 4, 10):
        grid = torch.tensor([0.5, -2.0, 1.0]).repeat(8, m)
        r = R.grid_ref(grid, torch.arange(8).repeat(3))
        assert bool((r["lens"] == 0).all()) and float(r["value"]) == 0.0
        assert bool((r["grad"] == 0).all()) and bool(torch.isfinite(r["grad"]).all())


@pytest.mark.parametrize("m", (2, 4, 10))
def test_the_closed_form_gradient_is_autograds(m):
    """sum_j dir_j (B_k(t_{j+1}) - B_k(t_j)) against fp64 autograd through de Casteljau's levels and the norm"""
    grid = R.flat_grid(16, m)
    rows = R.indices(37, 16)
    r = R.grid_ref(grid, rows, g_up=0.75)
    x = grid.double().requires_grad_(True)
    p = R.points(x[rows].reshape(37, m, 3))
    value = torch.linalg.vector_norm(p[:, 1:] - p[:, :-1], dim=-1).sum(-1).mean()
    (0.75 * value).backward()
    assert float((value.detach() - r["value"]).abs()) <= 1e-14
    assert float((x.grad - r["grad"]).abs().max()) <= 1e-13
