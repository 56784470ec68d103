"""tests/deform_sdf_ref.py on the CPU: the restatements against the fixtures recorded from the reference (g9_bezier, g10_laplace,
g15_march), the divergence reference against the closed form, the clean-input assertions for every input set the GPU tests use, and
torch's NaN rules in the marching restatement."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deform_sdf_ref as D
from conftest import load_golden


def test_warp_restatement_reproduces_g9_bezier():
    """the curves of warp_fp64, fed the fixture's control points through the est layout, against the reference's fp32 results"""
    g = load_golden("g9_bezier")
    t = g["t"].reshape(-1)
    N = t.numel()
    for n in list(range(2, 7)) + ["cubic"]:
        n, want = (4, g["cubic"]) if n == "cubic" else (n, g[f"dc{n}"])
        co = g[f"coeffs{n}"]                                                  # [n, N, 3]
        est = torch.cat([torch.zeros(N, 1), co.permute(1, 0, 2).reshape(N, 3 * n)], dim=1)
        ref = D.warp_ref(est, torch.zeros(N, 3), t, n)
        assert D.worst_ratio(want, ref["dp"], ref["dp_b"]) <= 1.0, n
        assert torch.equal(ref["rig"], torch.full((N, 1), 0.5, dtype=torch.float64))
        assert torch.equal(ref["warped"], ref["dp"] * 0.5)
    # the latent columns ride through the same curve: column j of the latent is curve j of another est
    est, pts, tt = D.warp_inputs(5, 2, 9)
    ref = D.warp_ref(est, pts, tt, 5, 2)
    ctrl = est[:, 17:27].reshape(9, 5, 2)
    for j in range(2):
        e2 = torch.cat([torch.zeros(9, 1), torch.stack([ctrl[:, :, j]] * 3, dim=-1).reshape(9, 15)], dim=1)
        assert torch.allclose(D.warp_ref(e2, pts, tt, 5)["dp"][:, 0], ref["enc_raw"][:, j], rtol=1e-14, atol=0)
    assert torch.allclose(ref["enc"], ref["enc_raw"] * torch.sigmoid(est[:, 16:17].double()), rtol=1e-14, atol=0)


def test_laplace_restatement_reproduces_g10_laplace():
    g = load_golden("g10_laplace")
    for sc in (0.1, 0.02, 1.5):
        beta = float(np.float32(sc))
        dens, b = D.laplace_ref(-g["sdf"], beta)          # (the fixture is laplace_cdf(sdf, scale); the density takes -sdf)
        assert D.worst_ratio(g[f"cdf_{sc}"], dens * beta, b * beta + D.U * dens * beta) <= 1.0, sc


def test_marching_restatement_reproduces_g15_march():
    g = load_golden("g15_march")
    r_o, r_d = g["r_o"].reshape(-1, 3), g["r_d"].reshape(-1, 3)
    R = r_o.shape[0]
    near, far, jit = float(g["an_near"]), float(g["an_far"]), float(g["jitter"])
    dist, hits, rem = torch.full((R,), near), torch.zeros(R, dtype=torch.bool), torch.ones(R, dtype=torch.bool)
    for _ in range(24):
        dist, hits, rem = D.sphere_step(D.analytic_sdf(r_o + r_d * dist[:, None]), 1e-3, far, dist, hits, rem)
    assert torch.equal(hits, g["an_sm_hits"].reshape(-1))
    assert float((dist - g["an_sm_dist"].reshape(-1)).abs().max()) <= 1e-6
    iters = 40
    step = (far - near + jit * (2 / iters)) / iters
    cm = D.analytic_sdf(r_o + near)
    idxs = torch.zeros(R, dtype=torch.int32)
    last, first = torch.full((R,), -1, dtype=torch.int32), torch.full((R,), -1, dtype=torch.int32)
    for i in range(iters):
        cm, idxs, last, first = D.sign_change_step(D.analytic_sdf(r_o + (near + step * (i + 1)) * r_d), i, cm, idxs, last, first)
    low, high = last.long()[:, None] * step, first.long()[:, None] * step
    assert torch.equal(low, g["an_last"].reshape(-1, 1)) and torch.equal(high, g["an_first"].reshape(-1, 1))
    best = r_o + (near + idxs.long()[:, None] * step) * r_d
    assert float((best - g["an_best"].reshape(-1, 3)).abs().max()) <= 1e-6
    sdf_at = lambda z: D.analytic_sdf(r_o + z * r_d)[:, None]
    sl, sh = sdf_at(low), sdf_at(high)
    z, todo = D.bisection_init(low, high, sl, sh, 1e-6)
    for _ in range(32):
        if not bool(todo.any()):
            break
        low, high, sl, sh, z, todo = D.bisection_step(sdf_at(z), 1e-6, low, high, sl, sh, z, todo)
    assert float((r_o + z * r_d - g["an_bi_pts"].reshape(-1, 3)).abs().max()) <= 1e-6


@pytest.mark.parametrize("n", range(2, 9))
def test_divergence_reference_agrees_with_the_closed_form(n):
    for N, pitch, kind in ((257, D.est_min_width(n), "interior"), (64, 38, "interior"), (9, 38, "zero"), (9, 38, "one"), (33, 38, "outside")):
        est, tan, t, e = D.ffjord_inputs(n, N, max(pitch, D.est_min_width(n)), kind)
        div, b = D.ffjord_ref(est, tan, t, e, n)
        closed = D.ffjord_closed_form(est, tan, t, e, n)
        assert float((div - closed).abs().max()) <= 1e-13 * max(1.0, float(closed.abs().max())), (n, N, kind)
        assert bool((b > 0).all())


def test_warp_gradient_reference_matches_the_bernstein_form():
    """autograd through de Casteljau / the cubic against B_k(t) written out: the two formulas of the same curve"""
    for n, n_rl in ((2, 0), (4, 2), (7, 1), (8, 16)):
        est, _, t = D.warp_inputs(n, n_rl, 17)
        est = D.pad_cols(est, D.est_min_width(n, n_rl) + 3)
        g_dp = D.uniform((17, 3), 77 + n)
        ge, b = D.warp_backward_ref(est, t, n, n_rl, g_dp=g_dp)
        B = D.bernstein(t.double().reshape(-1, 1), n)
        want = (B.unsqueeze(-1) * g_dp.double().unsqueeze(1)).reshape(17, 3 * n)
        assert torch.allclose(ge[:, 1:1 + 3 * n], want, rtol=1e-12, atol=1e-15)
        assert int(ge[:, 1 + 3 * n:].count_nonzero()) == 0 and int(ge[:, 0].count_nonzero()) == 0
        assert int(b[:, D.est_min_width(n, n_rl):].count_nonzero()) == 0     # unused columns: bound 0, exact zeros
        if n_rl:
            assert int(b[:, 1 + 3 * n:].count_nonzero()) == 0                 # no g_enc: the latent columns are exact zeros too


def test_clean_input_assertions_hold_for_every_gpu_input_set():
    for R in D.MARCH_ROWS:
        D.sphere_states(R), D.sign_states(R), D.bisect_states(R)
    for n in D.ACT_ROWS:
        x = D.act_inputs(n)
        D.act_deriv_ref(x, "leaky_relu", 1)
    for N in D.NORMALIZE_ROWS:
        D.normalize3_ref(D.normalize3_rows(N))
    D.normalize3_ref(D.normalize3_nan_rows())
    for N in D.LIGHT_ROWS:
        for per_c in (False, True):
            x, c, _ = D.light_inputs(N, per_c)
            for per_i in (False, True):
                for decay in (True, False):
                    D.point_light_ref(x, c, D.light_inputs(N, per_i)[2], decay)
    D.point_light_ref(*D.light_nan_inputs(), True)
    for beta in D.LAPLACE_BETAS:                       # (no threshold of its own: the kernel's path per element is restated in laplace_ref)
        for N in D.LAPLACE_ROWS:
            D.laplace_ref(D.laplace_inputs(N, float(np.float32(beta))), float(np.float32(beta)))
    # and the assertions do fire
    with pytest.raises(AssertionError):
        D.clean_threshold(torch.tensor([1e-3 + 1e-8]), float(np.float32(1e-3)), 1e-3)
    with pytest.raises(AssertionError):
        D.normalize3_ref(torch.tensor([[1e-12, 0.0, 0.0]]))
    with pytest.raises(AssertionError):
        D.act_deriv_ref(torch.tensor([1e-6]), "leaky_relu", 1)
    D.clean_threshold(torch.tensor([1e-3, 2e-3, float("nan")]), float(np.float32(1e-3)), 1e-3)   # (the fp32 threshold itself, clear, NaN)


def test_marching_restatement_follows_torch_nan_rules():
    nan = float("nan")
    sd = torch.tensor([nan, 0.5, nan, -1.0, 0.25])
    cm = torch.tensor([0.5, nan, nan, 0.5, 0.25])
    z = lambda v: torch.full((5,), v, dtype=torch.int32)
    cm2, idxs, last, first = D.sign_change_step(sd, 6, cm, z(0), z(-1), z(-1))
    assert torch.isnan(cm2).tolist() == [True, True, True, False, False]          # torch.minimum keeps a NaN from either side
    assert cm2[3:].tolist() == [-1.0, 0.25]
    assert idxs.tolist() == [0, 0, 0, 7, 0] and first.tolist() == [-1, -1, -1, 7, -1] and last.tolist() == [-1, -1, -1, 6, -1]
    # F.normalize and the point light's direction: a NaN component makes the whole row NaN
    assert bool(torch.isnan(F.normalize(torch.tensor([[1.0, nan, 2.0]]), dim=-1)).all())
    assert bool(torch.isnan(D.normalize3_ref(torch.tensor([[1.0, nan, 2.0]]))[0]).all())
    (d, _), (dist, _), (spec, _) = D.point_light_ref(torch.tensor([[nan, 0.0, 0.0]]), torch.zeros(3), torch.ones(3), True)
    assert bool(torch.isnan(d).all()) and bool(torch.isnan(dist).all()) and bool(torch.isnan(spec).all())
    # a NaN SDF value decides nothing in the sphere march, but the distance takes it
    dist, hits, rem = D.sphere_step(torch.tensor([nan, nan]), 1e-3, 4.0, torch.tensor([1.0, 1.0]), torch.tensor([False, False]),
                                    torch.tensor([True, False]))
    assert torch.isnan(dist).tolist() == [True, False] and hits.tolist() == [False, False] and rem.tolist() == [True, False]
    # bisection: a NaN midpoint moves neither end, and a NaN bracket value ends the row
    lo, hi, sl, sh = (torch.tensor([v, v]) for v in (1.0, 2.0, 0.5, -0.5))
    zz, todo = D.bisection_init(lo, hi, sl, sh, 1e-6)
    out = D.bisection_step(torch.tensor([nan, 0.25]), 1e-6, lo, hi, sl, sh, zz, todo)
    assert out[0].tolist() == [1.0, 1.5] and out[1].tolist() == [2.0, 2.0] and out[5].tolist() == [True, True]
    assert D.bisection_init(lo, hi, torch.tensor([nan, 0.5]), sh, 1e-6)[1].tolist() == [False, True]


def test_exact_thresholds_of_the_marching_restatement():
    """the edges the GPU tests feed the kernels, decided here by hand"""
    eps, far = float(np.float32(D.EPS)), float(np.float32(D.FAR))
    s, d, h, r = D.sphere_states(13)
    dist, hits, rem = D.sphere_step(s, D.EPS, D.FAR, d, h, r)
    assert not bool(hits[0]) and bool(rem[0])                      # sdf == eps is not a hit
    assert bool(hits[1]) and not bool(rem[1])
    assert bool(hits[2]) and float(d[2]) == far                    # dist == far still counts for a hit
    assert not bool(hits[3]) and not bool(rem[3]) and float(dist[3]) == far + 0.5
    assert not bool(hits[4]) and not bool(rem[4]) and float(dist[4]) > far and float(dist[4]) - far < 1e-6   # one ulp above far stops
    assert torch.equal(dist[5:9], d[5:9]) and torch.equal(hits[5:9], h[5:9]) and not bool(rem[5:9].any())     # rem == 0: untouched
    assert float(dist[12]) == far and not bool(hits[12]) and bool(rem[12])                                    # dist + sdf == far: goes on
    assert bool(hits[11]) and not bool(rem[11])
    sd, cm, idxs, last, first = D.sign_states(11)
    cm2, idxs2, last2, first2 = D.sign_change_step(sd, 8, cm, idxs, last, first)
    assert int(idxs2[0]) == int(idxs[0])                            # a tie leaves idxs alone
    assert int(idxs2[1]) == 9
    assert first2[2:4].tolist() == [-1, -1]                          # +-0 does not set first_neg
    assert int(first2[4]) == 9 and int(last2[4]) == 8
    assert int(first2[5]) == 3 and int(last2[5]) == 2                # first_neg is written once
    lo, hi, sl, sh, sm = D.bisect_states(9)
    z, todo = D.bisection_init(lo, hi, sl, sh, D.BISECT_EPS)
    assert todo.tolist() == [False, True, False, True, False, False, False, False, False]
    out = D.bisection_step(sm, D.BISECT_EPS, lo, hi, sl, sh, z, todo)
    assert float(out[0][1]) == 1.0 and float(out[1][1]) == 2.0 and bool(out[5][1])    # sdf_mid == 0 moves neither end
    assert float(out[1][3]) == float(z[3]) and not bool(out[5][3])                      # high moved: the bracket is eps wide, done
    assert torch.equal(out[4], (out[0] + out[1]) / 2)                                   # done rows still get the midpoint
