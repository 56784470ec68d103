"""The references, bounds and edge inputs of tests/encoder_ref.py checked on the CPU: they agree with the oracle's own encoders, the
fp32 oracle stays inside every bound on every named set (no input asks for the unattainable), each seeded mistake leaves the bounds on
a named set, and the restated sincos_cw / mip angle path are measured against fp64."""
import math

import numpy as np
import pytest
import torch

import oracle as O
import encoder_ref as ER


@pytest.fixture(scope="module")
def hash_refs():
    tabs = ER.hash_tables()
    return {name: ER.hash_ref(x, tabs) for name, x in ER.hash_sets().items()}


# --------------------------------------------------------------------------------------------------------------- hash
def test_hash_sets_are_what_they_claim():
    s = ER.hash_sets()
    assert set(s) == set(ER.HASH_SETS) and s["bulk"].shape == (4096, 3)
    full = s["lattice"][:ER.N_LATTICE_FULL]
    assert torch.equal(full * 16, (full * 16).round())                          # on the level-0 lattice
    _, w = ER.hash_weights32(full, 0)
    assert bool((w == 0).all())
    for l in range(8):                                                          # the zeros sit on the lattice of every level
        assert bool((ER.hash_weights32(s["lattice"][-4:], l)[1] == 0).all())
    # the float just below a plane: floor selects the cell below and the weight rounds up to (or stays just under) one
    dn = s["below"][:ER.N_LATTICE_FULL]
    fl, w = ER.hash_weights32(dn, 0)
    assert torch.equal(fl, (full * 16) - 1) and bool((w > 0.999).all()) and bool((w <= 1).all())
    # a tiny negative coordinate: floor is -1 and v - floor(v) rounds to exactly 1.0 (trunc would give 0 and w = v)
    t = s["tiny_neg"]
    neg = t < 0
    tiny, tinier = t.abs() <= 1e-8, t.abs() <= 1e-29
    fl, w = ER.hash_weights32(t, 0)
    assert bool((fl[neg & tiny] == -1).all()) and bool((w[neg & tinier] == 1).all()) and bool((w[neg & tiny] > 0.999).all())
    assert int((neg & tiny).sum()) == 9 and int((neg & tinier).sum()) == 6
    assert float(s["far"].abs().max()) >= 2.0 ** 26 and ER.hash_concat().shape[0] >= max(ER.HASH_COUNTS)


@pytest.mark.parametrize("name", ER.HASH_SETS)
def test_hash_reference_agrees_with_the_oracle(hash_refs, name):
    """indices are the oracle's; the fp32 oracle's features and the fp32 autograd of them (position gradient, directional derivative)
    are inside the bounds"""
    x, tabs, ref = ER.hash_sets()[name], ER.hash_tables(), hash_refs[name]
    N = x.shape[0]
    xr = x.clone().requires_grad_(True)
    feats = O.hash_encode(xr, list(tabs), include_input=True)
    assert ER.bits_equal(feats[:, :3].detach(), x)
    rf = ER.worst_ratio(feats[:, 3:], ref["feat"], ER.hash_fwd_bound(ref))
    g = ER.hash_probe(N, 501, 35)
    (gx,) = torch.autograd.grad((feats * g).sum(), xr)
    want, bound = ER.hash_grad_ref(ref, g[:, 3:], g_in=g[:, :3])
    rg = ER.worst_ratio(gx, want, bound)
    # the directional derivative is the adjoint of the position gradient: <g, J e> = <J^T g, e>
    tan = ER.hash_probe(N, 502, 3)
    t, tb = ER.hash_jvp_ref(ref, tan)
    lhs, rhs = (t * g[:, 3:].double()).sum(1), ((want - g[:, :3].double()) * tan.double()).sum(1)
    assert float((lhs - rhs).abs().max()) <= 1e-9 * float(lhs.abs().max()) and bool((tb > 0).all())
    print(f"\n[hash {name}] oracle fp32 / bound: features {rf:.3f}, position gradient {rg:.3f}")
    assert rf <= 1.0 and rg <= 1.0, (name, rf, rg)


def test_hash_lattice_level0_is_the_table_row(hash_refs):
    x, tabs, ref = ER.hash_sets()["lattice"][:ER.N_LATTICE_FULL], ER.hash_tables(), hash_refs["lattice"]
    row = tabs[0][ref["idx"][0, 0, :ER.N_LATTICE_FULL]]
    assert torch.equal(ref["feat"][:ER.N_LATTICE_FULL, :4], row.double())
    assert ER.bits_equal(O.hash_encode(x, list(tabs), include_input=False)[:, :4], row)


@pytest.mark.parametrize("mistake,sets", [("trunc", ("tiny_neg", "bulk", "below")), ("swap", ("bulk",)), ("w64", ("far", "below"))])
def test_hash_seeded_mistakes_leave_the_bounds(hash_refs, mistake, sets):
    tabs = ER.hash_tables()
    for name in sets:
        ref = hash_refs[name]
        clean = ER.worst_ratio(ER.hash_fp32(ER.hash_sets()[name], tabs), ref["feat"], ER.hash_fwd_bound(ref))
        bad = ER.worst_ratio(ER.hash_fp32(ER.hash_sets()[name], tabs, mistake), ref["feat"], ER.hash_fwd_bound(ref))
        print(f"\n[hash {mistake} on {name}] error / bound {bad:.3g} (clean {clean:.3f})")
        assert clean <= 1.0 < bad, (mistake, name, clean, bad)


# ------------------------------------------------------------------------------------------------------------ Fourier
def test_sincos_cw_restated_measured_against_fp64():
    """the figure csrc/common.h quotes: worst error of sincos_cw for |m| <= 3e3 (the GPU bound is 1.25 x these)"""
    ws, wc = ER.cw_worst()
    print(f"\n[sincos_cw restated, |m| <= 3e3] worst |sin error| {ws:.3e}, worst |cos error| {wc:.3e}")
    assert 1.0e-7 < ws < 2.0e-7 and 4.0e-7 < wc < 7.0e-7      # the polynomials' own truncation: 1.45e-7 / 5.81e-7 were measured


@pytest.mark.parametrize("name", ["P", "L", "E"])
def test_fourier_model_and_oracle_are_inside_the_bounds(name):
    x, b = ER.fourier_sets()[name]
    for D in ER.D_VARIANTS:
        for scale in ER.SCALES:
            xs, bs = x[:, :D].contiguous(), b[:D].contiguous()
            ref, bound = ER.fourier_ref(xs, bs, scale)
            m = ER.fourier_m(xs, bs, scale).numpy().astype(np.float32)
            s, c = ER.fourier_sincos_emul(m)
            r = ER.worst_ratio(torch.from_numpy(np.concatenate([s, c], axis=-1)), ref, bound)
            ro = ER.worst_ratio(O.fourier_encode(xs, bs, scale), ref, bound.clamp(max=ER.LIBM))   # torch's sin / cos: inside both bounds
            assert r <= 1.0 / ER.CW_MARGIN + 1e-9 and ro <= 1.0, (name, D, scale, r, ro)
    assert float(ER.fourier_m(x, b, 1.0).abs().max()) == (98304.0 if name == "L" else 3072.0)


@pytest.mark.parametrize("mistake,name", [("two_term", "P"), ("two_term", "E"), ("short_cos", "P"), ("no_switch", "L")])
def test_fourier_seeded_mistakes_leave_the_bounds(mistake, name):
    x, b = ER.fourier_sets()[name]
    ref, bound = ER.fourier_ref(x, b, 1.0)
    m = ER.fourier_m(x, b, 1.0).numpy().astype(np.float32)
    s, c = ER.fourier_sincos_emul(m, **{mistake: True})
    err = (torch.from_numpy(np.concatenate([s, c], axis=-1)).double() - ref).abs()
    bad = float((err / bound).max())
    print(f"\n[sincos {mistake} on {name}] worst error {float(err.max()):.3e}, error / bound {bad:.3g}")
    assert bad > 1.0


def test_the_old_budget_does_not_see_the_two_term_reduction():
    """why the argument-exact sets exist: against 2e-4 the dropped third constant (4.8e-5 at |m| <= 1e3, 1.4e-4 at 3e3) passes"""
    m = np.concatenate([ER.fourier_m(*ER.fourier_sets()[n], 1.0).numpy().astype(np.float32).ravel() for n in ("P", "E")])
    m = m[np.abs(m) <= ER.CW_SWITCH]
    s, c = ER.sincos_cw_emul(m, two_term=True)
    worst = max(float(np.abs(s - np.sin(m.astype(np.float64))).max()), float(np.abs(c - np.cos(m.astype(np.float64))).max()))
    print(f"\n[two-term reduction] worst error {worst:.3e} for |m| <= 3e3")
    assert 2e-5 < worst < ER.BULK_TOL


def test_fourier_bulk_and_positional_references():
    for sigma in (16, 32):
        x, b, ref = ER.fourier_bulk(sigma)
        assert ER.worst_ratio(O.fourier_encode(x, b), ref, torch.full_like(ref, ER.BULK_TOL)) <= 1.0
    for NB in (4, 5):
        x, bands, ref = ER.positional_case(NB)
        assert ref.shape == (257, 2 * 3 * NB)
        assert ER.worst_ratio(O.positional_encode(x, bands), ref, torch.full_like(ref, ER.LIBM)) <= 1.0


# ------------------------------------------------------------------------------------------------- elevation / azimuth
def test_elaz_reference_and_oracle():
    d, zero = ER.elaz_dirs()
    ref, bound = ER.elaz_ref(d)
    s = ER.elaz_sets()
    assert s["bulk"].shape == (70, 3) and s["zero"].shape == (8, 3)
    # where no clamp acts the restatement IS the oracle evaluated in fp64
    free = (torch.nn.functional.normalize(d.double(), dim=-1).abs().max(dim=-1).values < ER.LIM32 - 1e-9) & (d.double().norm(dim=-1) > 1e-11)
    assert int(free.sum()) >= 80
    assert float((O.dir_to_elev_azim(d.double())[free] - ref[free]).abs().max()) <= 1e-15
    got = O.dir_to_elev_azim(d)
    r = (got.double() - ref).abs() / bound
    print(f"\n[elev / azim] oracle fp32 / bound: elevation {float(r[:, 0].max()):.3f}, azimuth {float(r[:, 1].max()):.3f}")
    assert float(r.max()) <= 1.0
    # the zero direction: elevation pi / 2, azimuth 0 or +-pi by the signs of zero
    z = got[zero]
    assert bool((z[:, 0] == np.float32(math.pi / 2)).all())
    assert sorted(set(z[:, 1].tolist())) == [float(np.float32(-math.pi)), 0.0, float(np.float32(math.pi))]
    assert ER.bits_equal(ref[zero].float(), z)
    assert float(bound[:, 0].max()) > 4 * ER.U * 700        # the clamp is reached


def test_a_clamp_that_drops_nan_is_caught():
    """fmin(fmax(v, -lim), lim) returns its other operand for a NaN: a NaN direction comes out finite"""
    d, _ = ER.elaz_dirs()
    d = d[-8:].clone()
    d[3, 1] = float("nan")
    ref, _ = ER.elaz_ref(d)
    bad, _ = ER.elaz_ref(d, keep_nan=False)
    assert bool(ref[3].isnan().all()) and bool(O.dir_to_elev_azim(d)[3].isnan().all())
    assert bool(torch.isfinite(bad[3]).all())                # the seeded mistake: elevation acos(-lim), azimuth -3 pi / 4
    assert abs(float(bad[3, 0]) - math.pi) < 2e-3 and abs(float(bad[3, 1]) + 0.75 * math.pi) < 1e-6
    keep = [i for i in range(8) if i != 3]
    assert torch.equal(ref[keep], bad[keep])


# ---------------------------------------------------------------------------------------------------------------- mip
def test_mip_angle_path_restated_measured_against_fp64():
    w, w_low = ER.mip_worst(), ER.mip_worst(False)
    print(f"\n[mip_feature angle path restated] worst error {w:.3e}; without the low half of 1 / 2 pi {w_low:.3e}")
    assert 1e-7 < w < 7e-7
    assert w_low > 1e-3                                       # the seeded mistake, before any damping


@pytest.mark.parametrize("kind", ["cylinder", "cone"])
@pytest.mark.parametrize("H", [4, 2])
def test_mip_reference_and_oracle(H, kind):
    worst, alive = 0.0, 0
    for T in ER.MIP_T:
        for form in ("explicit", "nan"):
            rays, ts, end = ER.mip_crop(H), ER.MIP_TS[:T], ER.mip_t_end(T, form)
            ref, bound = ER.mip_ref(rays, ts, kind, end)
            got = O.mip_latent_intended(rays[..., :3], rays[..., 3:], ts, kind, end=end)
            assert got.shape == ref.shape == (T, 1, H, 3, 96)
            worst = max(worst, ER.worst_ratio(got, ref, bound))
            alive = max(alive, int((ref[..., 84:90].abs() > 0.05).sum()))       # degree 14 is not damped away on the perpendicular axes
            if kind == "cylinder":
                # the seeded mistake on the crop's own means: the undamped features leave the bound
                mean = ER.mip_moments(rays, ts, kind, end, torch.float32)[0].numpy()
                cov = ER.mip_moments(rays, ts, kind, end, torch.float64)[1].numpy()
                k = 14
                damp = np.exp(-0.5 * cov * 4.0 ** k)
                bad = damp * ER.mip_sin_emul(mean, k, 0, low=False)
                ok = damp * ER.mip_sin_emul(mean, k, 0)
                sl = slice(3 * k, 3 * k + 3)
                assert ER.worst_ratio(torch.from_numpy(ok), ref[..., sl], bound[..., sl]) <= 1.0
                assert ER.worst_ratio(torch.from_numpy(bad), ref[..., sl], bound[..., sl]) > 1.0
    print(f"\n[mip {kind} H={H}] oracle fp32 / bound {worst:.3f}")
    assert worst <= 1.0 and alive > 0
