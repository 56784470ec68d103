"""CPU checks of tests/ssim_ref.py -- the restatement that pins SSIM / MS-SSIM (no fixture of the reference exists: pytorch_msssim is not
installed) -- and of the host side of --loss-fns ssim / --msssim-loss.  The discrimination condition lives here: on the inputs the GPU tests
use, every mutant moves the value by at least 10 x the bound the kernels are held to."""
import pytest
import torch

import ssim_ref as R

C1, C2 = 1e-4, 9e-4
DEFECT = 1.0 - float(R.window().sum()) ** 2     # the 121 products of the fp32 table sum to 1 - 2.8e-9


def zero_one_slack(value):
    """x = 0, y = 1 under the fp32 table: mu2 = 1 - DEFECT and s2 = mu2 (1 - mu2) <= DEFECT, so cs >= 1 - DEFECT / C2 and the luminance
    ratio moves by at most 2 DEFECT relative: how far the DEFINITION is from C1 / (1 + C1), to first order"""
    return value * (DEFECT / C2 + 2 * DEFECT)


def test_window_is_the_rounded_normalised_gaussian():
    g = R.window()
    assert g.numel() == 11 and bool((g == g.flip(0)).all()) and bool((g.float().double() == g).all())
    assert 0 < DEFECT < 22 * R.U
    assert abs(float(g[5]) - 0.26601171493530273) == 0


def test_identical_images_give_one():
    x, _ = R.image_pair(2, 26, 26, 3)
    s, cs = R.ssim_ref(x, x)
    assert float((s - 1).abs().max()) <= 1e-13 and float((cs - 1).abs().max()) <= 1e-13
    z = torch.zeros(1, 11, 13, 2)
    s, cs = R.ssim_ref(z, z)
    assert bool((s == 1).all()) and bool((cs == 1).all())


def test_zero_against_one():
    z, o = torch.zeros(1, 12, 15, 1), torch.ones(1, 12, 15, 1)
    s, _ = R.ssim_ref(z, o)
    want = C1 / (1 + C1)
    assert float((s - want).abs().max()) <= zero_one_slack(want) + 1e-18


def test_scale_sides_and_the_size_check():
    x = torch.zeros(1, 161, 161, 1)
    sides = []
    for _ in range(4):
        x = R.halve_ref(x)
        sides.append(x.shape[1])
    assert sides == [81, 41, 21, 11]
    assert tuple(R.halve_ref(torch.zeros(1, 176, 163, 2)).shape) == (1, 88, 82, 2)
    with pytest.raises(ValueError):
        R.ms_ssim_ref(torch.zeros(1, 160, 200, 1), torch.zeros(1, 160, 200, 1))
    assert tuple(R.ms_ssim_ref(*R.image_pair(1, 161, 161, 1)).shape) == (1, 1)


def test_halve_pads_odd_sides_and_divides_by_four():
    x = torch.arange(15, dtype=torch.float32).reshape(1, 3, 5, 1)
    h = R.halve_ref(x)[0, :, :, 0]
    assert tuple(h.shape) == (2, 3)
    assert float(h[0, 0]) == 0.0 and float(h[0, 1]) == (1 + 2) / 4 and float(h[1, 1]) == (6 + 7 + 11 + 12) / 4 and float(h[1, 0]) == (5 + 10) / 4


@pytest.mark.parametrize("case", R.SSIM_CASES[:4])
def test_closed_form_gradient_is_autograds(case):
    x, y = R.image_pair(*case)
    g = R.upstream(case[0], case[3])
    auto = R.ssim_grad_ref(x, y, g)
    closed, bound = R.ssim_grad_terms(x, y, g)
    assert float((auto - closed).abs().max()) <= 1e-12 * float(auto.abs().max())
    assert bool((bound >= 0).all()) and float(bound.max()) < 1e-3 * float(auto.abs().max())
    # the border of g_x is covered by fewer windows: the corner pixel by exactly one, and it is not zero
    assert float(auto[:, 0, 0].abs().min()) >= 0 and float(auto[:, -1, -1].abs().max()) > 0


@pytest.mark.parametrize("case", R.SSIM_CASES)
def test_ssim_mutants_leave_the_bound(case):
    x, y = R.image_pair(*case)
    s, cs, bs, bc = R.ssim_reference(case)
    assert float(bs.max()) < 2e-5 and float(bc.max()) < 2e-5, "a first-order bound of a value of order 1"
    for name in ("sigma 1.0", "9 taps", "C1 / C2 swapped"):
        ms, mc = R.ssim_ref(x, y, **R.MUTANTS[name])
        ratio = float(((ms - s).abs() / bs).min())
        print(f"{case} {name}: ssim moves by {float((ms - s).abs().min()):.2e} .. {float((ms - s).abs().max()):.2e}, bound {float(bs.max()):.2e}, "
              f"least ratio {ratio:.0f}")
        assert ratio >= 10, (case, name, ratio)


@pytest.mark.parametrize("case", R.MS_CASES + R.CPU_MS_CASES)
def test_ms_ssim_mutants_leave_the_bound(case):
    """The value is what the runner reports: the mean over (n, c).  A mutant must move it by 10 x the mean of the entries' bounds, and at
    least one entry by 10 x its own bound (a single channel may sit where a mutant's move changes sign: 9 taps at 161 x 161 moves the
    three channels by 121, 174 and 7 bounds)."""
    x, y = R.image_pair(*case)
    ref, bound = R.ms_reference(case)
    assert bool((ref > 0.05).all()) and bool((ref < 0.999).all())
    assert float(bound.max()) < 1e-5
    for name in ("sigma 1.0", "9 taps", "no padding", "C1 / C2 swapped"):
        if name == "no padding" and min(case[1:3]) < 176:
            with pytest.raises(RuntimeError):      # 161 -> 80 -> 40 -> 20 -> 10: the mutant's last scale is smaller than the window
                R.ms_ssim_ref(x, y, **R.MUTANTS[name])
            continue
        m = R.ms_ssim_ref(x, y, **R.MUTANTS[name])
        per_entry = (m - ref).abs() / bound
        of_mean = float((m.mean() - ref.mean()).abs() / bound.mean())
        print(f"{case} {name}: ms-ssim moves by {float((m.mean() - ref.mean()).abs()):.2e}, bound {float(bound.mean()):.2e}: {of_mean:.0f} bounds; "
              f"per entry {[round(float(v)) for v in per_entry.flatten()]}")
        assert of_mean >= 10 and float(per_entry.max()) >= 10, (case, name, of_mean)


def test_no_relu_mutant_shows_on_the_anticorrelated_pair():
    x, y = R.noise_pair(1, 161, 161, 3)
    vals = R.ms_ssim_values(x, y)
    assert bool((vals[0] < -0.5).all()), "every cs of the first scale is far below 0: the bound cannot carry it across"
    assert bool((R.combine_ref(vals) == 0).all())
    assert bool(torch.isnan(R.combine_ref(vals, relu=False)).all())


# ------------------------------------------------------------------------------------------------------------ host plumbing
def test_combination_runs_on_the_host_and_is_the_restatements():
    from nerf_atlas_amd import ops
    vals = R.ms_ssim_values(*R.image_pair(1, 161, 161, 3))
    got = ops.ms_ssim_combine(vals)
    assert got.dtype == torch.float64 and float((got - R.combine_ref(vals)).abs().max()) <= 1e-15
    neg = vals.clone()
    neg[2] = -neg[2]
    assert bool((ops.ms_ssim_combine(neg) == 0).all())
    got32 = ops.ms_ssim_combine(vals.float())
    assert got32.dtype == torch.float32 and float((got32.double() - got).abs().max()) <= 32 * R.U
    assert ops.MS_SSIM_WEIGHTS == R.WEIGHTS
    with pytest.raises(ValueError):
        ops.ms_ssim_combine(vals[:4])


def test_flags_parse():
    from nerf_atlas_amd import train as T
    assert T.DEFAULTS["msssim_loss"] is False and T.make_args().msssim_loss is False
    a = T.args_from_argv(["--msssim-loss", "--loss-fns", "l2", "ssim"])
    assert a.msssim_loss is True and a.loss_fns == ["l2", "ssim"]
    assert T.args_from_argv([]).msssim_loss is False
    assert T.load_loss_fn(T.make_args(loss_fns=["ssim"])) is T.loss_map["ssim"]
    assert callable(T.load_loss_fn(T.make_args(loss_fns=["l2", "ssim"])))


def test_ssim_loss_names_the_crop_size_and_the_flag():
    from nerf_atlas_amd import train as T
    loss = T.load_loss_fn(T.make_args(loss_fns=["ssim"]))
    with pytest.raises(ValueError, match="--crop-size"):
        loss(torch.zeros(2, 10, 16, 3), torch.zeros(2, 10, 16, 3))
    with pytest.raises(NotImplementedError, match="--loss-fns ssim"):
        loss(torch.zeros(2, 16, 16, 3), torch.zeros(2, 16, 16, 3))


def test_metric_refuses_small_frames_and_cpu_tensors():
    from nerf_atlas_amd import ops
    from nerf_atlas_amd import train as T
    z = torch.zeros(1, 160, 176, 3)
    with pytest.raises(ValueError, match="larger than 160"):
        ops.ms_ssim(z, z)
    big = torch.zeros(1, 161, 161, 3)
    with pytest.raises(NotImplementedError, match="ops.ms_ssim"):
        ops.ms_ssim(big, big)
    with pytest.raises(NotImplementedError, match="--msssim-loss"):
        T.test_similarity([big[0]], big)
    with pytest.raises(NotImplementedError, match="ops.image_halve"):
        ops.image_halve(big)
    with pytest.raises(NotImplementedError, match="ops.ssim"):
        ops.ssim(big, big)
