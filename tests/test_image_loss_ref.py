"""The loss wrapper on the host: the fp64 restatement of tests/image_loss_ref.py and train.image_loss_torch against the
reference's recorded fp32 results (tests/golden/g30_image_loss.npz, tools/gen_golden.py g30), the definition's odd corners, the
auto-gamma rule, the command line, the errors raised by name, and that default flags leave load_loss_fn's result untouched."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import image_loss_ref as R
from conftest import GOLDEN, load_golden
from nerf_atlas_amd import train as T


@pytest.fixture(scope="module")
def g30():
    g = load_golden("g30_image_loss")
    assert g["combos"].tolist() == [R.combo_name(c) for c in R.COMBOS], "the fixture was recorded over another table: tools/gen_golden.py g30"
    return g


def test_the_generators_are_the_recorded_ones(g30):
    for name, (got, ref) in (("draw", R.kink_free_draw(1025, 30)), ("edge", R.edge_set())):
        assert np.array_equal(g30[f"{name}_got"].numpy(), got) and np.array_equal(g30[f"{name}_ref"].numpy(), ref)
    got, ref = R.kink_free_draw(1025, 30)
    gs, rs = np.sort(got.astype(np.float64), 1), np.sort(ref.astype(np.float64), 1)
    assert (gs[:, 2] - gs[:, 1]).min() > 1e-3 and (rs[:, 2] - rs[:, 1]).min() > 1e-3 and np.abs(got.astype(np.float64) - ref).min() > 1e-3
    assert np.abs(gs[:, 2] - rs[:, 2]).min() > 1e-3 and got.min() >= 1e-3 and got.max() <= 1.2 and ref.min() >= 0 and ref.max() <= 1


def test_restatement_against_the_reference(g30):
    """the fp64 restatement is the reference's function: its recorded fp32 results sit within the recorded deviation g_dev, and g_dev
    itself within the bound derived for an fp32 evaluation -- on every combination, both input sets, every element"""
    worst = 0.0
    for si, name in enumerate(("draw", "edge")):
        got, ref = g30[f"{name}_got"].numpy(), g30[f"{name}_ref"].numpy()
        for ci, c in enumerate(R.COMBOS):
            r = R.restate(got, ref, *c)
            dl = abs(float(g30[f"{name}_loss"][ci]) - r["loss"])
            dg = np.abs(g30[f"{name}_grad"][ci].numpy().astype(np.float64) - r["grad"])
            dev = g30["g_dev"][ci, si].numpy()
            assert dl <= dev[0] * (1 + 1e-9) + 1e-300 and dg.max() <= dev[1] * (1 + 1e-9) + 1e-300, (name, R.combo_name(c), dl, dg.max(), dev)
            assert dl <= r["loss_bound"] and (dg <= r["grad_bound"]).all(), (name, R.combo_name(c))
            ratio = max(dl / r["loss_bound"], float((dg[r["grad_bound"] > 0] / r["grad_bound"][r["grad_bound"] > 0]).max(initial=0.0)))
            worst = max(worst, ratio)
    print(f"[image loss ref] the reference's fp32 against the fp64 restatement: worst deviation / bound {worst:.3f}")


def test_image_loss_torch_against_the_reference(g30):
    """the plain-torch composition a CPU fit() trains with, in fp32, against the recorded values within bound + g_dev"""
    for si, name in enumerate(("draw", "edge")):
        got, ref = g30[f"{name}_got"], g30[f"{name}_ref"]
        for ci, c in enumerate(R.COMBOS):
            x = got.clone().requires_grad_(True)
            loss = T.image_loss_torch(x, ref, *c)
            g, = torch.autograd.grad(loss, x)
            r = R.restate(got.numpy(), ref.numpy(), *c)
            dev = g30["g_dev"][ci, si].numpy()
            assert abs(float(loss.detach()) - float(g30[f"{name}_loss"][ci])) <= r["loss_bound"] + dev[0], (name, R.combo_name(c))
            d = np.abs(g.numpy().astype(np.float64) - g30[f"{name}_grad"][ci].numpy())
            assert (d <= r["grad_bound"] + dev[1]).all(), (name, R.combo_name(c), d.max())


def test_hsv_is_zero_zero_max():
    """the reference's rgb2hsv takes its minimum from v.max: (0, 0, max) -- so an hsv l2 is the squared difference of the maxima over
    3 P elements, two thirds of them zero"""
    got, ref = R.kink_free_draw(65, 1)
    r = R.restate(got, ref, ("l2",), ("hsv",), False, 1.0)
    d = got.astype(np.float64).max(1) - ref.astype(np.float64).max(1)
    assert r["loss"] == pytest.approx((d * d).sum() / (3 * 65), rel=1e-14)
    loss = T.image_loss_torch(torch.from_numpy(got), torch.from_numpy(ref), ("l2",), ("hsv",))
    assert float(loss) == pytest.approx(r["loss"], rel=1e-5)
    k = got.argmax(1)
    assert (np.count_nonzero(r["grad"], axis=1) == 1).all() and (r["grad"][np.arange(65), k] != 0).all()


def test_a_tied_arg_max_takes_the_lowest_index():
    got = torch.tensor([[0.6, 0.6, 0.1], [0.2, 0.7, 0.7], [0.5, 0.5, 0.5]], requires_grad=True)
    ref = torch.tensor([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3]])
    g, = torch.autograd.grad(T.image_loss_torch(got, ref, ("l2",), ("hsv",)), got)
    assert (g != 0).tolist() == [[True, False, False], [False, True, False], [True, False, False]]
    r = R.restate(got.detach().numpy(), ref.numpy(), ("l2",), ("hsv",), False, 1.0)
    assert ((r["grad"] != 0) == (g != 0).numpy()).all()


def test_luminance_means_run_over_P():
    got, ref = R.kink_free_draw(7, 2)
    lum = lambda v: v.astype(np.float64) @ R.LUM
    assert R.restate(got, ref, ("l1",), ("luminance",), False, 1.0)["loss"] == pytest.approx(np.abs(lum(got) - lum(ref)).sum() / 7, rel=1e-14)


@pytest.mark.parametrize("mean, want", [
    (0.5 ** (1 / 0.40), 0.5),          # w = 0.40 < 0.55: aggressively 0.5
    (0.5 ** (1 / 0.54), 0.5),          # just below 0.55
    (0.5 ** (1 / 0.56), 0.56),         # just above: taken as it is
    (0.5 ** (1 / 0.89), 0.89),         # just below 0.9
    (0.5 ** (1 / 0.91), None),         # at or above 0.9: left alone
    (0.5 ** (1 / 3.0), None),
])
def test_auto_gamma_thresholds(mean, want, capsys):
    labels = torch.full((2, 4, 4, 3), mean, dtype=torch.float32)
    args = T.make_args(autogamma_correct_loss=True, gamma_correct_loss=1.25)
    T.auto_gamma(args, labels)
    note = capsys.readouterr().out
    if want is None:
        assert args.gamma_correct_loss == 1.25 and "ignoring" in note
    else:
        assert args.gamma_correct_loss == pytest.approx(want, rel=1e-5) and "autogamma correction weight is" in note
        assert want != 0.5 or args.gamma_correct_loss == 0.5


def test_auto_gamma_reads_the_image_tensor_of_a_labels_tuple(capsys):
    images, times = torch.full((3, 4, 4, 3), 0.5 ** (1 / 0.7)), torch.linspace(0, 1, 3)
    args = T.make_args(autogamma_correct_loss=True)
    T.auto_gamma(args, (images, times))
    assert args.gamma_correct_loss == pytest.approx(0.7, rel=1e-5) and "autogamma" in capsys.readouterr().out
    off = T.make_args()
    T.auto_gamma(off, (images, times))
    assert off.gamma_correct_loss == 1.0 and capsys.readouterr().out == ""
    bright = T.make_args(autogamma_correct_loss=True)   # a mean above 1: log > 0, w < 0 clamps to 0, then to 0.5
    T.auto_gamma(bright, torch.full((1, 2, 2, 3), 1.5))
    assert bright.gamma_correct_loss == 0.5


def test_command_line():
    a = T.args_from_argv(["--loss-fns", "l2", "rmse", "--color-spaces", "rgb", "xyz", "hsv", "--tone-map", "--gamma-correct-loss", "0.5"])
    assert (a.loss_fns, a.color_spaces, a.tone_map, a.gamma_correct_loss, a.autogamma_correct_loss) == (["l2", "rmse"], ["rgb", "xyz", "hsv"], True,
                                                                                                       0.5, False)
    d = T.args_from_argv([])
    assert (d.color_spaces, d.tone_map, d.gamma_correct_loss, d.autogamma_correct_loss) == (["rgb"], False, 1.0, False)
    assert T.args_from_argv(["--autogamma-correct-loss"]).autogamma_correct_loss is True


@pytest.mark.parametrize("overrides, names", [
    (dict(color_spaces=["rgb", "lab"]), "lab"),
    (dict(color_spaces=[]), "--color-spaces"),
    (dict(gamma_correct_loss=0.0), "--gamma-correct-loss"),
    (dict(gamma_correct_loss=-0.5), "--gamma-correct-loss"),
    (dict(gamma_correct_loss=float("nan")), "--gamma-correct-loss"),
    (dict(gamma_correct_loss=float("inf")), "--gamma-correct-loss"),
    (dict(loss_fns=["ssim"], tone_map=True), "ssim"),
    (dict(loss_fns=["l2", "ssim"], color_spaces=["hsv"]), "ssim"),
    (dict(loss_fns=["ssim"], gamma_correct_loss=0.5), "ssim"),
])
def test_errors_are_raised_by_name(overrides, names):
    with pytest.raises(ValueError, match=names):
        T.load_loss_fn(T.make_args(**overrides))


def test_default_flags_return_what_they_returned():
    """with the four flags at their defaults load_loss_fn hands out the very objects of before: F.mse_loss itself, the table's
    entries, and for several functions their plain mean"""
    assert T.load_loss_fn(T.make_args()) is F.mse_loss
    assert T.load_loss_fn(T.make_args(loss_fns=["l1"])) is F.l1_loss
    assert T.load_loss_fn(T.make_args(loss_fns=["rmse"])) is T.loss_map["rmse"]
    assert T.load_loss_fn(T.make_args(loss_fns=["ssim"])) is T.ssim_loss
    x, y = torch.rand(5, 3), torch.rand(5, 3)
    both = T.load_loss_fn(T.make_args(loss_fns=["l2", "rmse"]))
    assert torch.equal(both(x, y), (F.mse_loss(x, y) + T.loss_map["rmse"](x, y)) / 2)


def test_a_cpu_loss_with_flags_is_the_torch_composition():
    fn = T.load_loss_fn(T.make_args(loss_fns=["l2", "rmse"], color_spaces=["rgb", "xyz", "hsv"], tone_map=True, gamma_correct_loss=0.5))
    got, ref = (torch.from_numpy(v).reshape(5, 41, 5, 3) for v in R.kink_free_draw(1025, 30))
    x = got.permute(0, 2, 1, 3).requires_grad_(True)   # [B,h,w,3], not contiguous
    loss = fn(x, ref.permute(0, 2, 1, 3))
    loss.backward()
    r = R.restate(got.reshape(-1, 3).numpy(), ref.reshape(-1, 3).numpy(), ("l2", "rmse"), ("rgb", "xyz", "hsv"), True, 0.5)
    assert abs(float(loss.detach()) - r["loss"]) <= r["loss_bound"] and math.isfinite(float(loss.detach())) and x.grad.shape == x.shape


LOSS_FLAGS = ("--loss-fns", "--color-spaces", "--tone-map", "--gamma-correct-loss")


def without_loss_flags(argv):
    out, skipping = [], False
    for x in argv:
        if x in LOSS_FLAGS:
            skipping = True
        elif skipping and not (x.startswith("--") or x == "-lr"):
            continue
        else:
            skipping = False
            out.append(x)
    return out


def test_the_fixture_pins_the_loss():
    """the two recorded argv differ in the four loss flags only, and the reference's two curves separate by ten times the bar within
    the comparison window: the fixture pins the loss, not only the stream position"""
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_voxel_image_loss.json")))
    base = json.load(open(os.path.join(GOLDEN, "train_parity_voxel.json")))
    assert without_loss_flags(fx["argv"]) == without_loss_flags(base["argv"]) and fx["seed"] == base["seed"]
    assert fx["losses_without_flags"] == base["losses"]
    assert np.abs(np.array(fx["losses"][:10]) - np.array(base["losses"][:10])).max() >= 10 * 2e-4


def test_both_fixtures_carry_their_provenance_line():
    lines = open(os.path.join(GOLDEN, "PROVENANCE_image_loss.txt")).read().splitlines()
    for name, tool in (("g30_image_loss.npz", "tools/gen_golden.py g30"), ("train_parity_voxel_image_loss.json",
                                                                           "tools/ref_train_fixture.py voxel_image_loss")):
        assert os.path.exists(os.path.join(GOLDEN, name)) and any(l.startswith(name + ": " + tool) for l in lines), name
