"""--ffjord-div-decay and --dyn-diverge-decay over --dyn-model voxel in training, against the recorded reference
(tests/golden/train_parity_dyn_voxel_make.json: `make dyn_voxel`'s argv as shipped, --ffjord-div-decay 0.3 included;
train_parity_dyn_voxel_div.json: the same recipe with --dyn-diverge-decay in its place; tools/ref_train_fixture.py) by the mechanism of
tests/test_gpu_voxel_plv_train.py: the reference's argv plus this build's --voxel-refl-order 4, its random stream, procedural initial
grids, deterministic accumulation.

THE TERMS' BAR.  The per-iteration terms are not of order 1 (mean(alpha div^2) is 11 .. 28 here, the divergence term 0.015 .. 0.5), so
the project's 2e-4 loss bar is taken relatively.  Before fixing it the reference itself was run in fp32 against an fp64 copy of its model
at the same positions and steps, with the same draw, at the first five iterations (`ffjord_terms64`, `reg_terms64` in the fixtures):
    FFJORD term       largest relative deviation 7.4e-7
    divergence term   largest relative deviation 1.6e-5  (at the iteration whose term is 0.015: a mean that cancels to a tenth of its terms)
Both are below a quarter of the bar (5e-5), so the bar stays 2e-4 relative for both (`term_bar` recomputes this from the fixtures' own
numbers; had a deviation exceeded the quarter, 4 x the deviation would have been the bar).  Measured on the MI355X against the
reference's fp32 terms: FFJORD 6.6e-6, divergence 5.3e-5."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.procedural import proc_param

pytestmark = pytest.mark.gpu

LOSS_BAR = 2e-4


def procedural_init(model):
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(proc_param(k, tuple(v.shape))))


def term_bar(fp32, fp64):
    """the relative bar of the module docstring from the reference's own fp32 and fp64 terms of the first five iterations"""
    a, b = np.array(fp32[:5]), np.array(fp64[:5])
    dev = float((np.abs(a - b) / np.abs(b)).max())
    return (LOSS_BAR if dev <= LOSS_BAR / 4 else 4 * dev), dev


def train_twice(name, tmp_path_factory):
    """the recipe trained twice in deterministic mode (the second run is the reproducibility check's other side)"""
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config, nerf, refl
    fx = json.load(open(os.path.join(GOLDEN, f"train_parity_{name}.json")))
    data = make_scene(str(tmp_path_factory.mktemp(name) / "scene"), **fx["scene"]) + "/"
    out = []
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        for _ in range(2):
            args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")] + ["--voxel-refl-order", "4"])
            assert args.epochs == len(fx["losses"]) <= 60 and args.dyn_model == "voxel" and args.refl_kind == "pos-linear-view"
            out.append(T.fit(args, replay_reference_rng=True, init=procedural_init))
            m = out[-1]["model"]
            assert type(m) is nerf.DynamicNeRFVoxel and type(m.refl) is refl.PosLinearView and tuple(m.canonical.rgb.shape) == (64, 64, 64, 28)
    finally:
        config.set_deterministic(False)
    return fx, out, args


@pytest.fixture(scope="module")
def make_runs(tmp_path_factory):
    return train_twice("dyn_voxel_make", tmp_path_factory)


@pytest.fixture(scope="module")
def div_runs(tmp_path_factory):
    return train_twice("dyn_voxel_div", tmp_path_factory)


def check_curve_and_views(what, fx, res):
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    own = fx["other_runs"][0]
    print(f"[{what}] |loss - ref| first 5 {np.abs(got[:5] - ref[:5]).max():.2e}, all {len(ref)} {np.abs(got - ref).max():.2e} (the reference's own "
          f"{own['threads']}-thread run: {own['loss_linf']:.2e}); test PSNR {np.round(res['test_psnr'], 4).tolist()} vs "
          f"{np.round(fx['test_psnr'], 4).tolist()}: {d.max():.4f} dB (the reference's own runs: {own['psnr_linf']:.4f} dB)")
    assert own["psnr_linf"] <= 0.1, "the reference's own runs left the 0.1 dB bar: the chaotic-recipe rule would apply"
    assert np.abs(got[:5] - ref[:5]).max() <= LOSS_BAR
    assert d.max() <= 0.1, d


def check_reproducible(a, b):
    assert a["losses"] == b["losses"] and a["test_psnr"] == b["test_psnr"]
    for (k, x), (_, y) in zip(a["model"].state_dict().items(), b["model"].state_dict().items()):
        assert torch.equal(x, y), k


def test_make_dyn_voxel_as_shipped_tracks_the_reference(make_runs):
    """the first 5 losses within 2e-4, every test view within 0.1 dB (the reference's own 8- and 2-thread runs differ by less than 1e-5 dB, so that
    bar applies); mean(alpha div_approx^2) of the first five iterations within a relative 2e-4 -- the draw `e` sits at
    the reference's position of the random stream, or the terms (and everything drawn after them) would be other numbers altogether"""
    fx, (res, _), args = make_runs
    assert args.ffjord_div_decay == 0.3 and args.voxel_random_spline_len_decay == 1e-5 and args.offset_decay == 30
    check_curve_and_views("make dyn_voxel", fx, res)
    bar, dev = term_bar(fx["ffjord_terms"], fx["ffjord_terms64"])
    got, ref = np.array(res["ffjord_terms"]), np.array(fx["ffjord_terms"])
    rel = np.abs(got[:5] - ref[:5]) / np.abs(ref[:5])
    print(f"[make dyn_voxel] mean(alpha div^2) first 5: {got[:5].tolist()} vs {ref[:5].tolist()}: relative {rel.max():.2e}; bar {bar:.2e} (the "
          f"reference's fp32 vs fp64: {dev:.2e})")
    assert got.shape == ref.shape == (60,) and bool(np.isfinite(got).all())
    assert bar == LOSS_BAR and rel.max() <= bar
    tv_got, tv_ref = np.array(res["tv_terms"]), np.array(fx["tv_terms"])
    assert tv_got.shape == tv_ref.shape and np.abs(tv_got[:5] - tv_ref[:5]).max() <= LOSS_BAR        # the draw order around the new draw


def test_make_dyn_voxel_is_bitwise_reproducible(make_runs):
    _, (a, b), _ = make_runs
    check_reproducible(a, b)
    assert a["ffjord_terms"] == b["ffjord_terms"]


def test_dyn_diverge_decay_tracks_the_reference(div_runs):
    """the first 5 losses within 2e-4, every test view within 0.1 dB, the divergence term of the first five iterations within a relative
    2e-4; and the trained curve is the one WITH the term: over the last 10 losses it is closer to the reference's with-flag curve than to
    its without-flag curve (the two differ by up to 2.3e-3 there)"""
    fx, (res, _), args = div_runs
    assert args.dyn_diverge_decay == fx["diverge_weight"] and not args.ffjord_div_decay
    check_curve_and_views("dyn-diverge-decay", fx, res)
    bar, dev = term_bar(fx["reg_terms"], fx["reg_terms64"])
    got, ref = np.array(res["reg_terms"]), np.array(fx["reg_terms"])
    rel = np.abs(got[:5] - ref[:5]) / np.abs(ref[:5])
    print(f"[dyn-diverge-decay] term first 5: {got[:5].tolist()} vs {ref[:5].tolist()}: relative {rel.max():.2e}; bar {bar:.2e} (the reference's "
          f"fp32 vs fp64: {dev:.2e})")
    assert got.shape == ref.shape == (60,) and bar == LOSS_BAR and rel.max() <= bar
    assert all(v != v for v in res["ffjord_terms"]) and len(res["ffjord_terms"]) == 60                 # NaN where the flag is off
    losses, with_flag, without = np.array(res["losses"][-10:]), np.array(fx["losses"][-10:]), np.array(fx["losses_without_flag"][-10:])
    d_with, d_without = np.abs(losses - with_flag).max(), np.abs(losses - without).max()
    print(f"[dyn-diverge-decay] last 10 losses: {d_with:.2e} from the reference's curve with the flag, {d_without:.2e} from the one without")
    assert np.abs(with_flag - without).max() > 10 * LOSS_BAR and d_with < d_without


def test_dyn_diverge_decay_is_bitwise_reproducible(div_runs):
    _, (a, b), _ = div_runs
    check_reproducible(a, b)
    assert a["reg_terms"] == b["reg_terms"]


def test_runner_cli_runs_make_dyn_voxel_verbatim(tmp_path):
    """`make dyn_voxel`'s command line, --ffjord-div-decay 0.3 included, plus --voxel-refl-order 4, shortened (size, epochs, crop, steps),
    on the analytic dynamic scene: it trains and writes test frames with depth, flow and rigidity panels"""
    from PIL import Image
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2, dynamic=True) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--data-kind", "dnerf", "--size", "32", "--epochs", "6", "--near", "2", "--far", "6", "--batch-size", "2",
                       "--crop-size", "16", "--model", "voxel", "--dyn-model", "voxel", "-lr", "1e-2", "--loss-fns", "l2", "--test-crop-size", "20",
                       "--depth-images", "--flow-map", "--spline", "4", "--steps", "24", "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4",
                       "--voxel-tv-bezier", "1e-4", "--voxel-tv-rigidity", "1e-4", "--higher-end-chance", "1", "--offset-decay", "30",
                       "--ffjord-div-decay", "0.3", "--sigmoid-kind", "upshifted", "--voxel-random-spline-len-decay", "1e-5", "--notraintest",
                       "--seed", "-1", "--refl-kind", "pos-linear-view", "--voxel-refl-order", "4", "--rigidity-map", "--quiet", "--outdir", str(out),
                       "--save", str(tmp_path / "m.pt")])
    assert len(res["losses"]) == 6 and all(l == l for l in res["losses"]) and len(res["maps"]) == 2
    assert len(res["ffjord_terms"]) == 6 and all(np.isfinite(v) and v >= 0 for v in res["ffjord_terms"])
    for i in range(2):
        assert np.asarray(Image.open(out / f"test_{i:03}.png")).shape == (32, 5 * 32, 3)   # label | got | depth | flow | rigidity
