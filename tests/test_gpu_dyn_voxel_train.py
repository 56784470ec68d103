"""--dyn-model voxel trained against the recorded reference (tests/golden/train_parity_dyn_voxel.json: the reference's runner.main on the
analytic dynamic scene, tools/ref_train_fixture.py dyn_voxel) by the mechanism of tests/test_gpu_train.py: this build's loaders, kernels
and training loop with the reference's random stream, procedural initial grids, deterministic accumulation."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.procedural import proc_param

pytestmark = pytest.mark.gpu


def procedural_init(model):
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(proc_param(k, tuple(v.shape))))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the recipe trained twice in deterministic mode (the second run is the reproducibility check's other side)"""
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_dyn_voxel.json")))
    data = make_scene(str(tmp_path_factory.mktemp("dv") / "scene"), **fx["scene"]) + "/"
    out = []
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        for _ in range(2):
            args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")])
            assert args.epochs == len(fx["losses"]) == 200 and args.dyn_model == "voxel" and args.voxel_tv_bezier > 0 and args.offset_decay > 0
            out.append(T.fit(args, replay_reference_rng=True, init=procedural_init))
    finally:
        config.set_deterministic(False)
    return fx, out


def test_training_tracks_the_reference(runs):
    """The first 5 losses within 2e-4 (the project's same-trajectory bar); the recipe learns, asserted on the reference's own curve.

    END POINT.  The reference recorded twice, under 8 and 2 threads (`other_runs` in the fixture): its own two runs differ by 3.7e-4 in
    the worst loss and by 0.0009 / 0.0356 / 0.0315 dB in the three test views -- measurable (the trajectory amplifies summation order
    over 200 Adam steps), but under the project's 0.1 dB.  The chaotic recipes' rule, 3 x the reference's own range, gives 0.107 dB
    here; the bar is the project's 0.1 dB per view against the committed (8-thread) run, which satisfies both readings.  The two
    deformation-grid TV terms of every iteration are compared as well: they pin the draw order (after the sigma / rgb terms' place)."""
    fx, (res, _) = runs
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    own = fx["other_runs"][0]
    tv_got, tv_ref = np.array(res["tv_terms"])[:, 2:], np.array(fx["tv_terms"])
    print(f"[dyn voxel parity] |loss - ref| first 5 {np.abs(got[:5] - ref[:5]).max():.2e}, all 200 {np.abs(got - ref).max():.2e} (the reference's "
          f"own {own['threads']}-thread run: {own['loss_linf']:.2e}); test PSNR {np.round(res['test_psnr'], 4).tolist()} vs "
          f"{np.round(fx['test_psnr'], 4).tolist()}: {d.max():.4f} dB (the reference's own runs: {own['psnr_linf']:.4f} dB); TV terms first 5 "
          f"{np.abs(tv_got[:5] - tv_ref[:5]).max():.2e}")
    assert ref[-20:].mean() < 0.5 * ref[:20].mean(), "the recipe must actually learn"
    assert np.abs(got[:5] - ref[:5]).max() <= 2e-4
    assert tv_got.shape == tv_ref.shape and np.abs(tv_got[:5] - tv_ref[:5]).max() <= 2e-4 and np.isnan(np.array(res["tv_terms"])[:, :2]).all()
    assert d.max() <= 0.1, d


def test_the_deterministic_run_is_bitwise_reproducible(runs):
    _, (a, b) = runs
    assert a["losses"] == b["losses"] and a["test_psnr"] == b["test_psnr"]
    for (k, x), (_, y) in zip(a["model"].state_dict().items(), b["model"].state_dict().items()):
        assert torch.equal(x, y), k


def test_runner_cli_trains_and_writes_results(tmp_path):
    """python -m nerf_atlas_amd.runner --data-kind dnerf --model voxel --dyn-model voxel --spline 4 --refl-kind pos"""
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2, dynamic=True) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--data-kind", "dnerf", "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2",
                       "--steps", "24", "--epochs", "12", "--quiet", "--model", "voxel", "--dyn-model", "voxel", "--spline", "4", "--refl-kind", "pos",
                       "-lr", "1e-2", "--voxel-tv-bezier", "0.01", "--outdir", str(out), "--save", str(tmp_path / "m.pt")])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12
    sd = torch.load(tmp_path / "m.pt")
    assert sorted(sd) == ["canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid"] and tuple(sd["ctrl_pts_grid"].shape) == (64, 64, 64, 9)
