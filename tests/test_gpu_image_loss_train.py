"""The loss wrapper in training: tests/golden/train_parity_voxel_image_loss.json -- the reference's runner.main on the
analytic scene with the `voxel` recipe under --loss-fns l2 rmse --color-spaces rgb xyz hsv --tone-map --gamma-correct-loss 0.5
(tools/ref_train_fixture.py voxel_image_loss) -- replayed through this build's loaders, kernels and training loop with the reference's
random stream, and one run through the command line."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.procedural import proc_param

pytestmark = pytest.mark.gpu


def test_training_tracks_the_reference(tmp_path):
    """First 10 losses within 2e-4 (the bar tests/test_gpu_voxel.py holds train_parity_voxel.json to); the recipe learns on the
    reference's own curve -- to 0.62 x its start in 200 iterations, the rmse half of the loss falling like a square root; 0.75 x is
    asked of it --; every test view within the voxel recipe's 0.01 dB (DESIGN.md 3u records the measured deviation)."""
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_voxel_image_loss.json")))
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")])
    assert args.epochs == len(fx["losses"]) == 200 and args.model == "voxel"
    assert (args.loss_fns, args.color_spaces, args.tone_map, args.gamma_correct_loss) == (["l2", "rmse"], ["rgb", "xyz", "hsv"], True, 0.5)

    def procedural_init(model):
        with torch.no_grad():
            for k, v in model.state_dict().items():
                v.copy_(torch.from_numpy(proc_param(k, tuple(v.shape))))
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        res = T.fit(args, replay_reference_rng=True, init=procedural_init)
    finally:
        config.set_deterministic(False)
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    print(f"[voxel image-loss parity] |loss - ref| first 10 {np.abs(got[:10] - ref[:10]).max():.2e}, all 200 {np.abs(got - ref).max():.2e}; "
          f"test PSNR {np.round(res['test_psnr'], 4).tolist()} vs {np.round(fx['test_psnr'], 4).tolist()} ({d.max():.5f} dB)")
    assert ref[-20:].mean() < 0.75 * ref[:20].mean(), "the recipe must actually learn"
    assert np.abs(got[:10] - ref[:10]).max() <= 2e-4
    # measured on the MI355X: below 5e-6 dB in every view, far under half of the voxel recipe's 0.01 dB, so that bar is asserted
    assert d.max() <= 0.01, d


def test_runner_cli_trains_with_the_four_flags(tmp_path):
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2", "--steps", "24",
                       "--epochs", "12", "--quiet", "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2", "--outdir", str(out),
                       "--loss-fns", "l2", "rmse", "--color-spaces", "rgb", "xyz", "hsv", "--tone-map", "--gamma-correct-loss", "0.5"])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12 and all(np.isfinite(res["losses"]))
