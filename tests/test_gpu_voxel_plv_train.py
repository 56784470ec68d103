"""`make dyn_voxel`'s head trained against the recorded reference (tests/golden/train_parity_dyn_voxel_plv.json: the reference's
runner.main on the analytic dynamic scene with --refl-kind pos-linear-view, tools/ref_train_fixture.py dyn_voxel_plv) by the mechanism of
tests/test_gpu_dyn_voxel_train.py: the reference's argv plus this build's --voxel-refl-order 4, its random stream, procedural initial
grids, deterministic accumulation."""
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
    from nerf_atlas_amd import config, nerf, refl
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_dyn_voxel_plv.json")))
    data = make_scene(str(tmp_path_factory.mktemp("dvp") / "scene"), **fx["scene"]) + "/"
    out = []
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        for _ in range(2):
            args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")] + ["--voxel-refl-order", "4"])
            assert args.epochs == len(fx["losses"]) == 200 and args.dyn_model == "voxel" and args.refl_kind == "pos-linear-view"
            out.append(T.fit(args, replay_reference_rng=True, init=procedural_init))
            m = out[-1]["model"]
            assert type(m) is nerf.DynamicNeRFVoxel and type(m.refl) is refl.PosLinearView and tuple(m.canonical.rgb.shape) == (64, 64, 64, 28)
    finally:
        config.set_deterministic(False)
    return fx, out


def test_training_tracks_the_reference(runs):
    """The first 5 losses within the project's 2e-4; the recipe learns, asserted on the reference's own curve.

    END POINT.  The reference was recorded twice, under 8 and 2 threads (`other_runs` in the fixture): its own two runs differ by 3.4e-4
    in the worst loss and by 0.0060 / 0.0030 / 0.0806 dB in the three test views -- inside the project's 0.1 dB, so THAT bar applies: every
    test view within 0.1 dB of the committed (8-thread) run.  (The chaotic-recipe rule, 3 x the reference's own range = 0.24 dB, is the
    one that does NOT apply here.)  The two deformation-grid TV terms of the first iterations pin the draw order as in the `pos` recipe."""
    fx, (res, _) = runs
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    own = fx["other_runs"][0]
    tv_got, tv_ref = np.array(res["tv_terms"])[:, 2:], np.array(fx["tv_terms"])
    print(f"[dyn voxel plv parity] |loss - ref| first 5 {np.abs(got[:5] - ref[:5]).max():.2e}, all 200 {np.abs(got - ref).max():.2e} (the "
          f"reference's own {own['threads']}-thread run: {own['loss_linf']:.2e}); test PSNR {np.round(res['test_psnr'], 4).tolist()} vs "
          f"{np.round(fx['test_psnr'], 4).tolist()}: {d.max():.4f} dB (the reference's own runs: {own['psnr_linf']:.4f} dB); TV terms first 5 "
          f"{np.abs(tv_got[:5] - tv_ref[:5]).max():.2e}")
    assert own["psnr_linf"] <= 0.1, "the reference's own runs left the 0.1 dB bar: the chaotic-recipe rule would apply"
    assert ref[-20:].mean() < 0.5 * ref[:20].mean(), "the recipe must actually learn"
    assert np.abs(got[:5] - ref[:5]).max() <= 2e-4
    assert tv_got.shape == tv_ref.shape and np.abs(tv_got[:5] - tv_ref[:5]).max() <= 2e-4
    assert d.max() <= 0.1, d


def test_the_deterministic_run_is_bitwise_reproducible(runs):
    _, (a, b) = runs
    assert a["losses"] == b["losses"] and a["test_psnr"] == b["test_psnr"]
    for (k, x), (_, y) in zip(a["model"].state_dict().items(), b["model"].state_dict().items()):
        assert torch.equal(x, y), k


def test_runner_cli_runs_the_shipped_recipe_and_writes_the_panels(tmp_path):
    """`make dyn_voxel`'s command line with --voxel-refl-order 4 and without --ffjord-div-decay, shortened, on the analytic dynamic scene:
    it trains and writes test frames with depth, flow and rigidity panels"""
    import numpy as np
    from PIL import Image
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2, dynamic=True) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--data-kind", "dnerf", "--size", "32", "--epochs", "6", "--near", "2", "--far", "6", "--batch-size", "2",
                       "--crop-size", "16", "--model", "voxel", "--dyn-model", "voxel", "-lr", "1e-2", "--loss-fns", "l2", "--test-crop-size", "20",
                       "--depth-images", "--flow-map", "--spline", "4", "--steps", "24", "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4",
                       "--voxel-tv-bezier", "1e-4", "--voxel-tv-rigidity", "1e-4", "--higher-end-chance", "1", "--offset-decay", "30",
                       "--sigmoid-kind", "upshifted", "--voxel-random-spline-len-decay", "1e-5", "--notraintest", "--seed", "-1",
                       "--refl-kind", "pos-linear-view", "--voxel-refl-order", "4", "--rigidity-map", "--quiet", "--outdir", str(out),
                       "--save", str(tmp_path / "m.pt")])
    assert len(res["losses"]) == 6 and all(l == l for l in res["losses"]) and len(res["maps"]) == 2
    for maps in res["maps"]:
        assert {k: tuple(v.shape) for k, v in maps.items()} == {"depth": (32, 32, 1), "flow": (32, 32, 3), "rigidity": (32, 32, 1)}
        assert all(bool(torch.isfinite(v).all()) for v in maps.values())
    for i in range(2):
        assert np.asarray(Image.open(out / f"test_{i:03}.png")).shape == (32, 5 * 32, 3)   # label | got | depth | flow | rigidity
    sd = torch.load(tmp_path / "m.pt")
    assert tuple(sd["canonical.rgb"].shape) == (64, 64, 64, 28)
