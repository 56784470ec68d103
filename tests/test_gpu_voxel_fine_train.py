"""--voxel-steps-fine through train.fit: the static voxel model trained coarse -> fine on the analytic Blender-format scene
of the other training tests -- finite losses, the test render on the same route, reproducible under config.set_deterministic, composing
with --voxel-upsample and --voxel-tv-sigma, and nothing of it running with the flag at 0."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools.make_scene import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu


def scene(tmp_path):
    return make_scene(str(tmp_path / "s"), size=16, n_train=2, n_test=1) + "/"


def args(T, data, **kw):
    base = dict(data=data, model="voxel", refl_kind="pos", steps=8, voxel_steps_fine=8, size=16, crop_size=8, batch_size=1, epochs=25,
                learning_rate=1e-2)
    base.update(kw)
    return T.make_args(**base)


def test_training_is_finite_renders_coarse_to_fine_and_is_reproducible(tmp_path):
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    data = scene(tmp_path)
    config.set_deterministic(True)
    try:
        runs = [T.fit(args(T, data)) for _ in range(2)]
    finally:
        config.set_deterministic(False)
    losses = runs[0]["losses"]
    assert len(losses) == 25 and all(l == l and abs(l) != float("inf") for l in losses)
    print(f"\n[voxel coarse-fine fit 8 + 8] loss {sum(losses[:5]) / 5:.4f} -> {sum(losses[-5:]) / 5:.4f}, test PSNR {runs[0]['test_psnr_mean']:.2f} dB")
    assert runs[0]["losses"] == runs[1]["losses"]
    nerf_ = runs[0]["model"].nerf
    assert nerf_.steps_fine == 8 and nerf_.ts_ray is not None and nerf_.ts_ray.shape[-1] == 16   # the test render went coarse -> fine
    assert not hasattr(nerf_, "coarse")
    assert all(p == p for p in runs[0]["test_psnr"])


def test_composes_with_upsampling_and_total_variation(tmp_path):
    import nerf_atlas_amd.train as T
    res = T.fit(args(T, scene(tmp_path), voxel_upsample=["10:8"], voxel_tv_sigma=1e-3))
    assert len(res["losses"]) == 25 and all(l == l and abs(l) != float("inf") for l in res["losses"])
    nerf_ = res["model"].nerf
    assert nerf_.resolution == 8 and tuple(nerf_.densities.shape) == (8, 8, 8, 1) and nerf_.ts_ray.shape[-1] == 16


def test_flag_at_zero_runs_none_of_it(tmp_path, monkeypatch):
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import ops
    calls = {"voxel_proposal": 0, "resample_ts": 0}

    def counted(name):
        real = getattr(ops, name)

        def fn(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return fn
    for name in calls:
        monkeypatch.setattr(ops, name, counted(name))
    res = T.fit(args(T, scene(tmp_path), voxel_steps_fine=0, epochs=1))
    assert len(res["losses"]) == 1 and calls == {"voxel_proposal": 0, "resample_ts": 0}, calls
    assert res["model"].nerf.steps_fine == 0 and res["model"].nerf.ts_ray is None
    # ... and the counters do count: one step with the flag goes through both
    T.fit(args(T, scene(tmp_path), epochs=1))
    assert calls["voxel_proposal"] >= 1 and calls["resample_ts"] >= 1, calls
