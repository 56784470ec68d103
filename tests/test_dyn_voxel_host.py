"""Host wiring of --dyn-model voxel (no GPU): the model is built by load_model on the CPU with the reference's parameter names, the
total-variation weights are kept for it, and everything around it that is not built raises by name."""
import pytest
import torch

from nerf_atlas_amd import nerf, refl, train

ARGV = ["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4"]


def build(extra=()):
    args = train.args_from_argv(ARGV + list(extra))
    return args, train.load_model(args, is_dyn=True, device="cpu")


def test_load_model_builds_the_dynamic_voxel_model_on_the_cpu():
    args, m = build()
    assert type(m) is nerf.DynamicNeRFVoxel and type(m.canonical) is nerf.NeRFVoxel and m.nerf is m.canonical
    assert type(m.refl) is refl.Positional and m.sdf is None and m.intermediate_size == 0 and m.total_latent_size() == 0
    S = m.canonical.resolution
    assert tuple(m.ctrl_pts_grid.shape) == (S, S, S, 9) and tuple(m.rigidity_grid.shape) == (S, S, S, 1)
    assert bool((m.rigidity_grid == 0).all()) and 0.25 < float(m.ctrl_pts_grid.data.std()) < 0.35          # zeros / randn * 0.3
    assert m.densities is m.canonical.densities and m.rgb is m.canonical.rgb
    assert all(p.device.type == "cpu" for p in m.parameters())


@pytest.mark.parametrize("spline", (2, 5, 11))
def test_grid_shapes_follow_the_spline(spline):
    m = nerf.DynamicNeRFVoxel(nerf.NeRFVoxel(resolution=4), spline=spline)
    assert tuple(m.ctrl_pts_grid.shape) == (4, 4, 4, 3 * (spline - 1)) and tuple(m.rigidity_grid.shape) == (4, 4, 4, 1)


def test_state_dict_has_the_references_names():
    _, m = build()
    assert set(m.state_dict()) == {"ctrl_pts_grid", "rigidity_grid", "canonical.densities", "canonical.rgb"}
    m.set_bg("white")
    assert m.canonical.bg == "white"


def test_unset_voxel_tv_keeps_all_four_weights():
    args, m = build(["--voxel-tv-sigma", "0.1", "--voxel-tv-rgb", "0.2", "--voxel-tv-bezier", "0.3", "--voxel-tv-rigidity", "0.4"])
    train.unset_voxel_tv(args, m)
    assert (args.voxel_tv_sigma, args.voxel_tv_rgb, args.voxel_tv_bezier, args.voxel_tv_rigidity) == (0.1, 0.2, 0.3, 0.4)
    train.unset_voxel_tv(args, m.canonical)                      # the static model still drops the two it has no grid for
    assert (args.voxel_tv_sigma, args.voxel_tv_rgb, args.voxel_tv_bezier, args.voxel_tv_rigidity) == (0.1, 0.2, 0, 0)


def test_constructor_raises():
    vox = nerf.NeRFVoxel(resolution=4)
    for spline in (1, 0, -3):
        with pytest.raises(ValueError, match="spline"):
            nerf.DynamicNeRFVoxel(vox, spline=spline)
    with pytest.raises(NotImplementedError, match="spline"):
        nerf.DynamicNeRFVoxel(vox, spline=12)
    for canonical in (None, nerf.TinyNeRF(), torch.nn.Linear(1, 1)):
        with pytest.raises(NotImplementedError, match="--model voxel"):
            nerf.DynamicNeRFVoxel(canonical, spline=4)


def test_load_dyn_raises_by_name():
    with pytest.raises(NotImplementedError, match="--dyn-refl-latent"):
        build(["--dyn-refl-latent", "3"])
    args = train.args_from_argv(["--model", "plain", "--dyn-model", "voxel", "--spline", "4"])
    with pytest.raises(NotImplementedError, match="--dyn-model voxel over --model plain"):
        train.load_model(args, is_dyn=True, device="cpu")
    for kind in ("pos-linear-view", "sph-har"):                 # heads without a voxel form built here keep raising by name
        args = train.args_from_argv(ARGV[:2] + ["--refl-kind", kind] + ARGV[4:])
        with pytest.raises(NotImplementedError, match=kind):
            train.load_model(args, is_dyn=True, device="cpu")


def _train_args(extra):
    args, m = build(extra)
    args.epochs = 1
    return args, m


@pytest.mark.parametrize("flag", ("--ffjord-div-decay", "--dyn-diverge-decay"))
def test_divergence_regularisers_raise_by_name(flag):
    args, m = _train_args([flag, "0.1"])
    with pytest.raises(NotImplementedError, match=flag):
        train.train(m, None, None, None, args)


def test_voxel_upsample_raises_for_the_dynamic_model():
    args, m = _train_args(["--voxel-upsample", "1:8"])
    with pytest.raises(ValueError, match="--voxel-upsample with --dyn-model voxel"):
        train.train(m, None, None, None, args)
