"""--model voxel --refl-kind pos-linear-view --voxel-refl-order K on the host side (no device): the flag's parsing and refusals, the
head's voxel form, the redraw of `rgb`, parameter names and a reference-shaped checkpoint."""
import pytest
import torch

from nerf_atlas_amd import nerf, ops, refl, train

PLV = ["--model", "voxel", "--refl-kind", "pos-linear-view"]


def test_flag_parses_and_defaults_to_unset():
    assert train.args_from_argv(PLV).voxel_refl_order is None and train.make_args().voxel_refl_order is None
    assert train.args_from_argv(PLV + ["--voxel-refl-order", "4"]).voxel_refl_order == 4
    with pytest.raises(SystemExit):
        train.args_from_argv(PLV + ["--voxel-refl-order", "four"])


def test_bare_command_line_still_raises_by_name_and_names_the_flag():
    with pytest.raises(NotImplementedError, match="pos-linear-view") as err:
        train.load_model(train.args_from_argv(PLV), device="cpu")
    assert "--voxel-refl-order" in str(err.value)
    # the head itself, built without an order, has no voxel form and keeps both MLPs
    r = refl.PosLinearView(act="thin", latent_size=0, out_features=3)
    with pytest.raises(NotImplementedError, match="pos-linear-view"):
        r.to_voxel()
    assert hasattr(r, "pos") and hasattr(r, "view")


@pytest.mark.parametrize("k", (-1, 5, 17))
def test_order_outside_0_to_4_is_a_value_error(k):
    with pytest.raises(ValueError, match="--voxel-refl-order"):
        train.load_model(train.args_from_argv(PLV + ["--voxel-refl-order", str(k)]), device="cpu")
    with pytest.raises(ValueError, match="--voxel-refl-order"):
        refl.PosLinearView(act="thin", latent_size=0, out_features=3, voxel_order=k)


def test_flag_over_another_model_or_head_is_a_value_error_by_name():
    with pytest.raises(ValueError, match="--voxel-refl-order 4 over --model plain"):
        train.load_model(train.args_from_argv(["--model", "plain", "--refl-kind", "pos-linear-view", "--voxel-refl-order", "4"]), device="cpu")
    for kind in ("pos", "view", "sph-har"):
        with pytest.raises(ValueError, match=f"--voxel-refl-order 2 with --refl-kind {kind}"):
            train.load_model(train.args_from_argv(["--model", "voxel", "--refl-kind", kind, "--voxel-refl-order", "2"]), device="cpu")
    # without the flag those heads raise exactly as before
    with pytest.raises(NotImplementedError, match="sph-har"):
        train.load_model(train.args_from_argv(["--model", "voxel", "--refl-kind", "sph-har"]), device="cpu")
    with pytest.raises(NotImplementedError, match="does not have a voxel repr"):
        train.load_model(train.args_from_argv(["--model", "voxel", "--refl-kind", "view"]), device="cpu")


@pytest.mark.parametrize("k", range(5))
def test_to_voxel_deletes_both_mlps_and_set_refl_redraws_rgb(k):
    r = refl.PosLinearView(act="thin", latent_size=0, out_features=3, voxel_order=k)
    assert hasattr(r, "pos") and hasattr(r, "view")
    m = nerf.NeRFVoxel(resolution=4)
    before = m.rgb.detach().clone()
    m.set_refl(r)
    C = 3 + (k + 1) ** 2
    assert not hasattr(r, "pos") and not hasattr(r, "view") and not list(r.parameters()) and m.refl is r
    assert (r.order, r.num_sh_coeffs) == (k, (k + 1) ** 2) and m.brdf == r.pos_linear_voxel_forward
    assert tuple(m.rgb.shape) == (4, 4, 4, C) and 0 <= float(m.rgb.data.min()) and float(m.rgb.data.max()) < 1
    assert not torch.equal(m.rgb.detach()[..., :3], before)
    assert [(n, tuple(v.shape)) for n, v in m.state_dict().items()] == [("densities", (4, 4, 4, 1)), ("rgb", (4, 4, 4, C))]
    assert m._plv() and ops.PLV_CHANNELS[C] == k


def test_construction_order_keeps_the_reference_stream_position():
    """the head's two MLPs are built (and draw) BEFORE set_refl redraws rgb, as in the reference: rgb after load_model equals the draw
    that follows the same constructions"""
    args = train.args_from_argv(PLV + ["--voxel-refl-order", "4"])
    torch.manual_seed(7)
    m = train.load_model(args, device="cpu")
    torch.manual_seed(7)
    nerf.NeRFVoxel(resolution=64)
    refl.PosLinearView(act=args.sigmoid_kind, latent_size=0, out_features=3)
    want = torch.rand(64, 64, 64, 28)
    assert type(m) is nerf.NeRFVoxel and type(m.refl) is refl.PosLinearView and torch.equal(m.rgb.detach(), want)


def test_reference_shaped_checkpoint_loads_and_dyn_model_builds():
    args = train.args_from_argv(PLV + ["--voxel-refl-order", "4", "--dyn-model", "voxel", "--spline", "4"])
    m = train.load_model(args, is_dyn=True, device="cpu")
    assert type(m) is nerf.DynamicNeRFVoxel and sorted(m.state_dict()) == ["canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid"]
    assert tuple(m.canonical.rgb.shape) == (64, 64, 64, 28)
    c = train.load_model(train.args_from_argv(PLV + ["--voxel-refl-order", "4"]), device="cpu")
    sd = {"densities": torch.full((4, 4, 4, 1), 0.25), "rgb": torch.arange(4 * 4 * 4 * 28, dtype=torch.float32).reshape(4, 4, 4, 28)}
    c.load_state_dict(sd, strict=True)
    assert c.resolution == 4 and torch.equal(c.rgb.detach(), sd["rgb"]) and bool((c.densities == 0.25).all())
    with pytest.raises(RuntimeError, match="size mismatch"):
        c.load_state_dict({"densities": sd["densities"], "rgb": torch.zeros(4, 4, 4, 3)}, strict=True)


def test_voxel_forward_needs_the_lookups_expansion():
    r = refl.PosLinearView(act="thin", latent_size=0, out_features=3, voxel_order=1)
    r.to_voxel()
    with pytest.raises(ValueError, match="sh"):
        r.pos_linear_voxel_forward(torch.zeros(2, 3), torch.zeros(2, 3))
