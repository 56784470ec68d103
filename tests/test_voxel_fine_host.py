"""--voxel-steps-fine on the host side (no device): the flag, its refusals, the attribute and the four entry points' declarations."""
import pytest
import torch

from nerf_atlas_amd import _lib, nerf, train
from test_abi import header_symbols

VOXEL = ["--model", "voxel", "--refl-kind", "pos"]
SYMBOLS = ("na_voxel_proposal", "na_voxel_render_rayts", "na_voxel_plv_render_rayts", "na_voxel_sh_render_rayts")


def test_flag_parses_with_default_zero():
    assert train.DEFAULTS["voxel_steps_fine"] == 0
    assert train.args_from_argv(VOXEL).voxel_steps_fine == 0
    assert train.args_from_argv(VOXEL + ["--voxel-steps-fine", "24"]).voxel_steps_fine == 24
    assert train.make_args(voxel_steps_fine=8).voxel_steps_fine == 8


@pytest.mark.parametrize("head", (["--refl-kind", "pos"], ["--refl-kind", "pos-linear-view", "--voxel-refl-order", "2"],
                                  ["--refl-kind", "sph-har", "--voxel-sh-order", "1"]), ids=("pos", "plv", "sh"))
def test_load_model_sets_the_attribute(head):
    m = train.load_model(train.args_from_argv(["--model", "voxel"] + head + ["--voxel-steps-fine", "12"]), device="cpu")
    assert type(m) is nerf.NeRFVoxel and m.steps_fine == 12
    assert train.load_model(train.args_from_argv(["--model", "voxel"] + head), device="cpu").steps_fine == 0


def test_the_five_refusals_name_the_flag():
    load = lambda argv, **k: train.load_model(train.args_from_argv(argv), device="cpu", **k)
    with pytest.raises(ValueError, match="--voxel-steps-fine"):       # negative
        load(VOXEL + ["--voxel-steps-fine", "-1"])
    with pytest.raises(ValueError, match="--voxel-steps-fine 8 over --model plain"):   # another model
        load(["--model", "plain", "--refl-kind", "view", "--voxel-steps-fine", "8"])
    with pytest.raises(ValueError, match="--voxel-steps-fine 8 with --dyn-model voxel"):   # the voxel D-NeRF
        load(VOXEL + ["--dyn-model", "voxel", "--spline", "4", "--voxel-steps-fine", "8"], is_dyn=True)
    with pytest.raises(ValueError, match="--voxel-steps-fine 8 with --dyn-model"):   # is_dyn alone (the loader's own argument)
        load(VOXEL + ["--voxel-steps-fine", "8"], is_dyn=True)
    with pytest.raises(ValueError, match="--voxel-steps-fine 8 with --steps-fine 4"):   # both flags
        load(VOXEL + ["--voxel-steps-fine", "8", "--steps-fine", "4"])
    with pytest.raises(ValueError, match="--voxel-steps-fine 8 with --steps-fine 4"):
        load(["--model", "plain", "--refl-kind", "view", "--voxel-steps-fine", "8", "--steps-fine", "4"])


def test_steps_fine_over_voxel_keeps_its_own_message():
    with pytest.raises(ValueError, match=r"--steps-fine 8 \(coarse -> fine training\) needs --model plain .*got --model voxel"):
        train.load_model(train.args_from_argv(VOXEL + ["--steps-fine", "8"]), device="cpu")


def test_steps_fine_is_a_plain_attribute():
    m = nerf.NeRFVoxel(resolution=4)
    assert m.steps_fine == 0
    m.steps_fine = 16
    assert "steps_fine" not in m.state_dict() and list(m.state_dict()) == ["densities", "rgb"]
    assert "steps_fine" not in dict(m.named_buffers()) and "steps_fine" not in dict(m.named_parameters())
    m2 = nerf.NeRFVoxel(resolution=4)
    m2.load_state_dict(m.state_dict(), strict=True)
    assert m2.steps_fine == 0


def test_header_and_binding_table_agree_on_the_entry_points():
    declared = header_symbols()
    for name in SYMBOLS + ("na_voxel_fine_lanes",):
        assert name in declared and name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["na_voxel_proposal"]
    assert len(args) == 10
    assert [len(_lib.SIGNATURES[n][1]) for n in SYMBOLS[1:]] == [15, 15, 16]


def test_forward_dispatches_on_the_attribute(monkeypatch):
    m = nerf.NeRFVoxel(resolution=4, steps=4)
    seen = []
    monkeypatch.setattr(nerf.NeRFVoxel, "forward_coarse_fine", lambda self, rays, n, u=None: seen.append(n) or "fine")
    m.steps_fine = 5
    assert m(torch.zeros(2, 6)) == "fine" and seen == [5]
