"""Host wiring of the spline-length regularisers (no GPU): the two flags parse with the reference's defaults, a model without
ctrl_pts_grid is refused by the flag's name before the loop, and the header and the binding table agree on the four entry points."""
import pytest

from nerf_atlas_amd import _lib, nerf, train
from test_abi import header_symbols

ARGV = ["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4"]
FLAGS = ("--spline-len-decay", "--voxel-random-spline-len-decay")
SYMBOLS = ("na_grid_spline_len", "na_grid_spline_len_backward", "na_dyn_voxel_spline_len", "na_dyn_voxel_spline_len_backward")


def test_both_flags_parse():
    """`make dyn_voxel` passes --voxel-random-spline-len-decay on its command line"""
    args = train.args_from_argv(ARGV + ["--voxel-random-spline-len-decay", "1e-3", "--spline-len-decay", "0.25"])
    assert args.voxel_random_spline_len_decay == 1e-3 and args.spline_len_decay == 0.25


def test_defaults_are_zero():
    args = train.args_from_argv(ARGV)
    assert args.voxel_random_spline_len_decay == 0.0 and args.spline_len_decay == 0.0
    assert train.DEFAULTS["voxel_random_spline_len_decay"] == 0.0 and train.DEFAULTS["spline_len_decay"] == 0.0
    assert train.make_args().spline_len_decay == 0.0


@pytest.mark.parametrize("flag", FLAGS)
def test_a_model_without_control_point_grids_is_refused_by_name(flag):
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos", flag, "0.1"])
    m = train.load_model(args, is_dyn=False, device="cpu")
    assert type(m) is nerf.NeRFVoxel
    args.epochs = 1
    with pytest.raises(ValueError, match=flag):
        train.train(m, None, None, None, args)


def test_header_and_binding_table_agree_on_the_four_symbols():
    declared = header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["na_grid_spline_len"][1]) == 10 and len(_lib.SIGNATURES["na_grid_spline_len_backward"][1]) == 10
    assert len(_lib.SIGNATURES["na_dyn_voxel_spline_len"][1]) == 12 and len(_lib.SIGNATURES["na_dyn_voxel_spline_len_backward"][1]) == 12


def test_spline_len_needs_a_forward_first():
    args = train.args_from_argv(ARGV)
    m = train.load_model(args, is_dyn=True, device="cpu")
    with pytest.raises(RuntimeError, match="render first"):
        m.spline_len()
