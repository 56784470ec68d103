"""Host wiring of --ffjord-div-decay / --dyn-diverge-decay over --dyn-model voxel (no GPU): the two C entry points are declared, a model
whose grids are on the CPU raises by name (the terms are HIP kernels only), the model's two methods raise before a forward, and a
static model keeps its ValueErrors."""
import ctypes as C

import pytest

from nerf_atlas_amd import _lib, nerf, train

ARGV = ["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4"]
FLAGS = ("--ffjord-div-decay", "--dyn-diverge-decay")


def build(extra=()):
    args = train.args_from_argv(ARGV + list(extra))
    args.epochs = 1
    return args, train.load_model(args, is_dyn=True, device="cpu")


def test_signatures_are_declared():
    res, args = _lib.SIGNATURES["na_dyn_voxel_jac_quad"]
    assert res is C.c_int and len(args) == 11 and args[2] is _lib.c_i64 and args[7] is C.c_double and args[-1] is C.c_void_p
    res, args = _lib.SIGNATURES["na_dyn_voxel_jac_quad_backward"]
    assert res is C.c_int and len(args) == 10 and args[2] is _lib.c_i64 and args[5] is C.c_double and args[-1] is C.c_void_p


@pytest.mark.parametrize("flag", FLAGS)
def test_cpu_model_raises_by_name_before_the_data_is_touched(flag):
    args, m = build([flag, "0.3"])
    with pytest.raises(NotImplementedError, match=flag) as e:
        train.train(m, None, None, None, args)   # (cam and labels are None: anything that touched them would be another error)
    assert "GPU only" in str(e.value)


@pytest.mark.parametrize("method", ("ffjord_div", "sum_jacobian_div"))
def test_methods_raise_before_a_forward(method):
    _, m = build()
    call = (lambda: m.ffjord_div(None)) if method == "ffjord_div" else m.sum_jacobian_div
    with pytest.raises(RuntimeError, match=f"DynamicNeRFVoxel.{method}"):
        call()


def test_static_model_keeps_its_value_errors():
    for flag, needle in zip(FLAGS, ("--ffjord-div-decay needs a dynamic model", "--dyn-diverge-decay needs a dynamic model")):
        args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos", flag, "0.1"])
        args.epochs = 1
        m = train.load_model(args, is_dyn=False, device="cpu")
        assert type(m) is nerf.NeRFVoxel
        with pytest.raises(ValueError, match=needle):
            train.train(m, None, None, None, args)


def test_flags_off_do_not_raise_for_the_cpu_model():
    """the new check fires for the two flags only: without them train() goes on to the data (here None, a TypeError / AttributeError of
    its own, not the flags' NotImplementedError)"""
    args, m = build()
    with pytest.raises(Exception) as e:
        train.train(m, None, None, None, args)
    assert not isinstance(e.value, NotImplementedError)
