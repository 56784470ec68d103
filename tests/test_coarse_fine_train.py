"""Coarse -> fine TRAINING (--steps-fine), the parts that need no device: the three new C-ABI entry points are
declared, bound and exported from a unit of their own, they refuse bad arguments before anything is launched, the flag parses and
refuses the pairings the route is not built for, and the `steps_fine` attribute leaves the state_dict alone."""
import os
import re

import pytest

from conftest import REPO

NEW_SYMBOLS = ["na_compute_pts_rayts", "na_composite_rayts", "na_composite_rayts_backward"]


def test_new_symbols_are_declared_bound_and_exported():
    from nerf_atlas_amd import _lib, build
    src = open(os.path.join(REPO, "include", "nerf_atlas_amd.h")).read()
    declared = set(re.findall(r"\b(na_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_SYMBOLS + ["na_composite_rayts_backward_form"]:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    units = [u for u in build.UNITS if u[0] == "composite_rayts.hip"]
    assert len(units) == 1 and units[0][3] == "hazard", "one unit, built with the hazard scans, outside the render_ls units (their ISA pin stays)"


def test_entry_points_refuse_bad_arguments_without_a_device():
    from nerf_atlas_amd import _lib, build
    build.build(verbose=False)
    lib = _lib.load()
    fwd = lambda T, R, C, kind, bg, rand=None: lib.na_composite_rayts(None, None, None, None, T, R, C, kind, bg, rand, None, None, None, None)
    bwd = lambda T, R, C, kind, bg, form, rand=None: lib.na_composite_rayts_backward_form(None, None, None, None, T, R, C, kind, bg, rand, None,
                                                                                         None, None, form, None)
    assert fwd(8, 0, 3, 0, 0) == 0 and bwd(8, 0, 3, 0, 0, 0) == 0                 # R = 0: a no-op
    assert lib.na_compute_pts_rayts(None, 0, None, 8, None, None) == 0
    assert lib.na_composite_rayts_backward(None, None, None, None, 8, 0, 3, 0, 0, None, None, None, None, None) == 0
    assert fwd(0, 4, 3, 0, 0) == -1 and fwd(8, -1, 3, 0, 0) == -1 and fwd(8, 4, 9, 0, 0) == -1   # shapes
    assert fwd(8, 4, 3, 2, 0) == -3 and fwd(8, 4, 3, 0, 3) == -3                    # density kind, background kind
    assert fwd(8, 4, 3, 0, 2) == -2                                                # bg random without the draw
    assert fwd(8, 4, 3, 0, 0) == -2 and bwd(8, 4, 3, 0, 0, 0) == -2                # null pointers
    assert bwd(8, 4, 2, 0, 0, 0) == -3                                             # C of the backward: 1 or 3
    assert bwd(8, 4, 3, 0, 0, 7) == -1                                             # unknown form
    assert lib.na_compute_pts_rayts(None, 4, None, 0, None, None) == -1 and lib.na_compute_pts_rayts(None, 4, None, 8, None, None) == -2
    # the segmented form outside its 17 .. 256 steps is refused with a message, the other forms take any T
    for T in (16, 257, 4096):
        assert bwd(T, 4, 3, 0, 0, 2) == -3 and b"segmented" in lib.na_last_error()
        assert bwd(T, 4, 3, 0, 0, 0) == -2 and bwd(T, 4, 3, 0, 0, 1) == -2         # (past the shape checks: only the pointers are missing)
    assert bwd(17, 4, 3, 0, 0, 2) == -2 and bwd(256, 4, 3, 0, 0, 2) == -2


def test_steps_fine_flag_parses():
    import nerf_atlas_amd.train as T
    assert T.make_args().steps_fine == 0 and T.make_args(steps_fine=16).steps_fine == 16
    assert T.args_from_argv(["-d", "x/", "--steps-fine", "16"]).steps_fine == 16
    assert T.args_from_argv(["-d", "x/"]).steps_fine == 0


@pytest.mark.parametrize("pairing", [dict(model="tiny"), dict(model="volsdf"), dict(model="ae"), dict(refl_kind="pos"),
                                     dict(refl_kind="pos-linear-view"), dict(mip="cone"), dict(dyn_model="plain", spline=6)])
def test_unsupported_pairings_raise_naming_the_flag(pairing):
    import nerf_atlas_amd.train as T
    with pytest.raises(ValueError, match="--steps-fine"):
        T.load_model(T.make_args(steps_fine=16, **pairing), device="cpu")
    with pytest.raises(ValueError, match="--steps-fine"):
        T.load_model(T.make_args(steps_fine=16), is_dyn=True, device="cpu")     # a dynamic data set without the flag
    with pytest.raises(ValueError, match="--steps-fine"):
        T.load_model(T.make_args(steps_fine=-1), device="cpu")


def test_steps_fine_is_a_plain_attribute():
    import nerf_atlas_amd.nerf as nerf
    import nerf_atlas_amd.train as T
    m = nerf.PlainNeRF(steps=8, intermediate_size=64)
    assert m.steps_fine == 0
    keys = list(m.state_dict())
    m.steps_fine = 16
    assert list(m.state_dict()) == keys and not any("steps_fine" in k for k in keys)
    assert "steps_fine" not in dict(m.named_buffers()) and "steps_fine" not in dict(m.named_parameters())
    loaded = T.load_model(T.make_args(steps_fine=16), device="cpu")
    assert isinstance(loaded, nerf.PlainNeRF) and loaded.steps_fine == 16 and list(loaded.state_dict()) == list(T.load_model(T.make_args(), device="cpu").state_dict())
    assert T.load_model(T.make_args(), device="cpu").steps_fine == 0
