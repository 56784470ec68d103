"""CPU-side checks of the Fourier encoder's position gradient (csrc/fourier_grad.hip) and of the pairing it opens, D-NeRF over VolSDF's
MLP SDF network (`make dnerf_volsdf`, reference makefile:127-133): the fp64 restatement the GPU tests measure against reproduces the
reference's fp64 autograd, the ruler `ref32_dev` is what the reference's own fp32 autograd costs, the recipe's command line builds the
model, what stays closed still raises, and the new entry points are declared, bound and exported.  Everything numerical on the device:
tests/test_gpu_fourier_grad.py."""
import json
import os
import re

import numpy as np
import pytest
import torch

import fourier_grad_ref as R
from conftest import GOLDEN, REPO, load_golden

NEW_SYMBOLS = ["na_fourier_rows", "na_fourier_encode_backward_input", "na_fourier_encode_backward_input_saved"]
RECIPE = ["--model", "volsdf", "--sdf-kind", "mlp", "--data-kind", "dnerf", "--dyn-model", "plain", "--spline", "6", "--refl-kind",
          "pos-linear-view", "--sigmoid-kind", "upshifted", "--near", "2", "--far", "6", "-lr", "3e-4", "--loss-fns", "l2"]


def test_fp64_restatement_reproduces_the_reference():
    h = R.fixture()
    assert len(R.CASES) == 36
    worst = 0.0
    for case in R.CASES:
        x, basis, g = R.case_inputs(*case)
        assert x.shape == (257, case[1]) and basis.shape == (case[1], case[0]) and g.shape == (257, 2 * case[0]) and np.abs(x).max() > 5.9
        want = h["gx64." + R.tag(*case)]
        got = R.gx_ref(x, basis, case[2], g)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    print(f"\n[fourier_grad] fp64 restatement vs the reference's fp64 autograd: {worst:.2e} of the largest entry")
    assert worst <= 1e-12


def test_ref32_dev_is_argument_rounding():
    """The ruler: the reference's own fp32 autograd deviates from fp64 by about the rounding of its O(10^2 - 10^3) arguments -- a few 1e-6
    to 1e-4 of sum |be| (|g_sin| + |g_cos|) -- and never by nothing (a zero ruler would make the GPU bar unmeetable)."""
    devs = {case: R.ref32_dev(*case) for case in R.CASES}
    lo, hi = min(devs.values()), max(devs.values())
    print(f"\n[fourier_grad] ref32_dev over the 36 cases: {lo:.2e} .. {hi:.2e}")
    for (F, D, scale, sigma), v in devs.items():
        x, basis, _ = R.case_inputs(F, D, scale, sigma)
        half_ulp = float(np.spacing(np.float32(np.abs(x.astype(np.float64) @ (scale * basis.astype(np.float64))).max()))) / 2
        assert 0.02 * half_ulp <= v <= 8 * half_ulp, ((F, D, scale, sigma), v, half_ulp)


def test_recipe_command_line_builds_dnerf_over_volsdf():
    from nerf_atlas_amd import nerf, neural_blocks, refl, sdf, train
    args = train.args_from_argv(["-d", "s/"] + RECIPE)
    m = train.load_model(args, is_dyn=True, device="cpu")
    assert type(m) is nerf.DynamicNeRF and type(m.canonical) is nerf.VolSDF and type(m.sdf.underlying) is sdf.MLP
    assert type(m.sdf.underlying.mlp.enc) is neural_blocks.FourierEncoder and m.sdf.underlying.mlp.dim_p == 3 + 256
    assert type(m.refl) is refl.PosLinearView and m.spline_n == 6 and m.delta_estim.out.out_features == 19
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_dnerf_volsdf.json")))
    assert fx["recipe"]["model_argv"] == RECIPE and len(fx["losses"]) == fx["recipe"]["epochs"] == 30
    sp = json.load(open(os.path.join(GOLDEN, "train_spread_dnerf_volsdf.json")))["dnerf_volsdf"]["reference_runs"]
    assert sp[0]["test_psnr"] == fx["test_psnr"] and len(sp) >= 3


def test_state_dict_has_the_reference_layout():
    from nerf_atlas_amd import nerf, refl, sdf
    for name, kind, spline in (("view_s4", "view", 4), ("plv_s6", "pos-linear-view", 6)):
        h = load_golden("g22_dnerf_volsdf_" + name)
        s = sdf.SDF(sdf.MLP(intermediate_size=64), refl.View(latent_size=64, act="upshifted", out_features=3), isect=None, t_near=0.3, t_far=1.8)
        m = nerf.DynamicNeRF(canonical=nerf.VolSDF(sdf=s, steps=8, t_near=0.3, t_far=1.8, sigmoid_kind="upshifted"), spline=spline)
        m.set_refl(refl.refl_kinds[kind](latent_size=m.intermediate_size, act="upshifted", out_features=3))
        mine = {k: ",".join(str(d) for d in v.shape) for k, v in m.state_dict().items() if v.numel() > 0 and not k.endswith(("scale", "primes"))}
        theirs = dict(zip(h["param_names"].tolist(), h["param_shapes"].tolist()))
        assert mine == theirs
        assert set(h["grad_names"].tolist()) == {k for k, p in m.named_parameters() if p.numel() > 0 and not k.endswith("basis")}


def test_what_stays_closed():
    from nerf_atlas_amd import neural_blocks, train
    # the boundary of this pairing: NeRFAE under the same deformation model stays refused (tests/test_ae.py holds the original assertion)
    with pytest.raises(NotImplementedError, match="FourierEncoder"):
        train.load_model(train.args_from_argv(["-d", "s/", "--model", "ae", "--dyn-model", "plain", "--spline", "4"]), is_dyn=True, device="cpu")
    # the reference cannot run a reflectance latent over VolSDF (tools/gen_golden.py g22)
    with pytest.raises(NotImplementedError, match="dyn-refl-latent"):
        train.load_model(train.args_from_argv(["-d", "s/"] + RECIPE + ["--dyn-refl-latent", "3"]), is_dyn=True, device="cpu")
    x = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(NotImplementedError, match="PositionalEncoder"):
        neural_blocks.PositionalEncoder(input_dims=3)(x)
    with pytest.raises(NotImplementedError, match="LearnedFourierEncoder"):
        neural_blocks.LearnedFourierEncoder(input_dims=3)(x)
    with pytest.raises(ValueError):  # the differentiable encoder has no CPU implementation either
        neural_blocks.FourierEncoder(input_dims=3)(x)


def test_new_entry_points_are_declared_bound_and_exported():
    from nerf_atlas_amd import _lib, build
    src = open(os.path.join(REPO, "include", "nerf_atlas_amd.h")).read()
    declared = set(re.findall(r"\b(na_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    units = [u for u in build.UNITS if u[0] == "fourier_grad.hip"]
    assert len(units) == 1 and units[0][3] == "hazard", "one unit, built with the hazard scans, outside the render_ls units (their ISA pin stays)"
    # argument checks that need no device: shapes are refused before anything is launched
    z = lambda *a: lib.na_fourier_encode_backward_input(*a)
    assert z(None, 4, 9, None, 4, 1.0, None, 8, 0, 0, None, None) != 0       # D > 8
    assert z(None, 4, 3, None, 4, 1.0, None, 7, 0, 0, None, None) != 0       # 2F columns do not fit the pitch
    assert z(None, 4, 3, None, 4, 1.0, None, 11, 2, 1, None, None) != 0      # lead columns overlap the features
    assert z(None, 4, 3, None, 4, 1.0, None, 11, 3, 1, None, None) != 0      # null pointers
    assert z(None, 0, 3, None, 4, 1.0, None, 11, 3, 1, None, None) == 0      # empty batch
    assert lib.na_fourier_rows(None, 4, 3, None, 4, 1.0, None, 5, 4, None, None) != 0  # latent pitch below its width
    assert lib.na_fourier_rows(None, 0, 3, None, 4, 1.0, None, 0, 0, None, None) == 0
