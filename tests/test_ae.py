"""CPU-side checks of NeRFAE (`--model ae`; nerf.NeRFAE, csrc/ae_front.hip): the registry, the reference's state_dict layout (names and
shapes recorded from the reference class by tools/gen_golden.py g21), the command line down to the model, the head `load_model` installs,
what keeps raising, and the C ABI of the new entry points.  Everything numerical runs on the GPU: tests/test_gpu_ae.py."""
import os
import re

import pytest
import torch

from conftest import REPO, load_golden

NEW_SYMBOLS = ["na_ae_front_packed_bytes", "na_ae_front_pack", "na_ae_front", "na_row_normalize", "na_row_normalize_backward",
               "na_row_sqnorm_mean", "na_row_sqnorm_mean_backward"]


def test_registry_returns_the_class():
    from nerf_atlas_amd import nerf
    assert nerf.model_kinds["ae"] is nerf.NeRFAE and issubclass(nerf.NeRFAE, nerf.CommonNeRF)
    m = nerf.NeRFAE()
    assert m.encoding_size == 32 and m.intermediate_size == 32 and m.normalize_latent is False and m.regularize_latent is False
    for name in ("encode", "density_tform", "set_regularize_latent", "compute_encoded", "from_encoded", "from_pts", "forward"):
        assert hasattr(m, name), name
    m.set_regularize_latent()
    assert m.regularize_latent is True and m.latent_l2_loss == 0


@pytest.mark.parametrize("case", ["e32_i32_black", "e16_i32", "e32_i64"])
def test_state_dict_has_the_reference_layout(case):
    from nerf_atlas_amd import nerf
    h = load_golden("g21_ae_" + case)
    E, I = int(h["E"]), int(h["I"])
    m = nerf.NeRFAE(steps=16, t_near=2.0, t_far=6.0, intermediate_size=I, encoding_size=E)
    mine = {k: ",".join(str(d) for d in v.shape) for k, v in m.state_dict().items() if v.numel() > 0}
    theirs = dict(zip(h["param_names"].tolist(), h["param_shapes"].tolist()))  # (the reference's zero-size `empty_latent` is not recorded)
    assert mine == theirs
    assert m.refl.mlp.latent_size == E + I and tuple(m.encode.out.weight.shape) == (E, 128)
    assert tuple(m.density_tform.layers[0].weight.shape) == (64, 64 + E) and tuple(m.density_tform.out.weight.shape) == (1 + I, 64)


def test_command_line_reaches_the_model():
    from nerf_atlas_amd import nerf, refl, train
    args = train.args_from_argv(["-d", "s/", "--model", "ae", "--encoding-size", "16", "--normalize-latent", "--latent-l2-weight", "0.1"])
    assert args.encoding_size == 16 and args.normalize_latent is True and args.latent_l2_weight == 0.1
    m = train.load_model(args, device="cpu")
    assert type(m) is nerf.NeRFAE and m.encoding_size == 16 and m.normalize_latent and m.regularize_latent
    assert type(m.refl) is refl.View and m.refl.mlp.latent_size == 16 + args.shape_to_refl_size == 80
    # defaults of runner.py:412-416, and the weight is zeroed for every other model (src/nerf.py:113)
    d = train.args_from_argv(["-d", "s/", "--model", "ae"])
    assert (d.encoding_size, d.normalize_latent, d.latent_l2_weight) == (32, False, 0.0)
    m = train.load_model(d, device="cpu")
    assert not m.regularize_latent and m.refl.mlp.latent_size == 32 + 64
    p = train.args_from_argv(["-d", "s/", "--model", "plain", "--latent-l2-weight", "0.5"])
    train.load_model(p, device="cpu")
    assert p.latent_l2_weight == 0


def test_two_launch_shape_from_the_command_line():
    from nerf_atlas_amd import train
    args = train.args_from_argv(["-d", "s/", "--model", "ae", "--shape-to-refl-size", "32"])
    m = train.load_model(args, device="cpu").eval()
    assert m.refl.mlp.latent_size == 64 and m._head_ok(None)
    assert not train.load_model(train.args_from_argv(["-d", "s/", "--model", "ae"]), device="cpu")._head_ok(None)


def test_what_keeps_raising():
    from nerf_atlas_amd import nerf, train
    with pytest.raises(NotImplementedError):  # DynamicNeRFAE calls a time_estim that does not exist (src/nerf.py:1449-1469)
        train.load_model(train.args_from_argv(["-d", "s/", "--model", "ae", "--dyn-model", "ae", "--spline", "4"]), is_dyn=True, device="cpu")
    with pytest.raises(NotImplementedError, match="FourierEncoder"):
        train.load_model(train.args_from_argv(["-d", "s/", "--model", "ae", "--dyn-model", "plain", "--spline", "4"]), is_dyn=True, device="cpu")
    with pytest.raises(NotImplementedError, match="mip"):
        train.load_model(train.args_from_argv(["-d", "s/", "--model", "ae", "--mip", "cone"]), device="cpu")
    assert nerf.dyn_model_kinds["ae"] is not nerf.DynamicNeRF


def test_cpu_tensors_are_refused():
    from nerf_atlas_amd import nerf, ops
    m = nerf.NeRFAE(steps=4, t_near=2.0, t_far=6.0).eval()
    rays, ts = torch.zeros(5, 6), torch.linspace(2, 6, 4)
    with torch.no_grad():
        with pytest.raises(ValueError):
            m.front_rows(rays, ts)
        with pytest.raises(ValueError):
            m.from_pts(torch.zeros(4, 5, 3), ts, rays[:, :3], rays[:, 3:], rays=rays)
    with pytest.raises(ValueError):
        ops.ae_front(rays, ts, torch.zeros(3, 128), torch.zeros(16, dtype=torch.uint8), "bf16x3", 32, 32)
    with pytest.raises(ValueError):
        ops.row_normalize(torch.zeros(4, 32))
    with pytest.raises(ValueError):
        ops.row_sqnorm_mean(torch.zeros(4, 32))


def test_new_entry_points_are_declared_bound_and_exported():
    from nerf_atlas_amd import _lib, build
    src = open(os.path.join(REPO, "include", "nerf_atlas_amd.h")).read()
    declared = set(re.findall(r"\b(na_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    # shapes the front kernel is instantiated for; everything else has no packed form (the host then runs the per-layer path)
    for E in (16, 32, 64):
        for I in (32, 64):
            assert lib.na_ae_front_packed_bytes(1, E, I) > 0 and lib.na_ae_front_packed_bytes(3, E, I) == lib.na_ae_front_packed_bytes(1, E, I)
    assert lib.na_ae_front_packed_bytes(1, 48, 32) == 0 and lib.na_ae_front_packed_bytes(1, 32, 16) == 0
    assert lib.na_ae_front_packed_bytes(2, 32, 32) == 0  # plain f16: not a precision of this kernel
    assert any(u[0] == "ae_front.hip" and u[3] for u in build.UNITS), "the unit is built with the hazard scans"
