"""The spherical-harmonic colour head (`--refl-kind sph-har`, src/refl.py:696-731) off the GPU: registry, constructor protocol,
state_dict layout against the reference's (tests/golden/g20_plain_sph-har_o*.npz hold its parameter names and shapes), and the
command line down to refl.load."""
import pytest
import torch

from conftest import load_golden


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_state_dict_has_the_reference_layout(order):
    from nerf_atlas_amd import refl
    h = load_golden(f"g20_plain_sph-har_o{order}")
    r = refl.refl_kinds["sph-har"](latent_size=64, act="upshifted", out_features=3, order=order)
    assert isinstance(r, refl.SphericalHarmonic) and isinstance(r, refl.Reflectance)
    assert r.order == order and r.mlp.out.out_features == 3 * (order + 1) ** 2
    want = [(n[len("refl."):], tuple(int(s) for s in shp.split(","))) for n, shp in
            zip(h["param_names"].tolist(), h["param_shapes"].tolist()) if n.startswith("refl.")]
    got = [(k, tuple(v.shape)) for k, v in r.state_dict().items()]
    assert len(want) == 15 and got == want
    # the reference's initialisation: xavier weights, zero biases, a frozen random basis of sigma 32
    assert float(r.mlp.init.bias.detach().abs().max()) == 0.0 and not r.mlp.enc.basis.requires_grad
    assert not r.can_use_normal and not r.can_use_light


def test_default_order_and_rejected_arguments():
    from nerf_atlas_amd import refl
    assert refl.refl_kinds["sph-har"](latent_size=64, act="thin").order == 2
    for bad in (5, -1):
        with pytest.raises((ValueError, AssertionError)):
            refl.refl_kinds["sph-har"](latent_size=64, act="upshifted", out_features=3, order=bad)
    with pytest.raises((NotImplementedError, ValueError, AssertionError)):
        refl.refl_kinds["sph-har"](latent_size=64, act="upshifted", out_features=3, view="raw")


def test_refl_order_reaches_refl_load():
    from nerf_atlas_amd import refl, train
    assert train.make_args().refl_order == 2
    a = train.make_args(refl_order=3, refl_kind="sph-har", sigmoid_kind="leaky_relu")
    r = refl.load(a, a.refl_kind, a.space_kind, 64)
    assert isinstance(r, refl.SphericalHarmonic) and r.order == 3 and r.act_kind == "leaky_relu" and r.latent_size == 64
    a = train.args_from_argv(["-d", "scene/", "--model", "plain", "--refl-kind", "sph-har", "--sigmoid-kind", "leaky_relu", "-lr", "1e-3",
                              "--refl-order", "3"])
    assert a.refl_order == 3 and a.learning_rate == 1e-3
    r = refl.load(a, a.refl_kind, a.space_kind, 67)  # (DynamicNeRF with three refl_latent columns)
    assert r.order == 3 and r.mlp.init.in_features == 2 + 256 + 67
    # without the flag: the reference's default; the other heads do not see the argument
    a = train.args_from_argv(["-d", "scene/", "--refl-kind", "sph-har"])
    assert refl.load(a, a.refl_kind, a.space_kind, 64).order == 2
    a = train.make_args(refl_order=4, refl_kind="pos")
    assert isinstance(refl.load(a, a.refl_kind, a.space_kind, 64), refl.Positional)


def test_whole_model_builds_from_the_command_line():
    from nerf_atlas_amd import nerf, refl, train
    a = train.args_from_argv(["-d", "scene/", "--model", "plain", "--refl-kind", "sph-har", "--sigmoid-kind", "leaky_relu", "-lr", "1e-3"])
    m = train.load_model(a, device="cpu")
    assert isinstance(m, nerf.PlainNeRF) and isinstance(m.refl, refl.SphericalHarmonic) and m.refl.mlp.latent_size == 64
    h = load_golden("g20_plain_sph-har_o2")
    sd = m.state_dict()
    for n, shp in zip(h["param_names"].tolist(), h["param_shapes"].tolist()):
        assert n in sd and tuple(sd[n].shape) == tuple(int(s) for s in shp.split(",")), n


def test_relighting_heads_stay_out_of_scope():
    from nerf_atlas_amd import refl
    for k in ("cook-torrance", "diffuse", "rusin", "fourier", "weighted"):
        with pytest.raises(NotImplementedError):
            refl.refl_kinds[k]()


def test_the_head_has_no_cpu_implementation():
    from nerf_atlas_amd import refl
    r = refl.refl_kinds["sph-har"](latent_size=4, act="upshifted", out_features=3, order=1).eval()
    with torch.no_grad(), pytest.raises(ValueError):
        r(torch.zeros(5, 3), torch.ones(5, 3), latent=torch.zeros(5, 4))
