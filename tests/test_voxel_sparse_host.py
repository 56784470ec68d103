"""--voxel-sparsify / NeRFVoxel.sparsify on the host side (no device): the flag's parser and refusals, the buffer `live` in checkpoints,
upsample, the voxel D-NeRF's refusal, the CPU model's refusal, and the entry points' declarations."""
import pytest
import torch

from nerf_atlas_amd import _lib, nerf, ops, train
from test_abi import header_symbols

import voxel_sparse_ref as X

VOXEL = ["--model", "voxel", "--refl-kind", "pos"]
SYMBOLS = ("na_voxel_live_table", "na_voxel_live_samples", "na_voxel_mask_rows", "na_voxel_sparse_render")


# ------------------------------------------------------------------------------------------------------------ the flag
def test_flag_parses_into_a_plan():
    assert train.DEFAULTS["voxel_sparsify"] == []
    assert train.args_from_argv(VOXEL).voxel_sparsify == []
    a = train.args_from_argv(VOXEL + ["--voxel-sparsify", "0:0", "10:1e-2", "20:0.5"])
    assert a.voxel_sparsify == [(0, 0.0), (10, 0.01), (20, 0.5)]
    assert train.make_args(voxel_sparsify=[(3, 0.25)]).voxel_sparsify == [(3, 0.25)]
    assert train.parse_voxel_sparsify(["7:.5"]) == [(7, 0.5)]


@pytest.mark.parametrize("spec", (["5"], ["a:1"], ["-1:0.1"], ["1.5:0.1"], ["1:x"], ["1:-0.1"], ["1:nan"], ["1:inf"], ["1:2:3"],
                                  ["5:0.1", "5:0.2"], ["5:0.1", "3:0.2"], [(-1, 0.1)], [(2, -1.0)], [(1.5, 0.1)]))
def test_bad_plans_name_the_flag(spec):
    with pytest.raises(ValueError, match="--voxel-sparsify"):
        train.parse_voxel_sparsify(spec)


def test_the_refusals_name_the_flag():
    load = lambda argv, **k: train.load_model(train.args_from_argv(argv), device="cpu", **k)
    with pytest.raises(ValueError, match="--voxel-sparsify over --model plain"):
        load(["--model", "plain", "--refl-kind", "view", "--voxel-sparsify", "0:0.01"])
    with pytest.raises(ValueError, match="--voxel-sparsify with --dyn-model voxel"):
        load(VOXEL + ["--dyn-model", "voxel", "--spline", "4", "--voxel-sparsify", "0:0.01"], is_dyn=True)
    with pytest.raises(ValueError, match="--voxel-sparsify with --dyn-model"):
        load(VOXEL + ["--voxel-sparsify", "0:0.01"], is_dyn=True)
    assert type(load(VOXEL + ["--voxel-sparsify", "0:0.01"])) is nerf.NeRFVoxel


def test_d_thresh_is_the_restatement():
    for t in (0, 1e-6, 1e-2, 0.3, 1.0, 50.0, 1e3):
        assert ops.voxel_d_thresh(t) == X.d_thresh(t), t
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.voxel_d_thresh(bad)


# ------------------------------------------------------------------------------------------------------------ the buffer
def table(S, seed=0):
    return (torch.rand(S, S, S, generator=torch.Generator().manual_seed(seed)) < 0.5).to(torch.uint8)


def test_live_is_absent_until_set_and_round_trips_in_all_four_combinations():
    plain, marked = nerf.NeRFVoxel(resolution=4), nerf.NeRFVoxel(resolution=4)
    assert plain.live is None and list(plain.state_dict()) == ["densities", "rgb"]
    marked.live = table(4)
    assert list(marked.state_dict()) == ["densities", "rgb", "live"] and "live" in dict(marked.named_buffers())
    for has_table in (False, True):
        for ckpt in (plain, marked):
            m = nerf.NeRFVoxel(resolution=4)
            if has_table:
                m.live = table(4, 1)
            m.load_state_dict(ckpt.state_dict(), strict=True)
            if ckpt is marked:
                assert torch.equal(m.live, marked.live) and m.live.dtype == torch.uint8
            else:
                assert m.live is None and "live" not in m.state_dict()
            assert torch.equal(m.densities, ckpt.densities)
    # the table follows the checkpoint's resolution like the grids
    big = nerf.NeRFVoxel(resolution=6)
    big.live = table(6)
    m = nerf.NeRFVoxel(resolution=4)
    m.live = table(4)
    m.load_state_dict(big.state_dict(), strict=True)
    assert m.resolution == 6 and torch.equal(m.live, big.live)
    marked.clear_live()
    assert marked.live is None and list(marked.state_dict()) == ["densities", "rgb"]


def test_a_table_of_another_shape_or_type_is_refused():
    m = nerf.NeRFVoxel(resolution=4)
    sd = m.state_dict()
    for bad in (table(6), table(4).float(), table(4)[:2]):
        with pytest.raises(ValueError, match="live"):
            nerf.NeRFVoxel(resolution=4).load_state_dict(dict(sd, live=bad))


def test_upsample_clears_the_table_with_one_warning_line(monkeypatch, capsys):
    m = nerf.NeRFVoxel(resolution=4)
    m.live = table(4)
    # (the resampling itself is a HIP kernel: stand in for it, the subject is the table)
    monkeypatch.setattr(type(m.densities), "is_cuda", property(lambda self: True))
    monkeypatch.setattr(ops, "grid_upsample", lambda g, reso: torch.zeros((reso,) * 3 + (g.shape[-1],)))
    m.upsample(6)
    out = capsys.readouterr().out.strip().splitlines()
    assert m.live is None and m.resolution == 6
    assert len(out) == 1 and out[0].startswith("[warn]") and "sparsify" in out[0]
    m.upsample(8)
    assert capsys.readouterr().out == ""   # nothing to clear, nothing to say


def test_sparsify_on_a_cpu_model_raises_by_name():
    m = nerf.NeRFVoxel(resolution=4)
    with pytest.raises(ValueError, match="NeRFVoxel.sparsify"):
        m.sparsify(1e-2)
    with pytest.raises(ValueError):
        m.sparsify(-1.0)
    with pytest.raises(ValueError):
        m.sparsify(float("nan"))
    assert m.live is None


def test_the_voxel_dnerf_refuses_a_table_by_name():
    c = nerf.NeRFVoxel(resolution=4, steps=4)
    d = nerf.DynamicNeRFVoxel(c, spline=4)
    c.live = table(4)
    rays_t = (torch.zeros(1, 2, 2, 6), torch.zeros(1))
    for who, call in (("forward", lambda: d(rays_t)), ("forward_maps", lambda: d.forward_maps(rays_t)),
                      ("ffjord_div", lambda: d.ffjord_div(torch.zeros(1))), ("sum_jacobian_div", d.sum_jacobian_div),
                      ("spline_len", d.spline_len)):
        with pytest.raises(ValueError, match=f"DynamicNeRFVoxel.{who}.*liveness table"):
            call()


def test_table_checks_of_the_operators():
    den, rgb = torch.zeros(4, 4, 4, 1), torch.zeros(4, 4, 4, 3)
    for bad in (table(6), table(4).float(), table(4).transpose(0, 1), None):
        with pytest.raises(ValueError, match="liveness table"):
            ops._voxel_live(bad, 4, den.device)
    assert ops._voxel_live(table(4), 4, den.device) is not None
    assert ops.VOXEL_DEAD_DENSITY == -1e30 and ops.VOXEL_SPARSE_LANES == 16


# ------------------------------------------------------------------------------------------------------------ declarations
def test_header_and_binding_table_agree_on_the_entry_points():
    declared = header_symbols()
    for name in SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES, name
    assert [len(_lib.SIGNATURES[n][1]) for n in SYMBOLS] == [6, 11, 7, 19]
