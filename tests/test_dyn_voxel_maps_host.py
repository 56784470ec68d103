"""Host wiring of the voxel D-NeRF's test renderer (no GPU): the reference's seven flags parse with its defaults, the C header and the
ctypes table agree on na_dyn_voxel_render, forward_maps refuses training mode by name, and the panel helpers give the reference's
numbers (runner.py:940-947) on a hand-made frame -- with the all-zero flow frame, where the reference divides by zero, mid-grey."""
import os
import re

import pytest
import torch

from nerf_atlas_amd import _lib, nerf, render, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = ["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4"]


def test_the_seven_flags_parse_and_default_to_off():
    a = train.args_from_argv(ARGV)
    assert (a.depth_images, a.flow_map, a.rigidity_map, a.with_alpha) == (False, False, False, False)
    assert (a.render_over_time, a.render_over_time_steps, a.render_over_time_end_sec) == (-1, 100, 1.0)
    assert isinstance(a.render_over_time_end_sec, float)
    a = train.args_from_argv(ARGV + ["--depth-images", "--flow-map", "--rigidity-map", "--with-alpha", "--render-over-time", "2",
                                     "--render-over-time-steps", "7", "--render-over-time-end-sec", "0.5"])
    assert (a.depth_images, a.flow_map, a.rigidity_map, a.with_alpha) == (True, True, True, True)
    assert (a.render_over_time, a.render_over_time_steps, a.render_over_time_end_sec) == (2, 7, 0.5)


def test_make_args_accepts_the_new_keys():
    a = train.make_args(depth_images=True, flow_map=True, rigidity_map=True, with_alpha=True, render_over_time=0, render_over_time_steps=3,
                        render_over_time_end_sec=2.0)
    assert a.depth_images and a.flow_map and a.rigidity_map and a.with_alpha and a.render_over_time == 0
    assert a.render_over_time_steps == 3 and a.render_over_time_end_sec == 2.0
    with pytest.raises(AssertionError, match="unknown arguments"):
        train.make_args(depth_image=True)


def test_header_and_signature_table_agree_on_the_entry_point():
    with open(os.path.join(REPO, "include", "nerf_atlas_amd.h")) as fh:
        text = fh.read()
    m = re.search(r"\bint na_dyn_voxel_render\(([^;]*)\);", text)
    assert m is not None
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    res, args = _lib.SIGNATURES["na_dyn_voxel_render"]
    assert res is _lib.C.c_int and len(args) == len(params) == 23
    for p, ty in zip(params, args):
        want = (_lib.C.c_void_p if p.startswith("void*") else _lib.c_f32p if "float*" in p else _lib.c_i64 if p.startswith("int64_t") else
                _lib.C.c_double if p.startswith("double") else _lib.C.c_int)
        assert ty is want, (p, ty)
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names[:5] == ["rays", "t_ray", "R", "ts", "T"] and names[15:22] == ["out", "depth", "acc", "flow", "rigidity_map", "alpha", "weights"]


def test_the_unit_is_built():
    from nerf_atlas_amd import build
    assert any(u[0] == "dyn_voxel_render.hip" for u in build.UNITS)
    assert os.path.exists(os.path.join(build.CSRC, "dyn_voxel_render.hip"))


def build_model(training):
    args = train.args_from_argv(ARGV)
    m = train.load_model(args, is_dyn=True, device="cpu")
    return m.train() if training else m.eval()


def test_forward_maps_in_training_mode_raises_by_name():
    rays, t = torch.zeros(1, 2, 2, 6), torch.zeros(1)
    with pytest.raises(RuntimeError, match="forward_maps"):
        build_model(True).forward_maps((rays, t))
    with pytest.raises(RuntimeError, match="forward_maps"):          # eval mode, but gradients are being recorded
        build_model(False).forward_maps((rays, t))
    m = build_model(False)
    m.canonical._set_resolution(8)
    with torch.no_grad(), pytest.raises(ValueError, match="the deformation grids have no resampling"):
        m.forward_maps((rays, t))


def test_panels_give_the_references_numbers():
    depth = torch.tensor([[[1.0], [2.0]], [[4.0], [7.0]]])
    assert torch.equal(render.depth_panel(depth, 2.0, 6.0), torch.tensor([[[0.0], [0.0]], [[0.5], [1.0]]]))
    flow = torch.zeros(2, 2, 3)
    flow[0, 0] = torch.tensor([3.0, 0.0, -4.0])       # the largest norm: 5
    flow[1, 1] = torch.tensor([0.0, 1.25, 0.0])
    got = render.flow_panel(flow)
    ref = flow / flow.norm(keepdim=True, dim=-1).max()  # runner.py:944-946, operation by operation
    ref = ref.abs().sqrt().copysign(ref)
    ref = ref.add(1).div(2)
    assert torch.equal(got, ref)
    want00 = torch.tensor([(1 + 0.6 ** 0.5) / 2, 0.5, (1 - 0.8 ** 0.5) / 2])
    assert float((got[0, 0] - want00).abs().max()) <= 1e-7 and float(got[1, 1, 1]) == 0.75 and float(got[0, 1, 0]) == 0.5
    rig = torch.rand(2, 2, 1)
    assert render.rigidity_panel(rig) is rig
    panels = render.map_panels(dict(rigidity=rig, flow=flow, depth=depth), 2.0, 6.0)
    assert [p.shape[-1] for p in panels] == [1, 3, 1] and torch.equal(panels[1], got)      # the reference's order: depth, flow, rigidity
    assert render.map_panels({}, 2.0, 6.0) == []


def test_a_frame_without_flow_is_mid_grey():
    """the reference divides by the largest norm, 0: a NaN image.  Here the image of zero flow."""
    got = render.flow_panel(torch.zeros(3, 3, 3))
    assert torch.equal(got, torch.full((3, 3, 3), 0.5))


def test_render_frame_maps_rejects_an_unknown_map():
    with pytest.raises(ValueError, match="normals"):
        render.render_frame_maps(build_model(False), None, 4, 2, None, want=("depth", "normals"))
