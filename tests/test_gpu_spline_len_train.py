"""--spline-len-decay and --voxel-random-spline-len-decay in training (nerf.DynamicNeRFVoxel.spline_len, nerf.arc_len_grid, train.py):
the gradient that reaches ctrl_pts_grid through autograd against tests/spline_len_ref.py, and a short deterministic run."""
import numpy as np
import pytest
import torch

import voxel_ref as V
import spline_len_ref as R

pytestmark = pytest.mark.gpu

ARGV = ["--model", "voxel", "--refl-kind", "pos", "--dyn-model", "voxel", "--spline", "4"]   # tests/test_dyn_voxel_host.py
RUN = ["--near", "2", "--far", "6", "--steps", "16"]
GRIDS = ("canonical.densities", "canonical.rgb", "rigidity_grid")


def build(extra=()):
    from nerf_atlas_amd import train
    args = train.args_from_argv(ARGV + RUN + list(extra))
    torch.manual_seed(7)
    return args, train.load_model(args, is_dyn=True)


def test_both_terms_reach_ctrl_pts_grid_and_nothing_else():
    """one forward + backward at two views (the per-sample term is the weighted mean over all samples at any batch size) with and
    without the two terms, in the deterministic mode so that the image loss's gradient is the same bits in both: the difference on
    ctrl_pts_grid is the sum of the restatement's two gradients within their bounds plus the roundings of autograd's two additions;
    rigidity_grid and the canonical grids receive nothing from the terms"""
    from nerf_atlas_amd import config, nerf
    a, b = 0.7, 0.3
    _, m = build()
    m.eval()   # (no jitter of the steps: both passes see the same samples; the parameters require gradients, so the operator route runs)
    S = m.canonical.resolution
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    t = torch.tensor([0.25, 0.8], device="cuda")
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    idxs = R.indices(4096, S ** 3)
    params = dict(m.named_parameters())
    config.set_deterministic(True)
    try:
        grads = []
        for terms in (False, True):
            for p in params.values():
                p.grad = None
            loss = (m((rays, t)) - target).square().mean()
            if terms:
                loss = loss + a * m.spline_len(m.canonical.weights) + b * nerf.arc_len_grid(m.ctrl_pts_grid, idxs=idxs.cuda())
            loss.backward()
            grads.append({k: p.grad.detach().cpu().clone() for k, p in params.items()})
    finally:
        config.set_deterministic(False)
    plain, full = grads
    for k in GRIDS:
        assert torch.equal(plain[k].view(torch.int32), full[k].view(torch.int32)), k
    ctrl = m.ctrl_pts_grid.detach().cpu()
    pts, w = m.pts.cpu().reshape(-1, 3), m.canonical.weights.detach().cpu().reshape(-1)
    assert pts.shape[0] == 16 * 2 * 8 * 8
    rs = R.dyn_ref(pts, ctrl, 4, w, g_up=a, grid_radius=m.canonical.grid_radius)
    rg = R.grid_ref(ctrl.reshape(S ** 3, -1), R.rows_of_flat(idxs, (S, S, S)), g_up=b)
    img = plain["ctrl_pts_grid"].double().reshape(S ** 3, -1)
    want = img + rs["grad"] + rg["grad"]
    bound = rs["b_grad_det"] + rg["b_grad_det"] + 3 * V.U * (img.abs() + rs["grad"].abs() + rg["grad"].abs())
    ratio = V.worst_ratio(full["ctrl_pts_grid"].reshape(S ** 3, -1), want, bound)
    moved = int(((rs["grad"] != 0) | (rg["grad"] != 0)).any(dim=-1).sum())
    print(f"[spline-length terms through autograd] worst |err| / bound {ratio:.3f} over {moved} rows the terms reach")
    assert ratio <= 1.0 and moved > 4096 // 2


def test_three_iterations_are_finite_and_reproducible():
    """train.train with both weights on: finite losses, three finite rows of last_len_terms (device scalars), and under
    config.set_deterministic two runs from the same seeds end with the same parameter bits"""
    from nerf_atlas_amd import cameras, config, train
    size = 16
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]],
                        [[0.8, -0.36, 0.48, 1.9], [0.0, 0.8, 0.6, 2.4], [-0.6, -0.48, 0.64, 2.6]]], dtype=torch.float32)
    labels = (torch.full((2, size, size, 3), 0.25), torch.tensor([0.0, 1.0]))
    extra = ["--size", str(size), "--crop-size", "8", "--batch-size", "2", "--epochs", "3", "-lr", "1e-2", "--spline-len-decay", "0.1",
             "--voxel-random-spline-len-decay", "0.01"]
    ends = []
    config.set_deterministic(True)
    try:
        for _ in range(2):
            args, m = build(extra)
            cam = cameras.NeRFCamera(cam_to_world=c2w.clone(), focal=0.5 * size / np.tan(0.5 * 0.6911)).to("cuda")
            train.seed(args.seed)
            opt = train.load_optim(args, m.parameters())
            losses = train.train(m, cam, labels, opt, args)
            rows = [[float(v) for v in row] for row in train.train.last_len_terms]
            assert len(losses) == 3 and all(np.isfinite(losses))
            assert len(rows) == 3 and all(len(r) == 2 and np.isfinite(r).all() and min(r) > 0 for r in rows)
            assert all(torch.is_tensor(v) and v.is_cuda for row in train.train.last_len_terms for v in row)
            ends.append({k: p.detach().cpu().clone() for k, p in m.named_parameters()})
    finally:
        config.set_deterministic(False)
    for k in ends[0]:
        assert torch.equal(ends[0][k].view(torch.int32), ends[1][k].view(torch.int32)), k
    assert not torch.equal(ends[0]["ctrl_pts_grid"], build()[1].ctrl_pts_grid.detach().cpu())
