#!/usr/bin/env python3
"""Times of the pos-linear-view voxel head on the GPU (csrc/voxel.hip, na_dyn_voxel_plv_render), written to
profiles/voxel_plv/bench.json.

    python tools/voxel_plv_bench.py [--reps 9] [--inner 20] [--out profiles/voxel_plv]

The method is tools/voxel_bench.py's (device events around `inner` back-to-back calls, every shape warmed up, the sides of a
comparison alternated inside one repetition, the median of `reps` repetitions with min .. max).  Shape: the `make dyn_voxel` crop,
2 views x 44 x 44 rays x 80 steps = 309 760 samples, S = 64, order 4 (C = 28), spline 4, rays from the project's ray generator; and
the 64 x 64 x 80 test tile with all maps.

"torch" rows are what a user would otherwise run: a plain-PyTorch restatement of the reference's head (advanced indexing of [N, 29]
per corner, eval_sh restated from its closed forms, autograd), written for this tool and run on the same GPU in fp32 -- never a kernel
of this project.  Both scatter variants (csrc/voxel.hip: 1 whole rows in the LDS table, 2 leading sums in the table and the
coefficient block straight to memory) are timed in both accumulation modes; the shipped one is NA_PLV_SCATTER's.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tools.voxel_bench import finish, row, timed  # noqa: E402
from tools.dyn_voxel_bench import torch_lookup, torch_warp  # noqa: E402


def torch_sh4(d):
    """the 25 real spherical harmonics of degrees 0..4 at unit directions d [..., 3], the reference's signs; [..., 25]"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
        1.0925484305920792 * xy, -1.0925484305920792 * yz, 0.31539156525252005 * (2 * zz - xx - yy), -1.0925484305920792 * xz,
        0.5462742152960396 * (xx - yy), -0.5900435899266435 * y * (3 * xx - yy), 2.890611442640554 * xy * z,
        -0.4570457994644658 * y * (4 * zz - xx - yy), 0.3731763325901154 * z * (2 * zz - 3 * xx - 3 * yy),
        -0.4570457994644658 * x * (4 * zz - xx - yy), 1.445305721320277 * z * (xx - yy), -0.5900435899266435 * x * (xx - 3 * yy),
        2.5033429417967046 * xy * (xx - yy), -1.7701307697799304 * yz * (3 * xx - yy), 0.9461746957575601 * xy * (7 * zz - 1),
        -0.6690465435572892 * yz * (7 * zz - 3), 0.10578554691520431 * (zz * (35 * zz - 30) + 3), -0.6690465435572892 * xz * (7 * zz - 3),
        0.47308734787878004 * (xx - yy) * (7 * zz - 1), -1.7701307697799304 * xz * (xx - 3 * yy),
        0.6258357354491761 * (xx * (xx - 3 * yy) - yy * (3 * xx - yy))], dim=-1)


def torch_head(params, view):
    """PosLinearView.pos_linear_voxel_forward (src/refl.py:265-272) with the upshifted sigmoid: params [..., 28], view [..., 3]"""
    raw_rgb, co = params.split([3, 25], dim=-1)
    lin = (co * torch_sh4(torch.nn.functional.normalize(view, dim=-1))).sum(dim=-1, keepdim=True).sigmoid()
    return (raw_rgb.sigmoid() + 1e-2) * (lin / 2 + 0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_plv"))
    ap.add_argument("--tag", default="bench")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_plv_ref as P
    import voxel_ref as V
    import dyn_voxel_ref as D
    from nerf_atlas_amd import config, nerf, ops, refl
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    S, T, K, n, gr = 64, 80, 4, 4, 1.3
    C = 3 + (K + 1) ** 2
    den, rgb = (x.to(dev) for x in P.grid_values(S, K))
    ctrl, rig = (x.to(dev) for x in D.dyn_grids(S, n))
    ctrl = ctrl * 0.3
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(2)])).float().to(dev)
    focal = 0.5 * 64 / math.tan(0.5 * FOV_X)
    rays = ops.raygen(c2w, focal, 64, (10, 10, 44, 44))
    ts = torch.linspace(2.0, 6.0, T, device=dev)
    pts = ops.compute_pts(rays, ts)                                   # [T,2,44,44,3]
    N = pts.numel() // 3
    shape = f"N={N} S={S} K={K}"
    rows = []
    grid_bytes = 4 * (1 + C) * S ** 3
    view = rays[..., 3:].unsqueeze(0).expand_as(pts)
    grid29 = torch.cat([den, rgb], dim=-1)

    # ---- the lookup
    def torch_lookup_head():
        raw = torch_lookup(pts, grid29, gr)
        return raw[..., :4], (raw[..., 4:] * torch_sh4(torch.nn.functional.normalize(view, dim=-1))).sum(-1)
    t = timed({"hip": lambda: ops.voxel_plv_sample(den, rgb, gr, rays, pts=pts), "torch": torch_lookup_head}, a.reps, a.inner)
    rows.append(row("voxel_plv_sample (one launch)", t["hip"], shape, N * (12 + 16 + 4) + grid_bytes,
                    note="the gather is 8 rows of 112 B per sample (277 MB of row reads served by the caches: the grid is 30 MB)"))
    rows.append(row("torch lookup [N,29] + eval_sh", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))

    # ---- the scatter: both variants, both modes
    g_raw = torch.from_numpy(V.proc_uniform((N, 4), 5201, 1.0)).to(dev)
    g_sh = torch.from_numpy(V.proc_uniform((N,), 5202, 1.0)).to(dev)
    every = N * 8 * (1 + C) * 4
    for det in (False, True):
        if det:
            config.set_deterministic(True)
        try:
            t = timed({v: (lambda v=v: ops.voxel_plv_sample_backward(g_raw, g_sh, S, K, gr, rays, pts=pts, variant=v)) for v in (1, 2)},
                      a.reps, a.inner)
        finally:
            if det:
                config.set_deterministic(False)
        for v, what in ((1, "whole rows in the LDS table"), (2, "leading sums in the table, coefficients to memory")):
            rows.append(row(f"voxel_plv_sample_backward variant {v}, {'2^-40 fixed point' if det else 'fp32 atomics'}", t[v], shape,
                            atomic_bytes=every * (2 if det else 1),
                            note=what + "; the time includes allocating and zeroing the two gradient tensors"
                            + (" and zeroing and folding the 60.8 MB fixed-point workspace" if det else "")))

    # ---- the position gradient
    wp = pts.clone().requires_grad_(True)

    def torch_pts_grad():
        wp.grad = None
        raw = torch_lookup(wp, grid29, gr)
        s = (raw[..., 4:] * torch_sh4(torch.nn.functional.normalize(view, dim=-1))).sum(-1)
        torch.autograd.backward([raw[..., :4], s], [g_raw.reshape(raw.shape[:-1] + (4,)), g_sh.reshape(s.shape)])
    t = timed({"hip": lambda: ops.voxel_plv_sample_backward_pts(g_raw, g_sh, pts, rays, den, rgb, gr), "torch": torch_pts_grad}, a.reps,
              max(1, a.inner // 2))
    rows.append(row("voxel_plv_sample_backward_pts (gather)", t["hip"], shape, N * (12 + 16 + 4 + 12) + grid_bytes))
    rows.append(row("torch lookup + eval_sh, forward + position gradient", t["torch"], shape,
                    note="plain-torch restatement written for this tool (the baseline)"))

    # ---- the static model: forward + backward
    c = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    c.set_refl(refl.PosLinearView(act="upshifted", latent_size=0, out_features=3, voxel_order=K))
    c = c.to(dev).train()
    target = torch.full(tuple(rays.shape[:-1]) + (3,), 0.5, device=dev)

    def fwd_bwd():
        c.densities.grad = c.rgb.grad = None
        (c(rays) - target).square().mean().backward()
    dt, rt = (x.detach().clone().requires_grad_(True) for x in (c.densities, c.rgb))
    dists = torch.cat([ts[1:] - ts[:-1], torch.full((1,), 1e10, device=dev)])[:, None, None, None] * rays[..., 3:].norm(dim=-1)[None]

    def torch_model():
        dt.grad = rt.grad = None
        raw = torch_lookup(pts, torch.cat([dt, rt], dim=-1), gr)
        alpha = 1 - torch.exp(-torch.nn.functional.softplus(raw[..., 0] - 1) * dists)
        trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:1]), 1 - alpha[:-1] + 1e-10], dim=0), dim=0)
        out = ((alpha * trans)[..., None] * torch_head(raw[..., 1:], view)).sum(dim=0)
        (out - target).square().mean().backward()
    t = timed({"hip": fwd_bwd, "torch": torch_model}, a.reps, max(1, a.inner // 4))
    rows.append(row("NeRFVoxel + pos-linear-view, forward + backward", t["hip"], shape,
                    note="stratified steps drawn per call (training mode); fp32 atomics"))
    rows.append(row("torch model, forward + backward", t["torch"], shape,
                    note="plain-torch restatement written for this tool: what a user would otherwise run"))
    c.eval()
    with torch.no_grad():
        t = timed({"eval": lambda: c(rays)}, a.reps, a.inner)
    rows.append(row("eval route (voxel_plv_render, one launch)", t["eval"], shape))

    # ---- the 64 x 64 x 80 test tile with all maps: one launch against the composition
    tile = ops.raygen(c2w[:1], focal, 64, (0, 0, 64, 64))[0].reshape(-1, 6).contiguous()
    R = tile.shape[0]
    tt = torch.full((R,), 0.4, device=dev)
    ones = torch.ones(T, R, 1, device=dev)
    ones[-1] = 0
    want = ("depth", "acc", "flow", "rigidity")

    def composition():
        p = ops.compute_pts(tile, ts)
        w, dp, r = ops.dyn_voxel_warp(p, tt[None, :].expand(T, R).contiguous(), ctrl, rig, n, gr)
        out, alpha, weights = ops.voxel_plv_render(tile, ts, den, rgb, gr, "upshifted", "black", True, pts=w)
        return (out, ops.integrate(weights, ts[:, None, None].expand(T, R, 1).contiguous()), ops.integrate(weights, ones),
                ops.integrate(weights, (dp * r[..., None]).contiguous()), ops.integrate(weights, r[..., None].contiguous()))
    one = ops.dyn_voxel_render(tile, tt, ts, den, rgb, ctrl, rig, n, gr, "upshifted", "black", want=want, plv=True)
    ref = composition()
    assert all(torch.equal(a_, b_) for a_, b_ in zip((one["rgb"], one["depth"], one["acc"], one["flow"], one["rigidity"]), ref))
    t = timed({"one": lambda: ops.dyn_voxel_render(tile, tt, ts, den, rgb, ctrl, rig, n, gr, "upshifted", "black", want=want, plv=True),
               "composition": composition}, a.reps, a.inner)
    tshape = f"R={R} T={T} S={S} K={K} spline={n}"
    rows.append(row("dyn_voxel_plv_render, all maps (one launch)", t["one"], tshape))
    rows.append(row("composition: pts, warp, voxel_plv_render, integrate x 4", t["composition"], tshape,
                    note="this project's own launches; bit for bit the same result (checked here before timing)"))
    finish(a, rows)


if __name__ == "__main__":
    main()
