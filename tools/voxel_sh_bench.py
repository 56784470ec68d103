#!/usr/bin/env python3
"""Times of the spherical-harmonic voxel head on the GPU (csrc/voxel.hip, na_dyn_voxel_sh_render), written to
profiles/voxel_sh/bench.json.

    python tools/voxel_sh_bench.py [--reps 9] [--inner 20] [--out profiles/voxel_sh]

The method is tools/voxel_bench.py's (device events around `inner` back-to-back calls, every shape warmed up, the sides of a
comparison alternated inside one repetition, the median of `reps` repetitions with min .. max).  Shape: tools/voxel_plv_bench.py's crop
of `make dyn_voxel`, 2 views x 44 x 44 rays x 80 steps = 309 760 samples, S = 64, order 4 (C = 75), spline 4; and the 64 x 64 x 80 test
tile with all maps.

"torch" rows are what a user would otherwise run: a plain-PyTorch restatement of the head (advanced indexing of [N, 76] per corner, the
[N, 3, 25] coefficients times eval_sh restated from its closed forms, autograd), written for this tool and run on the same GPU in fp32
-- never a kernel of this project.  Both scatter geometries (csrc/voxel_plv.h: 1 whole rows in the LDS table, 2 a pass per colour
channel) are timed in both accumulation modes; the pos-linear-view head's lookup and scatter (C = 28) stand next to them for scale.
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
from tools.dyn_voxel_bench import torch_lookup  # noqa: E402
from tools.voxel_plv_bench import torch_sh4  # noqa: E402


def torch_contract(co, view):
    """co [..., 75] interpolated coefficients, view [..., 3] -> s [..., 3]"""
    Y = torch_sh4(torch.nn.functional.normalize(view, dim=-1))
    return (co.reshape(co.shape[:-1] + (3, 25)) * Y[..., None, :]).sum(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_sh"))
    ap.add_argument("--tag", default="bench")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_plv_ref as P
    import voxel_sh_ref as H
    import voxel_ref as V
    import dyn_voxel_ref as D
    from nerf_atlas_amd import config, nerf, ops, refl
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    S, T, K, n, gr = 64, 80, 4, 4, 1.3
    C = 3 * (K + 1) ** 2
    den, rgb = (x.to(dev) for x in H.grid_values(S, K))
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
    grid76 = torch.cat([den, rgb], dim=-1)
    pden, prgb = (x.to(dev) for x in P.grid_values(S, K))
    g_raw = torch.from_numpy(V.proc_uniform((N, 4), 5201, 1.0)).to(dev)
    g_sh = torch.from_numpy(V.proc_uniform((N,), 5202, 1.0)).to(dev)

    # ---- the lookup
    def torch_lookup_head():
        raw = torch_lookup(pts, grid76, gr)
        return torch.cat([raw[..., :1], torch_contract(raw[..., 1:], view)], dim=-1)
    t = timed({"hip": lambda: ops.voxel_sh_sample(den, rgb, K, gr, rays, pts=pts), "torch": torch_lookup_head,
               "plv": lambda: ops.voxel_plv_sample(pden, prgb, gr, rays, pts=pts)}, a.reps, a.inner)
    rows.append(row("voxel_sh_sample (one launch)", t["hip"], shape, N * (12 + 16) + grid_bytes,
                    note="the gather is 8 rows of 300 B per sample (743 MB of row reads served by the caches: the grid is 80 MB)"))
    rows.append(row("torch lookup [N,76] + eval_sh", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))
    rows.append(row("voxel_plv_sample, C = 28 (for scale)", t["plv"], shape))

    # ---- the scatter: both geometries, both modes, next to the pos-linear-view head's shipped scatter
    every = N * 8 * (1 + C) * 4
    for det in (False, True):
        if det:
            config.set_deterministic(True)
        try:
            sides = {v: (lambda v=v: ops.voxel_sh_sample_backward(g_raw, S, K, gr, rays, pts=pts, variant=v)) for v in (1, 2)}
            sides["plv"] = lambda: ops.voxel_plv_sample_backward(g_raw, g_sh, S, K, gr, rays, pts=pts)
            t = timed(sides, a.reps, max(1, a.inner // 2))
        finally:
            if det:
                config.set_deterministic(False)
        mode = "2^-40 fixed point" if det else "fp32 atomics"
        for v, what in ((1, "whole rows in the LDS table"), (2, "a pass per colour channel, [density | one block] in the table")):
            rows.append(row(f"voxel_sh_sample_backward variant {v}, {mode}", t[v], shape, atomic_bytes=every * (2 if det else 1),
                            note=what + "; added bytes count every contribution as if it reached memory (the table's job is that most do "
                            "not); the time includes allocating and zeroing the two gradient tensors"
                            + (" and zeroing and folding the 159 MB fixed-point workspace" if det else "")))
        rows.append(row(f"voxel_plv_sample_backward, C = 28, {mode} (for scale)", t["plv"], shape))

    def torch_scatter():
        g = grid76.detach().clone().requires_grad_(True)
        raw = torch_lookup(pts, g, gr)
        out = torch.cat([raw[..., :1], torch_contract(raw[..., 1:], view)], dim=-1)
        out.backward(g_raw.reshape(out.shape))
        return g.grad
    t = timed({"torch": torch_scatter}, a.reps, max(1, a.inner // 4))
    rows.append(row("torch lookup + eval_sh, forward + grid gradient", t["torch"], shape,
                    note="plain-torch restatement written for this tool (the baseline of the scatter: autograd's index_put)"))

    # ---- the position gradient
    wp = pts.clone().requires_grad_(True)

    def torch_pts_grad():
        wp.grad = None
        raw = torch_lookup(wp, grid76, gr)
        out = torch.cat([raw[..., :1], torch_contract(raw[..., 1:], view)], dim=-1)
        out.backward(g_raw.reshape(out.shape))
    t = timed({"hip": lambda: ops.voxel_sh_sample_backward_pts(g_raw, pts, rays, den, rgb, K, gr), "torch": torch_pts_grad}, a.reps,
              max(1, a.inner // 2))
    rows.append(row("voxel_sh_sample_backward_pts (gather)", t["hip"], shape, N * (12 + 16 + 12) + grid_bytes))
    rows.append(row("torch lookup + eval_sh, forward + position gradient", t["torch"], shape,
                    note="plain-torch restatement written for this tool (the baseline)"))

    # ---- the static model: forward + backward
    c = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    c.set_refl(refl.SphericalHarmonic(act="upshifted", latent_size=0, out_features=3, voxel_order=K))
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
        out = ((alpha * trans)[..., None] * (torch_contract(raw[..., 1:], view).sigmoid() + 1e-2)).sum(dim=0)
        (out - target).square().mean().backward()
    t = timed({"hip": fwd_bwd, "torch": torch_model}, a.reps, max(1, a.inner // 4))
    rows.append(row("NeRFVoxel + sph-har, forward + backward", t["hip"], shape,
                    note="stratified steps drawn per call (training mode); fp32 atomics"))
    rows.append(row("torch model, forward + backward", t["torch"], shape,
                    note="plain-torch restatement written for this tool: what a user would otherwise run"))
    c.eval()
    with torch.no_grad():
        t = timed({"eval": lambda: c(rays)}, a.reps, a.inner)
    rows.append(row("eval route (voxel_sh_render, one launch)", t["eval"], shape))

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
        out, alpha, weights = ops.voxel_sh_render(tile, ts, den, rgb, K, gr, "upshifted", "black", True, pts=w)
        return (out, ops.integrate(weights, ts[:, None, None].expand(T, R, 1).contiguous()), ops.integrate(weights, ones),
                ops.integrate(weights, (dp * r[..., None]).contiguous()), ops.integrate(weights, r[..., None].contiguous()))
    render = lambda: ops.dyn_voxel_render(tile, tt, ts, den, rgb, ctrl, rig, n, gr, "upshifted", "black", want=want, sh_order=K)
    one, ref = render(), composition()
    assert all(torch.equal(a_, b_) for a_, b_ in zip((one["rgb"], one["depth"], one["acc"], one["flow"], one["rigidity"]), ref))
    t = timed({"one": render, "composition": composition}, a.reps, a.inner)
    tshape = f"R={R} T={T} S={S} K={K} spline={n}"
    rows.append(row("dyn_voxel_sh_render, all maps (one launch)", t["one"], tshape))
    rows.append(row("composition: pts, warp, voxel_sh_render, integrate x 4", t["composition"], tshape,
                    note="this project's own launches; bit for bit the same result (checked here before timing)"))
    finish(a, rows)


if __name__ == "__main__":
    main()
