#!/usr/bin/env python3
"""Times of --dyn-model voxel on the GPU (csrc/dyn_voxel.hip, na_voxel_sample_backward_pts), written to profiles/dyn_voxel/bench.json.

    python tools/dyn_voxel_bench.py [--reps 9] [--inner 20] [--out profiles/dyn_voxel]

The method is tools/voxel_bench.py's (device events around `inner` back-to-back calls, every shape warmed up, the sides of a
comparison alternated inside one repetition, the median of `reps` repetitions with min .. max).  Shape: the `make dyn_voxel` crop,
2 views x 44 x 44 rays x 80 steps = 309 760 samples, S = 64, spline 4, rays from the project's ray generator, two frame times.

"torch" rows are the BASELINE: a plain-PyTorch restatement of the reference's forward (advanced indexing, the spline, the sigmoid)
and autograd's backward of it, written for this tool and run on the same GPU in fp32 -- never a kernel of this project.

For the scatter: the added bytes over the time against the 1.3 TB/s chip-wide rate of global float atomics, once counting every
contribution as if it went to memory on its own and once counting what reaches memory when every grid row of a workgroup's run finds a
slot in the LDS table (distinct rows per workgroup x row width; computed on the host from the cells -- probe failures, which send a
contribution past the table, are not counted, so the absorbed share printed is an upper bound).
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


def torch_cells(pts, S, grid_radius):
    step = grid_radius * 2 / S
    last = grid_radius - step / 2

    def centre(n):
        return ((torch.floor(n.clamp(-grid_radius, grid_radius) / step + 1e-10) + 0.5) * step).clamp(-last, last)
    lo, hi = centre(pts - 0.5 * step), centre(pts + 0.5 * step)
    frac = (pts - lo) / step
    index = lambda c: (torch.floor(c / step + 1e-10) + S / 2).long().clamp(0, S - 1)
    return (index(lo), index(hi)), (1 - frac, frac)


def torch_lookup(pts, grid, grid_radius):
    """the 8-neighbour lookup of a channel-last grid in plain torch; [..., C]"""
    idx, wgt = torch_cells(pts, grid.shape[0], grid_radius)
    out = 0
    for u in range(8):
        b = [(u >> i) & 1 for i in range(3)]
        w = wgt[b[0]][..., 0] * wgt[b[1]][..., 1] * wgt[b[2]][..., 2]
        out = out + w[..., None] * grid[idx[b[0]][..., 0], idx[b[1]][..., 1], idx[b[2]][..., 2]]
    return out


def torch_warp(pts, t, ctrl, rig, n, grid_radius):
    """src/nerf.py:1571-1586 in plain torch: (warped, dp, rigidity)"""
    cp = torch_lookup(pts, ctrl, grid_radius).split(3, dim=-1)
    cp = torch.stack([torch.zeros_like(cp[0])] + list(cp), dim=0)
    tt = t[..., None]
    if n == 4:
        m1t = 1 - tt
        k = torch.stack([m1t * m1t * m1t, 3 * m1t * m1t * tt, 3 * tt * tt * m1t, tt * tt * tt], dim=0)
        dp = (k * cp).sum(dim=0)
    else:
        for _ in range(1, n):
            cp = cp[:-1] * (1 - tt) + cp[1:] * tt
        dp = cp.squeeze(0)
    r = torch_lookup(pts, rig, grid_radius).sigmoid()
    return pts + dp * r, dp, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn_voxel"))
    ap.add_argument("--tag", default="bench")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_ref as V
    import dyn_voxel_ref as D
    from nerf_atlas_amd import config, nerf, ops, refl, train
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    S, T, n, gr = 64, 80, 4, 1.3
    CH, W = 3 * (n - 1), 3 * (n - 1) + 1
    den, rgb = (x.to(dev) for x in V.grid_values(S))
    ctrl, rig = (x.to(dev) for x in D.dyn_grids(S, n))
    ctrl = ctrl * 0.3
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(2)])).float().to(dev)
    rays = ops.raygen(c2w, 0.5 * 64 / math.tan(0.5 * FOV_X), 64, (10, 10, 44, 44))
    assert rays.shape == (2, 44, 44, 6)
    ts = torch.linspace(2.0, 6.0, T, device=dev)
    pts = ops.compute_pts(rays, ts)                                   # [T,2,44,44,3]
    N = pts.numel() // 3
    tt = torch.tensor([0.25, 0.8], device=dev)[None, :, None, None].expand(pts.shape[:-1]).contiguous()
    shape = f"N={N} S={S} spline={n}"
    grids_bytes = 4 * W * S ** 3
    rows = []

    # ---- the deformation
    t = timed({"hip": lambda: ops.dyn_voxel_warp(pts, tt, ctrl, rig, n, gr),
               "torch": lambda: torch_warp(pts, tt, ctrl, rig, n, gr)}, a.reps, a.inner)
    rows.append(row("dyn_voxel_warp (one launch)", t["hip"], shape, N * (12 + 4 + 12 + 12 + 4) + grids_bytes))
    rows.append(row("torch warp, forward", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))

    # ---- its backward
    warped, dp, r = ops.dyn_voxel_warp(pts, tt, ctrl, rig, n, gr)
    g_w, g_dp, g_r = (torch.from_numpy(V.proc_uniform(s, seed, 1.0)).to(dev) for s, seed in (((N, 3), 5101), ((N, 3), 5102), ((N,), 5103)))
    cr, rr = ctrl.clone().requires_grad_(True), rig.clone().requires_grad_(True)

    def torch_fwd_bwd():
        cr.grad = rr.grad = None
        w_, dp_, r_ = torch_warp(pts, tt, cr, rr, n, gr)
        torch.autograd.backward([w_, dp_, r_], [g_w.reshape(w_.shape), g_dp.reshape(dp_.shape), g_r.reshape(r_.shape)])

    def scatter():
        ops.dyn_voxel_warp_backward(pts, tt, dp, r, S, n, gr, g_w, g_dp, g_r)
    # what reaches memory if every row of a workgroup's run finds a slot: distinct rows per workgroup
    ids, _ = V.cells(pts.reshape(-1, 3).cpu(), S, gr)
    rws = V.rows_of(ids, S)                                           # [N,8]
    wgs = min(4096, (N + 255) // 256)
    per = ((N + wgs - 1) // wgs + 255) // 256 * 256
    distinct = sum(int(torch.unique(rws[i:i + per]).numel()) for i in range(0, N, per))
    every, flushed = N * 8 * W * 4, distinct * W * 4
    absorbed = 1 - distinct / (N * 8)
    print(f"contributions {N * 8}, distinct rows per workgroup summed {distinct}: the table absorbs at most {absorbed:.1%}")
    t = timed({"atomics": scatter}, a.reps, a.inner)
    note = (f"added bytes = every contribution on its own; with every row in a slot {flushed} bytes reach memory "
            f"({flushed / (statistics_median(t['atomics']) * 1e-3) / 1e12:.3f} TB/s), the table absorbs at most {absorbed:.3f} of the contributions.  "
            "The time includes allocating and zeroing the two gradient tensors")
    rows.append(row("dyn_voxel_warp_backward, fp32 atomics", t["atomics"], shape, N * 60 + 2 * grids_bytes, atomic_bytes=every, note=note))
    config.set_deterministic(True)
    try:
        t = timed({"fixed": scatter}, a.reps, a.inner)
    finally:
        config.set_deterministic(False)
    rows.append(row("dyn_voxel_warp_backward, 2^-40 fixed point", t["fixed"], shape, N * 60 + 2 * grids_bytes + 2 * 8 * W * S ** 3,
                    atomic_bytes=2 * every))
    t = timed({"torch": torch_fwd_bwd}, a.reps, max(1, a.inner // 4))
    rows.append(row("torch warp, forward + backward", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))

    # ---- the position gradient of the canonical lookup
    g_raw = torch.from_numpy(V.proc_uniform((N, 4), 5104, 1.0)).to(dev)
    wp = warped.clone().requires_grad_(True)
    grid4 = torch.cat([den, rgb], dim=-1)

    def torch_pts_grad():
        wp.grad = None
        torch_lookup(wp, grid4, gr).backward(g_raw.reshape(wp.shape[:-1] + (4,)))
    t = timed({"hip": lambda: ops.voxel_sample_backward_pts(g_raw, warped, den, rgb, gr), "torch": torch_pts_grad}, a.reps, max(1, a.inner // 2))
    rows.append(row("voxel_sample_backward_pts (gather)", t["hip"], shape, N * (12 + 16 + 12) + 16 * S ** 3))
    rows.append(row("torch lookup, forward + position gradient", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))

    # ---- the whole model: forward + backward (+ one-launch Adam)
    c = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    c.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    m = nerf.DynamicNeRFVoxel(c, spline=n).to(dev).train()
    opt = train.NaAdam(m.parameters(), lr=1e-2)
    target = torch.full(tuple(rays.shape[:-1]) + (3,), 0.5, device=dev)
    times = torch.tensor([0.25, 0.8], device=dev)

    def fwd_bwd():
        opt.zero_grad()
        (m((rays, times)) - target).square().mean().backward()

    def step():
        fwd_bwd()
        opt.step()
    dt, rt, ct, gt = (x.detach().clone().requires_grad_(True) for x in (c.densities, c.rgb, m.ctrl_pts_grid, m.rigidity_grid))
    dists = torch.cat([ts[1:] - ts[:-1], torch.full((1,), 1e10, device=dev)])[:, None, None, None] * rays[..., 3:].norm(dim=-1)[None]

    def torch_model():
        for p_ in (dt, rt, ct, gt):
            p_.grad = None
        w_, _, _ = torch_warp(pts, tt, ct, gt, n, gr)
        raw = torch_lookup(w_, torch.cat([dt, rt], dim=-1), gr)
        alpha = 1 - torch.exp(-torch.nn.functional.softplus(raw[..., 0] - 1) * dists)
        trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:1]), 1 - alpha[:-1] + 1e-10], dim=0), dim=0)
        out = ((alpha * trans)[..., None] * (torch.sigmoid(raw[..., 1:]) * 1.002 - 0.001)).sum(dim=0)
        (out - target).square().mean().backward()
    t = timed({"hip": fwd_bwd, "torch": torch_model}, a.reps, max(1, a.inner // 4))
    rows.append(row("DynamicNeRFVoxel forward + backward", t["hip"], shape))
    rows.append(row("torch model, forward + backward", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))
    t = timed({"step": step}, a.reps, max(1, a.inner // 4))
    rows.append(row("training step (fwd, l2, bwd, Adam)", t["step"], shape))
    m.eval()
    with torch.no_grad():
        t = timed({"eval": lambda: m((rays, times))}, a.reps, a.inner)
    rows.append(row("eval route (warp + render)", t["eval"], shape))
    finish(a, rows)


def statistics_median(v):
    import statistics
    return statistics.median(v)


if __name__ == "__main__":
    main()
