#!/usr/bin/env python3
"""Times of the grid operators on the GPU (csrc/grid_ops.hip), written to profiles/voxel/grid_bench.json.

    python tools/grid_bench.py [--reps 9] [--inner 20] [--parent PATH] [--out profiles/voxel]

The method of tools/voxel_bench.py (its `timed` and `row`): device events around `inner` back-to-back calls, every shape warmed up
first, the sides of a comparison alternated inside one repetition, the median of `reps` repetitions with the spread next to it.
  * total variation, value + gradient, 32 768 samples at 64^3 x 1, 64^3 x 3 and 128^3 x 28, against the same arithmetic as torch
    operators on the device (advanced indexing + autograd: what a user would otherwise run -- written for this tool);
  * upsample 64 -> 128 and 128 -> 256 (3 channels), against F.interpolate on the device;
  * one `make voxel`-shaped training step (tools/voxel_bench.py's) without and with both TV terms.  --parent PATH: a built checkout of
    the parent commit; its step is timed by a child process of this one on the same device, alternating with a child that times
    this checkout's step, and the two must agree (the step without the terms runs no new code).
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_tv(grid, idxs):
    s0, s1, s2, _ = grid.shape
    x, y, z = idxs % s0, (idxs // s0) % s1, (idxs // (s0 * s1)) % s2
    adj = lambda v, s: torch.where(v == s - 1, v - 1, v + 1)
    e = grid[x, y, z]
    dx, dy, dz = e - grid[adj(x, s0), y, z], e - grid[x, adj(y, s1), z], e - grid[x, y, adj(z, s2)]
    return (dx.square() + dy.square() + dz.square()).clamp(min=1e-10).sqrt().mean()


def step_setup(root, tv):
    """the training step of tools/voxel_bench.py on the package under `root`; tv: add both total-variation terms"""
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from nerf_atlas_amd import nerf, ops, refl, train
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    S, T = 64, 64
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(10)])).float().to(dev)
    rays = ops.raygen(c2w, 0.5 * 64 / math.tan(0.5 * FOV_X), 64, (12, 12, 40, 40))
    torch.manual_seed(0)
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    m.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    m = m.to(dev).train()
    opt = train.NaAdam(m.parameters(), lr=1e-2)
    target = torch.full(tuple(rays.shape[:-1]) + (3,), 0.5, device=dev)

    def step():
        opt.zero_grad()
        loss = (m(rays) - target).square().mean()
        if tv:
            loss = loss + 1e-3 * nerf.total_variation(m.densities) + 1e-4 * nerf.total_variation(m.rgb)
        loss.backward()
        opt.step()
    return step


def child(root, reps, inner):
    """one process, one package: the step without the terms; prints the per-call times as a json line"""
    sys.path.insert(0, REPO)
    from tools.voxel_bench import timed
    print(json.dumps(timed({"step": step_setup(root, False)}, reps, inner)["step"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    if a.child:
        return child(a.child, a.reps, a.inner)
    sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
    import torch.nn.functional as F
    from oracle.procedural import proc_uniform
    from nerf_atlas_amd import ops
    from tools.voxel_bench import row, timed
    dev = torch.device("cuda")
    rows = []
    n = 32 ** 3
    for S, C in ((64, 1), (64, 3), (128, 28)):
        grid = torch.from_numpy(proc_uniform((S, S, S, C), 5600 + C, 1.0)).to(dev)
        idxs = torch.randint(0, S ** 3, (n,), device=dev)
        one = torch.ones((), device=dev)
        leaf = grid.clone().requires_grad_(True)

        def hip():
            ops.grid_tv(grid, idxs, trusted=True)
            ops.grid_tv_backward(grid, idxs, one, trusted=True)

        def plain():
            leaf.grad = None
            torch_tv(leaf, idxs).backward()
        t = timed({"hip": hip, "torch": plain}, a.reps, a.inner)
        shape = f"{S}^3 x {C}, {n} samples"
        touched = n * 4 * C * 4 * 3 + n * 8 * 2 + grid.numel() * 4   # 4 rows read twice and added to once, the indices twice, the zeroed gradient
        rows.append(row("grid_tv + grid_tv_backward", t["hip"], shape, touched, note="two launches + allocating and zeroing the gradient"))
        rows.append(row("torch operators, forward + backward", t["torch"], shape, note="plain-torch restatement written for this tool"))
    for S, R in ((64, 128), (128, 256)):
        grid = torch.from_numpy(proc_uniform((S, S, S, 3), 5610 + S, 1.0)).to(dev)
        ncdhw = grid.permute(3, 0, 1, 2)[None]
        t = timed({"hip": lambda: ops.grid_upsample(grid, R),
                   "torch": lambda: F.interpolate(ncdhw, size=R, mode="trilinear").squeeze(0).permute(1, 2, 3, 0).contiguous()},
                  a.reps, max(1, a.inner // 2))
        shape = f"{S} -> {R}, 3 channels"
        rows.append(row("grid_upsample", t["hip"], shape, (S ** 3 + R ** 3) * 12))
        rows.append(row("F.interpolate + back to channel-last", t["torch"], shape, (S ** 3 + R ** 3) * 12, note="what upsample_grid (src/nerf.py:377-379) runs"))
    t = timed({"plain": step_setup(REPO, False), "tv": step_setup(REPO, True)}, a.reps, a.inner)
    rows.append(row("training step without the TV terms", t["plain"], "N=1024000 S=64"))
    rows.append(row("training step with both TV terms", t["tv"], "N=1024000 S=64", note="+ 2 x (randint, grid_tv, grid_tv_backward) and two scalar nodes"))
    if a.parent:
        sides = {"this checkout": REPO, "parent commit": os.path.abspath(a.parent)}
        got = {k: [] for k in sides}
        for _ in range(2):   # the two packages alternate, each in a fresh process
            for k, root in sides.items():
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--reps", str(a.reps), "--inner", str(a.inner)],
                                     capture_output=True, text=True, timeout=300, check=True).stdout
                got[k] += json.loads(out.strip().splitlines()[-1])
        for k in sides:
            rows.append(row(f"training step without the TV terms, {k} (child process)", got[k], "N=1024000 S=64"))
        ratio = statistics.median(got["this checkout"]) / statistics.median(got["parent commit"])
        print(f"step without the terms: this checkout / parent commit = {ratio:.4f}")
        rows.append(dict(name="this checkout / parent commit, medians", ratio=ratio))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "grid_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, inner=a.inner, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
