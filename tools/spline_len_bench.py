#!/usr/bin/env python3
"""Times of the two spline-length regularisers on the GPU (csrc/spline_len.hip), written to profiles/spline_len/bench.json.

    python tools/spline_len_bench.py [--reps 9] [--inner 20] [--out profiles/spline_len]

The method is tools/voxel_bench.py's (device events around `inner` back-to-back calls, every shape warmed up, the sides of a
comparison alternated inside one repetition, the median of `reps` repetitions with min .. max).  Shape: the `make dyn_voxel` crop,
2 views x 44 x 44 rays x 80 steps = 309 760 samples, S = 64, spline 4, rays from the project's ray generator; the random-voxel term at
its 16^3 indices.  Every row is value + gradient (the value's launch, the upstream scalar, the gradient's launch, allocating and
zeroing the gradient tensor), which is what an iteration of training pays.

"torch" rows are the BASELINE: a plain-PyTorch restatement of the reference's arc_len (every control point of every sample as a
tensor, 16 de Casteljau evaluations, autograd's backward), written for this tool and run on the same GPU in fp32 -- never a kernel of
this project.
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


def torch_arc_len(cp, t):
    """cp [n, N, 3], t [16] -> [N]: de Casteljau at every t, the norms of the 15 differences, their sum"""
    b = cp[:, :, None, :]
    tt = t[None, None, :, None]
    for _ in range(1, cp.shape[0]):
        b = b[:-1] * (1 - tt) + b[1:] * tt
    p = b[0]
    return torch.linalg.vector_norm(p[:, 1:] - p[:, :-1], dim=-1).sum(dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spline_len"))
    ap.add_argument("--tag", default="bench")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_ref as V
    import spline_len_ref as R
    from nerf_atlas_amd import config, nerf, ops
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    S, T, n, gr, K = 64, 80, 4, 1.3, 16 ** 3
    ctrl = (R.ctrl_grid(S, n) * 0.3).to(dev)
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(2)])).float().to(dev)
    rays = ops.raygen(c2w, 0.5 * 64 / math.tan(0.5 * FOV_X), 64, (10, 10, 44, 44))
    ts = torch.linspace(2.0, 6.0, T, device=dev)
    pts = ops.compute_pts(rays, ts)                                   # [T,2,44,44,3]
    N = pts.numel() // 3
    w = torch.from_numpy(V.proc_uniform((N,), 6001, 0.5) + 0.5).to(dev).reshape(pts.shape[:-1]).contiguous()
    table = torch.linspace(0, 1, 16).to(dev)
    one = torch.ones(1, device=dev)
    shape = f"N={N} S={S} spline={n}"
    grid_bytes = 4 * 3 * (n - 1) * S ** 3
    lerps = 16 * 3 * (n * (n - 1) // 2)
    rows = []

    # ---- the per-sample term
    def hip_sample():
        ops.dyn_voxel_spline_len(pts, ctrl, n, gr, w)
        ops.dyn_voxel_spline_len_backward(pts, ctrl, n, gr, one, w)
    cr = ctrl.clone().requires_grad_(True)

    def torch_sample():
        cr.grad = None
        cp = torch_lookup(pts, cr, gr).reshape(N, n - 1, 3).movedim(1, 0)
        cp = torch.cat([torch.zeros_like(cp[:1]), cp], dim=0)
        (w.reshape(N) * torch_arc_len(cp, table)).mean().backward()
    # the two sides compute the same numbers: the project's 1e-4 bar on value and gradient before anything is timed
    v_hip, g_hip = ops.dyn_voxel_spline_len(pts, ctrl, n, gr, w), ops.dyn_voxel_spline_len_backward(pts, ctrl, n, gr, one, w)
    torch_sample()
    cp = torch_lookup(pts, ctrl, gr).reshape(N, n - 1, 3).movedim(1, 0)
    v_torch = (w.reshape(N) * torch_arc_len(torch.cat([torch.zeros_like(cp[:1]), cp], dim=0), table)).mean()
    dev_v, dev_g = float((v_hip - v_torch).abs()), float((g_hip - cr.grad).abs().max() / cr.grad.abs().max())
    print(f"per-sample term: value {float(v_hip):.7f} (torch {float(v_torch):.7f}), gradient off by {dev_g:.2e} of the largest entry")
    assert dev_v <= 1e-4 * max(1.0, abs(float(v_torch))) and dev_g <= 1e-4
    t = timed({"hip": hip_sample, "torch": torch_sample}, a.reps, max(1, a.inner // 4))
    note = f"{lerps} lerps per sample and pass; bytes = positions, weights and the grid once per launch + the gradient tensor"
    rows.append(row("--spline-len-decay term, value + gradient", t["hip"], shape, 2 * (N * 16 + grid_bytes) + 2 * grid_bytes, note=note))
    rows.append(row("torch restatement, value + gradient", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))
    t = timed({"value": lambda: ops.dyn_voxel_spline_len(pts, ctrl, n, gr, w),
               "gradient": lambda: ops.dyn_voxel_spline_len_backward(pts, ctrl, n, gr, one, w)}, a.reps, a.inner)
    rows.append(row("dyn_voxel_spline_len (one launch)", t["value"], shape, N * 16 + grid_bytes))
    rows.append(row("dyn_voxel_spline_len_backward, fp32 atomics", t["gradient"], shape, N * 16 + 3 * grid_bytes,
                    atomic_bytes=N * 8 * 3 * (n - 1) * 4, note="added bytes = every contribution on its own; the time includes zeroing the gradient tensor"))
    config.set_deterministic(True)
    try:
        t = timed({"fixed": hip_sample}, a.reps, max(1, a.inner // 4))
    finally:
        config.set_deterministic(False)
    rows.append(row("--spline-len-decay term, 2^-40 fixed point", t["fixed"], shape))

    # ---- the random-voxel term and its draw
    shape_g = f"K={K} S={S} spline={n}"
    cg = ctrl.clone().requires_grad_(True)

    def hip_grid():
        cg.grad = None
        nerf.arc_len_grid(cg).backward()

    def torch_grid():
        cr.grad = None
        idxs = nerf.random_sample_grid(cr, K)
        x, y, z = idxs % S, idxs // S % S, idxs // (S * S) % S
        data = torch.stack(cr[x, y, z].split(3, dim=-1), dim=0)
        torch_arc_len(data, table).mean().backward()
    idxs = nerf.random_sample_grid(ctrl, K)
    x, y, z = idxs % S, idxs // S % S, idxs // (S * S) % S
    v_hip = nerf.arc_len_grid(ctrl, idxs=idxs)
    v_torch = torch_arc_len(torch.stack(ctrl[x, y, z].split(3, dim=-1), dim=0), table).mean()
    print(f"random-voxel term: value {float(v_hip):.7f} (torch {float(v_torch):.7f})")
    assert float((v_hip - v_torch).abs()) <= 1e-4 * max(1.0, abs(float(v_torch)))
    t = timed({"hip": hip_grid, "torch": torch_grid}, a.reps, a.inner)
    rows.append(row("--voxel-random-spline-len-decay term, draw + value + gradient", t["hip"], shape_g,
                    note="through autograd: the draw, its decode to rows, two launches, zeroing the [S,S,S,9] gradient tensor"))
    rows.append(row("torch restatement, draw + value + gradient", t["torch"], shape_g, note="plain-torch restatement written for this tool (the baseline)"))
    rws = R.rows_of_flat(idxs, (S, S, S))
    t = timed({"draw": lambda: nerf.random_sample_grid(ctrl, K), "value": lambda: ops.grid_spline_len(ctrl, rws, True),
               "gradient": lambda: ops.grid_spline_len_backward(ctrl, rws, one, True)}, a.reps, a.inner)
    rows.append(row("the 16^3 draw (utils.randint)", t["draw"], shape_g))
    rows.append(row("grid_spline_len (one launch)", t["value"], shape_g, K * (8 + 12 * (n - 1))))
    rows.append(row("grid_spline_len_backward, fp32 atomics", t["gradient"], shape_g, K * (8 + 24 * (n - 1)) + grid_bytes,
                    note="the time includes zeroing the gradient tensor, which is most of it"))
    finish(a, rows)


if __name__ == "__main__":
    main()
