#!/usr/bin/env python3
"""Times of the two divergence regularisers of --dyn-model voxel on the GPU (csrc/dyn_voxel_div.hip), written to
profiles/dyn_voxel_div/bench.json.

    python tools/dyn_voxel_div_bench.py [--reps 9] [--inner 20] [--out profiles/dyn_voxel_div]

The method is tools/voxel_bench.py's (device events around `inner` back-to-back calls, every shape warmed up, the sides of a
comparison alternated inside one repetition, the median of `reps` repetitions with min .. max).  Shape: the `make dyn_voxel` crop,
2 views x 44 x 44 rays x 80 steps = 309 760 samples, S = 64, spline 4, rays from the project's ray generator.

Each new launch is set against two yardsticks on the same inputs: na_dyn_voxel_warp, which reads the same eight rows per sample, and a
plain-PyTorch double-autograd restatement of the lookup ("torch" rows: the only other route to the Jacobian, written for this tool and
run on the same GPU in fp32 -- never a kernel of this project).  The last rows are a training iteration of the recipe (its argv on the
analytic dynamic scene at 64 x 64, crop 44, 80 steps, batch 2) without the flags and with each: host clock around `iters` iterations
that end in a device synchronise.
"""
import argparse
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from tools.voxel_bench import finish, row, timed  # noqa: E402
from tools.dyn_voxel_bench import torch_warp  # noqa: E402

RECIPE = ["--data-kind", "dnerf", "--size", "64", "--near", "2", "--far", "6", "--batch-size", "2", "--crop-size", "44", "--model", "voxel",
          "--dyn-model", "voxel", "-lr", "1e-2", "--loss-fns", "l2", "--spline", "4", "--steps", "80", "--voxel-tv-sigma", "1e-3",
          "--voxel-tv-rgb", "1e-4", "--voxel-tv-bezier", "1e-4", "--voxel-tv-rigidity", "1e-4", "--higher-end-chance", "1", "--offset-decay",
          "30", "--sigmoid-kind", "upshifted", "--voxel-random-spline-len-decay", "1e-5", "--seed", "1337", "--refl-kind", "pos-linear-view",
          "--voxel-refl-order", "4", "--quiet"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--iters", type=int, default=10, help="training iterations per timed window")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn_voxel_div"))
    ap.add_argument("--tag", default="bench")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_ref as V
    import dyn_voxel_ref as DV
    import dyn_voxel_div_ref as R
    from nerf_atlas_amd import config, loaders, ops
    import nerf_atlas_amd.train as T
    from tools.make_scene import FOV_X, look_at_origin, make_scene
    dev = torch.device("cuda")
    S, steps, n, gr = 64, 80, 4, 1.3
    ctrl, rig = DV.dyn_grids(S, n)
    ctrl, rig = (ctrl * 0.3).to(dev), rig.to(dev)
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(2)])).float().to(dev)
    rays = ops.raygen(c2w, 0.5 * 64 / math.tan(0.5 * FOV_X), 64, (10, 10, 44, 44))
    pts = ops.compute_pts(rays, torch.linspace(2.0, 6.0, steps, device=dev))                  # [T,2,44,44,3]
    N = pts.numel() // 3
    tt = torch.tensor([0.25, 0.8], device=dev)[None, :, None, None].expand(pts.shape[:-1]).contiguous()
    e = torch.from_numpy(V.proc_uniform((N, 3), 6101, 1.0)).to(dev).reshape(pts.shape).contiguous()
    g = torch.full(pts.shape[:-1], 1.0 / N, device=dev)
    shape = f"N={N} S={S} spline={n}"
    row_bytes = 4 * 3 * (n - 1)
    grid_bytes = row_bytes * S ** 3
    rows = []

    # ---- the restatement computes the same numbers: the project's 1e-4 bar, relative to the largest value, before anything is timed
    def torch_ffjord():
        p = pts.clone().requires_grad_(True)
        _, dp, r = torch_warp(p, tt, ctrl, rig, n, gr)
        ge, = torch.autograd.grad(dp * r, p, grad_outputs=e)
        return (ge * e).sum(dim=-1)
    cr = ctrl.clone().requires_grad_(True)

    def torch_divergence():
        cr.grad = None
        p = pts.clone().requires_grad_(True)
        _, dp, _ = torch_warp(p, tt, cr, rig, n, gr)
        gp, = torch.autograd.grad(dp, p, grad_outputs=torch.ones_like(dp), create_graph=True)
        div = gp.sum(dim=-1)
        div.mean().backward()
        return div.detach()

    def hip_divergence():
        ops.dyn_voxel_jac_quad(pts, tt, ctrl, None, n, gr)
        ops.dyn_voxel_jac_quad_backward(pts, tt, S, n, gr, g)
    for name, hip, ref in (("e . J_rigid e", ops.dyn_voxel_jac_quad(pts, tt, ctrl, rig, n, gr, e), torch_ffjord()),
                           ("1 . J_dp 1", ops.dyn_voxel_jac_quad(pts, tt, ctrl, None, n, gr), torch_divergence())):
        off = float((hip - ref).abs().max() / ref.abs().max())
        print(f"{name}: off the torch restatement by {off:.2e} of the largest value ({float(ref.abs().max()):.3g})")
        assert off <= 1e-4
    # the gradient sums up to thousands of fp32 addends per entry on either side, each in its own order: the kernel is held to the fp64
    # restatement's derived bound (tests/dyn_voxel_div_ref.py) at this very shape; the fp32 torch side's distance is printed next to it
    g_hip = ops.dyn_voxel_jac_quad_backward(pts, tt, S, n, gr, g)
    ref, mag, cnt, _ = R.jac_quad_backward_ref(pts.reshape(-1, 3).cpu(), tt.reshape(-1).cpu(), S, n, g.reshape(-1).cpu(), gr)
    ratio = V.worst_ratio(g_hip.reshape(ref.shape), ref, R.scatter_bound(ref, mag, cnt, n, False))
    scale = float(ref.abs().max())
    off_hip, off_torch = (float((x.detach().cpu().double().reshape(ref.shape) - ref).abs().max()) / scale for x in (g_hip, cr.grad))
    print(f"d mean(1 . J_dp 1) / d ctrl_pts_grid against the fp64 restatement: kernel {off_hip:.2e} of the largest entry (worst |err| / bound "
          f"{ratio:.3f}, up to {int(cnt.max())} addends per entry), fp32 torch restatement {off_torch:.2e}")
    assert ratio <= 1.0 and off_torch <= 1e-3

    # ---- the launches against na_dyn_voxel_warp on the same inputs
    t = timed({"warp": lambda: ops.dyn_voxel_warp(pts, tt, ctrl, rig, n, gr),
               "dp": lambda: ops.dyn_voxel_jac_quad(pts, tt, ctrl, None, n, gr),
               "rigid": lambda: ops.dyn_voxel_jac_quad(pts, tt, ctrl, rig, n, gr, e),
               "bwd": lambda: ops.dyn_voxel_jac_quad_backward(pts, tt, S, n, gr, g)}, a.reps, a.inner)
    rows.append(row("dyn_voxel_warp (the yardstick: same rows)", t["warp"], shape, N * (16 + 28) + grid_bytes + 4 * S ** 3,
                    note="bytes = positions, times and the three outputs per sample + both grids once"))
    rows.append(row("dyn_voxel_jac_quad, dp form, v = ones", t["dp"], shape, N * (16 + 4) + grid_bytes))
    rows.append(row("dyn_voxel_jac_quad, rigid form, v = e", t["rigid"], shape, N * (16 + 12 + 4) + grid_bytes + 4 * S ** 3))
    rows.append(row("dyn_voxel_jac_quad_backward, fp32 atomics", t["bwd"], shape, N * (16 + 4) + 2 * grid_bytes,
                    atomic_bytes=N * 8 * row_bytes, note="added bytes = every contribution on its own; the time includes zeroing the gradient tensor"))
    config.set_deterministic(True)
    try:
        t = timed({"fixed": lambda: ops.dyn_voxel_jac_quad_backward(pts, tt, S, n, gr, g)}, a.reps, max(1, a.inner // 4))
    finally:
        config.set_deterministic(False)
    rows.append(row("dyn_voxel_jac_quad_backward, 2^-40 fixed point", t["fixed"], shape))

    # ---- each term against its double-autograd restatement
    t = timed({"hip": lambda: ops.dyn_voxel_jac_quad(pts, tt, ctrl, rig, n, gr, e), "torch": torch_ffjord}, a.reps, max(1, a.inner // 4))
    rows.append(row("--ffjord-div-decay term (one launch)", t["hip"], shape))
    rows.append(row("torch restatement, autograd.grad w.r.t. pts", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))
    t = timed({"hip": hip_divergence, "torch": torch_divergence}, a.reps, max(1, a.inner // 4))
    rows.append(row("--dyn-diverge-decay term, value + gradient", t["hip"], shape))
    rows.append(row("torch restatement, double autograd", t["torch"], shape, note="plain-torch restatement written for this tool (the baseline)"))

    # ---- a training iteration of the recipe without the flags and with each
    with tempfile.TemporaryDirectory() as td:
        data = make_scene(os.path.join(td, "scene"), size=64, n_train=12, n_test=3, dynamic=True) + "/"

        def trainer(extra):
            args = T.args_from_argv(["-d", data, "--epochs", str(a.iters)] + RECIPE + extra)
            T.seed(args.seed)
            labels, cam, _ = loaders.load(args, training=True)
            model = T.load_model(args, True, dev)
            model.nerf.steps, model.nerf.t_near, model.nerf.t_far = args.steps, args.near, args.far
            T.unset_voxel_tv(args, model)
            opt = T.load_optim(args, model.parameters())
            cam = cam.to(dev)
            return lambda: T.train(model, cam, labels, opt, args)
        sides = {"none": trainer([]), "ffjord": trainer(["--ffjord-div-decay", "0.3"]), "diverge": trainer(["--dyn-diverge-decay", "0.1"])}
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in sides}
        for _ in range(a.reps):
            for k, fn in sides.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.iters)
    it_shape = f"2 x 44 x 44 x {steps}, S={S}"
    rows.append(row("training iteration, make dyn_voxel minus --ffjord-div-decay", ms["none"], it_shape, note=f"host clock over {a.iters} iterations"))
    rows.append(row("training iteration, make dyn_voxel as shipped", ms["ffjord"], it_shape))
    rows.append(row("training iteration, --dyn-diverge-decay 0.1 instead", ms["diverge"], it_shape))
    finish(a, rows)


if __name__ == "__main__":
    main()
