#!/usr/bin/env python3
"""Compositing over per-ray steps (csrc/composite_rayts.hip) and the training step it opens, timed in one call:

  1. the forward and the backward kernels at (T, R) = (128, 16384), (192, 4096), (192, 16384) -- the backward in both forms,
     `seq` (one thread per ray walks T) and `seg` (a thread per 16-step segment, the segments meeting in LDS) -- next to
     na_composite / na_composite_backward at the same (T, R) on shared steps, which is what the step cost before per-ray rows.
     Per sample the per-ray kernels read 5 input floats (density, 3 colours, its step) where the shared ones read 4, and write the
     same outputs: the cap the shipped form is held to is 1.25 x the shared kernel's time.
  2. one training step at 64 + 128 (2 views x 32 x 32 rays; forward, joint loss, backward, one-launch Adam) next to a shared-step
     step with 192 steps on the same rays.  The coarse pass is extra work: the ratio is the record, there is no target.

Timing: device events around `iters` calls after `warm` warm-up calls, the variants alternated inside every repetition, median and
min / max of the repetitions.  No ratio is asserted: the numbers are the record (DESIGN.md 3h quotes them).

    python tools/composite_rayts_bench.py [--json profiles/coarse_fine_train/bench.json] [--reps 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.procedural import proc_uniform  # noqa: E402

SIZES = ((128, 16384), (192, 4096), (192, 16384))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def alternate(fns, reps, iters, warm=3):
    """{name: [seconds per call] x reps}: every repetition times every variant once, in turn"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            out[k].append(window(fn, iters))
    return out


def summary(ts, nbytes=None):
    d = dict(median_us=round(statistics.median(ts) * 1e6, 2), min_us=round(min(ts) * 1e6, 2), max_us=round(max(ts) * 1e6, 2), reps=len(ts))
    if nbytes is not None:
        d.update(bytes=nbytes, gb_per_s=round(nbytes / statistics.median(ts) * 1e-9, 1))
    return d


def kernel_section(ops, T, R, reps):
    """the operators write into fresh tensors like the training step's do (the caching allocator hands the same blocks back)"""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(T + R)
    density = torch.from_numpy(proc_uniform((T, R), 1, 4.0)).to(dev)
    feat = (torch.from_numpy(proc_uniform((T, R, 3), 2, 0.5)) + 0.5).to(dev)
    rays = torch.cat([torch.zeros(R, 3), torch.from_numpy(proc_uniform((R, 3), 3, 1.0))], -1).to(dev)
    ts, _ = ops.compute_ts(2.0, 6.0, T, dev)
    rows = torch.sort(2.0 + 4.0 * torch.rand(R, T, generator=g), dim=1).values.to(dev)   # every ray its own increasing row
    g_out = torch.from_numpy(proc_uniform((R, 3), 4, 1.0)).to(dev)
    fns = {
        "forward_shared": lambda: ops.composite(density, feat, ts, rays, True, "white"),
        "forward_rayts": lambda: ops.composite_rayts(density, feat, rows, rays, True, "white"),
        "backward_shared": lambda: ops.composite_backward(density, feat, ts, rays, g_out, True, "white"),
        "backward_rayts_seq": lambda: ops.composite_rayts_backward(density, feat, rows, rays, g_out, True, "white", form="seq"),
        "backward_rayts_seg": lambda: ops.composite_rayts_backward(density, feat, rows, rays, g_out, True, "white", form="seg"),
        "backward_rayts_auto": lambda: ops.composite_rayts_backward(density, feat, rows, rays, g_out, True, "white"),
        "pts_shared": lambda: ops.compute_pts(rays, ts),
        "pts_rayts": lambda: ops.compute_pts_rayts(rays, rows),
    }
    # the two backward forms are the same sums in another association: they agree to rounding, and the shipped one is one of them
    a, b, c = fns["backward_rayts_seq"](), fns["backward_rayts_seg"](), fns["backward_rayts_auto"]()
    agree = float((a[0] - b[0]).abs().max() / a[0].abs().max())
    shipped = "seg" if torch.equal(c[0], b[0]) and torch.equal(c[1], b[1]) else "seq" if torch.equal(c[0], a[0]) else "?"
    t = alternate(fns, reps, iters=20)
    n = T * R
    nbytes = {"forward_shared": n * (4 + 2) * 4, "forward_rayts": n * (5 + 2) * 4, "backward_shared": n * (4 + 4) * 4,
              "backward_rayts_seq": n * (5 + 4) * 4 + 2 * n * 4 + n * 4, "backward_rayts_seg": n * (5 + 4) * 4,
              "pts_shared": n * 12, "pts_rayts": n * 16}
    res = dict(T=T, R=R, shipped_backward_form=shipped, seq_vs_seg_linf_of_max=agree, timings={k: summary(v, nbytes.get(k)) for k, v in t.items()})
    med = {k: statistics.median(v) for k, v in t.items()}
    res["ratios"] = dict(forward_rayts_over_shared=round(med["forward_rayts"] / med["forward_shared"], 3),
                         backward_seq_over_shared=round(med["backward_rayts_seq"] / med["backward_shared"], 3),
                         backward_seg_over_shared=round(med["backward_rayts_seg"] / med["backward_shared"], 3),
                         backward_shipped_over_shared=round(med["backward_rayts_auto"] / med["backward_shared"], 3))
    return res


def step_section(reps):
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import cameras, config, render
    dev = torch.device("cuda", 0)
    size, crop = 64, (16, 16, 32, 32)
    focal = 0.5 * size / math.tan(0.5 * 0.6911)
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]], [[0.8, -0.36, 0.48, 1.9], [0.0, 0.8, 0.6, 2.4], [-0.6, -0.48, 0.64, 2.6]]])
    cam = cameras.NeRFCamera(cam_to_world=c2w, focal=focal).to(dev)
    target = torch.from_numpy(proc_uniform((2, 32, 32, 3), 3, 0.5)).to(dev) + 0.5
    common = dict(data="s/", model="plain", refl_kind="view", sigmoid_kind="upshifted", near=2.0, far=6.0, size=size, render_size=size)
    recipes = {"coarse_fine_64_128": dict(steps=64, steps_fine=128), "shared_192": dict(steps=192, steps_fine=0),
               "shared_64": dict(steps=64, steps_fine=0)}
    out = {"rays": 2 * 32 * 32}
    for prec in ("bf16x3", "fp32"):
        config.set_train_precision(prec)
        torch.manual_seed(0)
        fns = {}
        for name, r in recipes.items():
            args = T.make_args(**common, **r)
            m = T.load_model(args)
            m.steps, m.t_near, m.t_far = args.steps, args.near, args.far
            m.train()
            opt = T.load_optim(args, m.parameters())
            mse = torch.nn.functional.mse_loss

            def step(m=m, opt=opt, fine=r["steps_fine"] > 0):
                o, _ = render.render(m, cam, crop, size=size)
                loss = mse(o, target)
                if fine:
                    loss = loss + mse(m.coarse, target)
                loss.backward()
                opt.step()
                opt.zero_grad()
            fns[name] = step
        t = alternate(fns, reps, iters=5, warm=3)
        med = {k: statistics.median(v) for k, v in t.items()}
        out[prec] = {k: dict(median_ms=round(med[k] * 1e3, 3), min_ms=round(min(v) * 1e3, 3), max_ms=round(max(v) * 1e3, 3), reps=len(v))
                     for k, v in t.items()}
        out[prec]["coarse_fine_over_shared_192"] = round(med["coarse_fine_64_128"] / med["shared_192"], 3)
    config.set_train_precision("bf16x3")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-step", action="store_true", help="kernels only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from nerf_atlas_amd import ops
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__,
               kernels=[kernel_section(ops, T, R, a.reps) for T, R in SIZES])
    if not a.no_step:
        res["train_step"] = step_section(a.reps)
    print(json.dumps(res, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
