#!/usr/bin/env python3
"""The Fourier encoder's position gradient (csrc/fourier_grad.hip) and the training step it opens, timed in one call:

  1. the backward kernel at N = 262 144 samples (D = 3, F = 128, sigma 16: VolSDF's MLP SDF network), as the init rows' gradient
     (pitch 259, features at column 3, the raw columns added) and as the standalone encoder's (pitch 256), in both variants --
     `recompute` (m, sin, cos again with the forward's arithmetic) and `read_back` (sin / cos from the forward's saved rows: twice the
     bytes) -- against the same gradient formed by existing operators the way SkipConnMLP.forward_with_input_tangents forms the
     encoder's Jacobian: fourier_encode, the swap of its halves, mul_bcast with the signed basis, mul_bcast with the upstream
     gradient, a sum over the features, the add of the raw columns;
  2. the forward rows kernel against cat([x, fourier_encode(x)]);
  3. a training step (forward, loss, backward, one-launch Adam) of DynamicNeRF(VolSDF(sdf.MLP), spline 6, pos-linear-view) next to the
     static VolSDF(sdf.MLP) step on the same rays: 2 views x 32 x 32 rays x 64 steps = 131 072 samples, both training arithmetics.

Timing: device events around `iters` calls after `warm` warm-up calls, the variants alternated inside every repetition, median and
min / max of the repetitions.  Algorithmic bytes of the kernel: recompute reads g's 256 feature columns + x and writes gx
(1 024 + 12 + 12 (+ 12 lead) bytes per sample), read_back the 256 saved columns on top.  No ratio is asserted: the numbers are the record.

    python tools/fourier_grad_bench.py [--json profiles/fourier_grad/bench.json] [--reps 7]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.procedural import proc_param, proc_uniform  # noqa: E402


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


def kernel_section(ops, N, reps):
    dev = torch.device("cuda", 0)
    D, F = 3, 128
    basis = torch.from_numpy(proc_param("basis", (D, F)) * 16.0).to(dev)
    x = torch.from_numpy(proc_uniform((N, D), 1, 3.0)).to(dev)
    g_rows = torch.from_numpy(proc_uniform((N, D + 2 * F), 2, 1.0)).to(dev)
    g_feat = g_rows[:, D:].contiguous()
    rows = ops.fourier_rows(x, basis, 1.0)
    enc = ops.fourier_encode(x, basis, 1.0)
    signed = torch.cat([basis, -basis], dim=-1)[:, None, :].expand(D, N, 2 * F).contiguous()  # (a constant of the step: built once)

    def operators():
        e = ops.fourier_encode(x, basis, 1.0)
        swapped = torch.cat([e[:, F:], e[:, :F]], dim=-1).contiguous()
        denc = ops.mul_bcast(swapped, signed)
        return ops.mul_bcast(g_feat, denc).sum(dim=-1).t() + g_rows[:, :D]

    fns = {
        "rows_recompute": lambda: ops.fourier_encode_backward_input(x, basis, 1.0, g_rows, col0=D, lead=True),
        "rows_read_back": lambda: ops.fourier_encode_backward_input(x, basis, 1.0, g_rows, col0=D, lead=True, saved=rows, saved_col0=D),
        "standalone_recompute": lambda: ops.fourier_encode_backward_input(x, basis, 1.0, g_feat),
        "standalone_read_back": lambda: ops.fourier_encode_backward_input(x, basis, 1.0, g_feat, saved=enc),
        "existing_operators": operators,
        "forward_rows": lambda: ops.fourier_rows(x, basis, 1.0),
        "forward_encode_cat": lambda: torch.cat([x, ops.fourier_encode(x, basis, 1.0)], dim=-1),
    }
    a, b, c = fns["rows_recompute"](), fns["rows_read_back"](), fns["existing_operators"]()
    assert torch.equal(a, b), "reading the forward's own sin / cos back gives the recomputed bits"
    scale = float(c.abs().max())
    agree = float((a - c).abs().max()) / scale
    t = alternate(fns, reps, iters=20)
    per = 2 * F * 4 + 2 * D * 4
    nbytes = {"rows_recompute": N * (per + D * 4), "rows_read_back": N * (per + D * 4 + 2 * F * 4), "standalone_recompute": N * per,
              "standalone_read_back": N * (per + 2 * F * 4), "forward_rows": N * (D * 4 + (D + 2 * F) * 4)}
    return dict(N=N, D=D, F=F, sigma=16, variants_bit_identical=True, kernel_vs_operators_linf_of_max=agree,
                timings={k: summary(v, nbytes.get(k)) for k, v in t.items()})


def step_section(reps):
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import cameras, config, render
    dev = torch.device("cuda", 0)
    size, crop, steps = 64, (16, 16, 32, 32), 64
    focal = 0.5 * size / math.tan(0.5 * 0.6911)
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]], [[0.8, -0.36, 0.48, 1.9], [0.0, 0.8, 0.6, 2.4], [-0.6, -0.48, 0.64, 2.6]]])
    cam = cameras.NeRFCamera(cam_to_world=c2w, focal=focal).to(dev)
    times = torch.tensor([0.25, 0.8], device=dev)
    target = torch.from_numpy(proc_uniform((2, 32, 32, 3), 3, 0.5)).to(dev) + 0.5
    common = dict(data="s/", model="volsdf", sdf_kind="mlp", refl_kind="pos-linear-view", sigmoid_kind="upshifted", near=2.0, far=6.0,
                  steps=steps, learning_rate=3e-4, size=size, render_size=size)
    out = {"samples": 2 * 32 * 32 * steps, "steps": steps}
    for prec in ("bf16x3", "fp32"):
        config.set_train_precision(prec)
        torch.manual_seed(0)
        models = {"static_volsdf_mlp": (T.load_model(T.make_args(**common)), None),
                  "dnerf_volsdf": (T.load_model(T.make_args(dyn_model="plain", spline=6, data_kind="dnerf", **common), is_dyn=True), times)}
        fns = {}
        for name, (m, tt) in models.items():
            m.train()
            opt = T.load_optim(T.make_args(**common), m.parameters())

            def step(m=m, tt=tt, opt=opt):
                o, _ = render.render(m, cam, crop, size=size, times=tt)
                torch.nn.functional.mse_loss(o, target).backward()
                opt.step()
                opt.zero_grad()
            fns[name] = step
        t = alternate(fns, reps, iters=5, warm=3)
        out[prec] = {k: dict(median_ms=round(statistics.median(v) * 1e3, 3), min_ms=round(min(v) * 1e3, 3), max_ms=round(max(v) * 1e3, 3),
                             reps=len(v)) for k, v in t.items()}
    config.set_train_precision("bf16x3")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--samples", type=int, default=262144)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    from nerf_atlas_amd import ops
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, kernel=kernel_section(ops, a.samples, a.reps),
               train_step=step_section(a.reps))
    print(json.dumps(res, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
