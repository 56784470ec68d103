#!/usr/bin/env python3
"""Times of SSIM / MS-SSIM on the GPU (csrc/ssim.hip) next to the plain-torch restatement on the same device, written to
profiles/ssim/bench.json.

    python tools/ssim_bench.py [--reps 9] [--inner 50] [--out profiles/ssim]

Device events around `inner` back-to-back calls, every shape warmed up first, the two sides of a comparison alternated inside one
repetition, the median of `reps` repetitions with the spread next to it.
  * the `make dnerf` training crop, 2 x 18 x 18 x 3: 1 - mean SSIM forward and backward (train.loss_map["ssim"] against the fp32 torch
    restatement with autograd: grouped F.conv2d on permuted copies, what a user would otherwise run);
  * ops.ms_ssim on a batch of eight 256 x 256 x 3 test frames against the fp32 torch restatement (no backward: a metric).
Next to the times: the error of both sides against the fp64 restatement of tests/ssim_ref.py and the bound the kernels are held to.
No speed-up is promised; the file records what was measured.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def torch_ssim(x, y, g):
    """the definition in fp32 torch operators on the device: channel-last in, (ssim [N,C], cs [N,C])"""
    x, y = x.permute(0, 3, 1, 2), y.permute(0, 3, 1, 2)
    C = x.shape[1]
    gv, gh = g.reshape(1, 1, 11, 1).expand(C, 1, 11, 1), g.reshape(1, 1, 1, 11).expand(C, 1, 1, 11)
    filt = lambda v: F.conv2d(F.conv2d(v, gv, groups=C), gh, groups=C)
    mu1, mu2 = filt(x), filt(y)
    s1, s2, s12 = filt(x * x) - mu1 * mu1, filt(y * y) - mu2 * mu2, filt(x * y) - mu1 * mu2
    cs = (2 * s12 + 9e-4) / (s1 + s2 + 9e-4)
    s = (2 * mu1 * mu2 + 1e-4) / (mu1 * mu1 + mu2 * mu2 + 1e-4) * cs
    return s.mean(dim=(2, 3)), cs.mean(dim=(2, 3))


def torch_ms_ssim(x, y, g):
    vals = []
    for i in range(5):
        s, cs = torch_ssim(x, y, g)
        vals.append(torch.relu(cs if i < 4 else s))
        if i < 4:
            pool = lambda v: F.avg_pool2d(v.permute(0, 3, 1, 2), 2, padding=[v.shape[1] % 2, v.shape[2] % 2]).permute(0, 2, 3, 1)
            x, y = pool(x), pool(y)
    w = torch.tensor(WEIGHTS, device=x.device)[:, None, None]
    return torch.prod(torch.stack(vals) ** w, dim=0)


def timed(fns, reps, inner):
    """{name: [ms per call] x reps}: the sides alternate inside a repetition"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / inner)
    return out


def row(name, shape, ms, **extra):
    return dict(name=name, shape=shape, ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), reps=len(ms), **extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ssim"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback"
    import ssim_ref as R
    from nerf_atlas_amd import ops, train
    dev = torch.device("cuda")
    g = R.window().float().to(dev)
    rows = []

    # ---- the training crop: forward + backward
    x, y = R.image_pair(2, 18, 18, 3)
    xd, yd = x.to(dev).requires_grad_(True), y.to(dev)
    loss_hip = train.loss_map["ssim"]

    def step_hip():
        xd.grad = None
        loss_hip(xd, yd).backward()

    def step_torch():
        xd.grad = None
        (1 - torch_ssim(xd, yd, g)[0].mean()).backward()
    t = timed({"hip": step_hip, "torch": step_torch}, a.reps, a.inner)
    gup = torch.full((2, 3), -1.0 / 6.0, dtype=torch.float64)
    g_ref, g_bound = R.ssim_grad_ref(x, y, gup), R.ssim_grad_terms(x, y, gup)[1] + R.U * R.ssim_grad_ref(x, y, gup).abs()
    errs = {}
    for k, fn in (("hip", step_hip), ("torch", step_torch)):
        fn()
        errs[k] = dict(grad_max_err=float((xd.grad.cpu().double() - g_ref).abs().max()), grad_worst_ratio=R.worst_ratio(xd.grad, g_ref, g_bound))
    for k, what in (("hip", "train.loss_map['ssim'] forward + backward (na_ssim: 2 launches, na_ssim_backward: 1)"),
                    ("torch", "fp32 torch restatement forward + backward (autograd)")):
        rows.append(row(what, "2 x 18 x 18 x 3", t[k], grad_bound_max=float(g_bound.max()), **errs[k]))

    # ---- the metric on a batch of test frames
    x, y = R.image_pair(8, 256, 256, 3)
    xd, yd = x.to(dev), y.to(dev)
    with torch.no_grad():
        t = timed({"hip": lambda: ops.ms_ssim(xd, yd), "torch": lambda: torch_ms_ssim(xd, yd, g)}, a.reps, max(a.inner // 5, 4))
        ref, bound = R.ms_ssim_bound(x, y)
        for k, what, got in (("hip", "ops.ms_ssim (5 x na_ssim + 4 x na_image_halve + the combination)", ops.ms_ssim(xd, yd)),
                             ("torch", "fp32 torch restatement of ms_ssim", torch_ms_ssim(xd, yd, g))):
            rows.append(row(what, "8 x 256 x 256 x 3", t[k], max_err=float((got.cpu().double() - ref).abs().max()), bound_max=float(bound.max()),
                            worst_ratio=R.worst_ratio(got, ref, bound)))
    os.makedirs(a.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, inner=a.inner, rows=rows)
    with open(os.path.join(a.out, "bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    for r in rows:
        print(f"{r['name']:<95} {r['shape']:<18} {r['ms_median']:.4f} ms ({r['ms_min']:.4f} .. {r['ms_max']:.4f})")


if __name__ == "__main__":
    main()
