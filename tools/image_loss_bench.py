#!/usr/bin/env python3
"""Times of the fused loss wrapper on the GPU (csrc/image_loss.hip) next to the plain-torch composition of the same definition on the
same device, written to profiles/image_loss/bench.json.

    python tools/image_loss_bench.py [--reps 9] [--inner 50] [--out profiles/image_loss]

Device events around `inner` back-to-back calls, every shape warmed up first, the two sides alternated inside one repetition, the
median of `reps` repetitions with the spread next to it.  Forward + backward of the function train.load_loss_fn returns under
--loss-fns l2 rmse --color-spaces rgb xyz hsv --tone-map --gamma-correct-loss 0.5 (ag.ImageLossFn: one launch each way) against
train.image_loss_torch with autograd, on `make dnerf`'s crop 2 x 18 x 18 x 3 and `make voxel`'s 10 x 40 x 40 x 3.  Next to the times:
the error of both sides against the fp64 restatement of tests/image_loss_ref.py, as the worst ratio to the bound the kernel is held
to.  No speed-up is promised; the file records what was measured.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

FLAGS = dict(loss_fns=["l2", "rmse"], color_spaces=["rgb", "xyz", "hsv"], tone_map=True, gamma_correct_loss=0.5)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image_loss"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU: there is no fallback"
    import image_loss_ref as R
    from nerf_atlas_amd import train
    combo = (tuple(FLAGS["loss_fns"]), tuple(FLAGS["color_spaces"]), FLAGS["tone_map"], FLAGS["gamma_correct_loss"])
    fused = train.load_loss_fn(train.make_args(**FLAGS))
    rows = []
    for shape in ((2, 18, 18, 3), (10, 40, 40, 3)):
        P = int(np.prod(shape[:-1]))
        got, ref = R.kink_free_draw(P, 40 + P)
        x, y = torch.from_numpy(got).cuda().view(shape).requires_grad_(True), torch.from_numpy(ref).cuda().view(shape)

        def step_hip():
            x.grad = None
            fused(x, y).backward()

        def step_torch():
            x.grad = None
            train.image_loss_torch(x, y, *combo).backward()
        t = timed({"hip": step_hip, "torch": step_torch}, a.reps, a.inner)
        r = R.restate(got, ref, *combo)
        for k, fn, what in (("hip", step_hip, "fused loss forward + backward (na_image_loss + na_image_loss_backward: 2 launches)"),
                            ("torch", step_torch, "fp32 torch composition forward + backward (autograd)")):
            fn()
            d = np.abs(x.grad.detach().cpu().numpy().reshape(-1, 3).astype(np.float64) - r["grad"])
            ms = t[k]
            rows.append(dict(name=what, shape=" x ".join(map(str, shape)), flags=FLAGS, ms_median=statistics.median(ms), ms_min=min(ms),
                             ms_max=max(ms), reps=len(ms), grad_max_err=float(d.max()),
                             grad_worst_ratio=float((d[r["grad_bound"] > 0] / r["grad_bound"][r["grad_bound"] > 0]).max())))
    os.makedirs(a.out, exist_ok=True)
    res = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, inner=a.inner, rows=rows)
    with open(os.path.join(a.out, "bench.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    for r in rows:
        print(f"{r['name']:<90} {r['shape']:<18} {r['ms_median']:.4f} ms ({r['ms_min']:.4f} .. {r['ms_max']:.4f})  grad err / bound "
              f"{r['grad_worst_ratio']:.3f}")


if __name__ == "__main__":
    main()
