#!/usr/bin/env python3
"""One optimiser step of every --opt-kind on PlainNeRF(view)'s parameter list: the one-launch step (csrc/optim.hip, train.NaSGD /
NaRMSprop / NaAdam / NaAdamW) against torch's foreach optimiser of the same kind.

    python tools/optim_bench.py [--reps 9] [--inner 50] [--out profiles/optim]

The method of tools/voxel_bench.py (its `timed` and `row`): same process, same parameter shapes, gradients set once; both sides warmed
up, alternated inside every repetition; device events around `inner` back-to-back steps (a step is a few launches: the window also
holds the host's work between them, which is part of what a training loop pays); the median of `reps` repetitions with the spread.
The algorithmic bytes of a step: every parameter and state tensor read and written once, the gradient read once.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

KINDS = {  # kind: (class name, hyperparameters, state tensors)
    "sgd": ("NaSGD", dict(lr=2e-2), 0),
    "rmsprop": ("NaRMSprop", dict(lr=2e-2, eps=1e-7), 1),
    "adam": ("NaAdam", dict(lr=5e-4, eps=1e-7), 2),
    "adam --decay 1e-5": ("NaAdam", dict(lr=5e-4, eps=1e-7, weight_decay=1e-5), 2),
    "adamw": ("NaAdamW", dict(lr=5e-4, eps=1e-7), 2),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "optim"))
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import nerf_atlas_amd.nerf as nerf
    import nerf_atlas_amd.train as T
    from tools.voxel_bench import row, timed
    dev = torch.device("cuda")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in nerf.PlainNeRF(steps=64, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted").parameters()]
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    rows = []
    for kind, (name, hyper, states) in KINDS.items():
        sides = {}
        for side, cls in (("one launch", getattr(T, name)), ("torch foreach", getattr(T, name).TORCH)):
            ps = [torch.nn.Parameter(torch.randn(*s, device=dev) * 0.1) for s in shapes]
            for p in ps:
                p.grad = torch.randn_like(p) * 1e-3
            sides[side] = cls(ps, **hyper, **({"foreach": True} if side == "torch foreach" else {})).step
        t = timed(sides, a.reps, a.inner)
        shape = f"{len(shapes)} tensors, {numel} elements"
        for side in sides:
            rows.append(row(f"{kind}: {side}", t[side], shape, numel * 4 * (3 + 2 * states)))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "optim_bench.json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, reps=a.reps, inner=a.inner, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
