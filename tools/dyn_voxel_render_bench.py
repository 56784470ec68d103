#!/usr/bin/env python3
"""One launch against the launches it replaces: the voxel D-NeRF's test renderer (csrc/dyn_voxel_render.hip) on the GPU, written to
profiles/dyn_voxel_render/bench.json.

    python tools/dyn_voxel_render_bench.py [--loads 3] [--reps 9] [--inner 20] [--out profiles/dyn_voxel_render]

Geometry: `make dyn_voxel`'s test set -- S 64, spline 4, 80 steps between 2 and 6, --test-crop-size 64 at --size 128 -- with all maps
(depth, acc, flow, rigidity), rays from the project's ray generator.  Two shapes: one 64 x 64 tile (4096 rays: 64 waves for 256 CUs)
and a whole 128 x 128 frame in one call (16 384 rays).  Two routes over the same tensors:
    one launch    ops.dyn_voxel_render
    composition   ops.compute_pts -> ops.dyn_voxel_warp -> ops.voxel_render(pts = warped) -> 4 x ops.integrate (+ the torch kernels
                  that form `ts`, the ones column and dp * rigidity for them), as DynamicNeRFVoxel.forward and render.depth_map /
                  alpha_map / flow_map / rigidity_map run them
The two are compared bit for bit before anything is timed.  Method: tools/voxel_bench.py's (device events around `inner`
back-to-back calls, both routes warmed up, the routes ALTERNATED inside every repetition of one call, the median of `reps`
repetitions with min .. max).  The whole measurement is LOADED `--loads` times, each in a fresh process: the spread of a route is
max - min of its per-load medians, and the project's rule calls the difference a gain only if it exceeds three times the larger
spread.  The parent process never opens the GPU."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

S, T, SPLINE, GR, SIZE = 64, 80, 4, 1.3, 128
SHAPES = (("64x64 tile", (32, 32, 64, 64)), ("128x128 frame", (0, 0, 128, 128)))
MAPS = ("depth", "acc", "flow", "rigidity")


def sample_bytes(R):
    """what the composition writes and reads back per call that the one launch keeps in registers: pts, warped, dp (12 B each),
    rigidity, alpha, weights (4 B each) written once; pts read by the warp, warped by the render, weights by the four integrations,
    dp once and rigidity twice by what feeds them"""
    return R * T * ((3 * 12 + 3 * 4) + (12 + 12 + 4 * 4 + 12 + 2 * 4))


def child(a):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_ref as V
    import dyn_voxel_ref as D
    from nerf_atlas_amd import ops
    from tools.make_scene import FOV_X, look_at_origin
    from tools.voxel_bench import row, timed
    dev = torch.device("cuda")
    den, rgb = (x.to(dev) for x in V.grid_values(S))
    ctrl, rig = (x.to(dev) for x in D.dyn_grids(S, SPLINE))
    ctrl = ctrl * 0.3
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7, 0.3)[:3]])).float().to(dev)
    ts = torch.linspace(2.0, 6.0, T, device=dev)
    rows = []
    for name, crop in SHAPES:
        rays = ops.raygen(c2w, 0.5 * SIZE / math.tan(0.5 * FOV_X), SIZE, crop)          # [1,h,w,6]
        batch = tuple(rays.shape[:-1])
        R = rays.numel() // 6
        t = torch.full(batch, 0.4, device=dev)

        def one_launch():
            return ops.dyn_voxel_render(rays, t, ts, den, rgb, ctrl, rig, SPLINE, GR, "upshifted", "black", want=MAPS)

        def composition():
            pts = ops.compute_pts(rays, ts)
            warped, dp, r = ops.dyn_voxel_warp(pts, t[None].expand((T,) + batch).contiguous(), ctrl, rig, SPLINE, GR)
            out, _, w = ops.voxel_render(rays, ts, den, rgb, GR, "upshifted", "black", True, pts=warped)
            ones = torch.ones(w.shape + (1,), device=dev)
            ones[-1] = 0
            r = r.unsqueeze(-1)
            return dict(rgb=out, depth=ops.integrate(w, ts[:, None, None, None, None].expand(w.shape + (1,)).contiguous()),
                        acc=ops.integrate(w, ones), flow=ops.integrate(w, (dp * r).contiguous()), rigidity=ops.integrate(w, r.contiguous()))
        a_, b_ = one_launch(), composition()
        assert all(torch.equal(a_[k], b_[k]) for k in ("rgb",) + MAPS), "the two routes must be the same bits before they are timed"
        ms = timed({"one launch": one_launch, "composition": composition}, a.reps, a.inner)
        shape = f"R={R} T={T} S={S} spline={SPLINE}"
        rows.append(row(f"{name}: one launch", ms["one launch"], shape, note="no per-sample tensor"))
        rows.append(row(f"{name}: composition", ms["composition"], shape, sample_bytes(R),
                        note="bytes = the per-sample tensors written and read back between its launches"))
    print("ROWS " + json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rows=rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loads", type=int, default=3, help="fresh processes the whole measurement is repeated in")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn_voxel_render"))
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.reps >= 7 and a.loads >= 2
    if a.child:
        return child(a)
    loads = []
    for i in range(a.loads):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--inner", str(a.inner)],
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"load {i} failed with exit status {r.returncode}: nothing further is started")
        loads.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:]))
        print(f"load {i}: " + "; ".join(f"{x['name']} {x['ms_median']:.4f} ms ({x['ms_min']:.4f} .. {x['ms_max']:.4f})" for x in loads[-1]["rows"]), flush=True)
    summary = []
    for name, _ in SHAPES:
        med = {route: [next(x["ms_median"] for x in l["rows"] if x["name"] == f"{name}: {route}") for l in loads]
               for route in ("one launch", "composition")}
        spread = max(max(v) - min(v) for v in med.values())
        diff = statistics.median(med["composition"]) - statistics.median(med["one launch"])
        verdict = "gain" if diff > 3 * spread else "loss" if -diff > 3 * spread else "no difference by the 3 x spread rule"
        summary.append(dict(shape=name, one_launch_ms=med["one launch"], composition_ms=med["composition"], difference_ms=diff,
                            spread_ms=spread, verdict=verdict))
        print(f"{name}: one launch {statistics.median(med['one launch']):.4f} ms, composition {statistics.median(med['composition']):.4f} ms, "
              f"difference {diff:+.4f} ms, spread of repeated loads {spread:.4f} ms -> {verdict}")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.tag + ".json"), "w") as f:
        json.dump(dict(device=loads[0]["device"], torch=loads[0]["torch"], library=os.environ.get("NA_LIB_PATH", "shipped"), reps=a.reps,
                       inner=a.inner, loads=[l["rows"] for l in loads], summary=summary), f, indent=1)


if __name__ == "__main__":
    main()
