#!/usr/bin/env python3
"""The dense per-ray-step renderer against the sparse launch of a sparsified --model voxel (csrc/voxel_sparse.hip, `--voxel-sparsify`;
DESIGN.md 3w), written to profiles/voxel_sparse/bench.json.

    python tools/voxel_sparse_bench.py [--reps 7] [--inner 10] [--out profiles/voxel_sparse]

Scene and tile are tools/voxel_fine_bench.py's: the seeded thin shell of radius 0.8 in an S = 64 grid, `make voxel`'s 64 x 64 test tile
(near 2 / far 6, rays from the project's ray generator), the per-voxel RGB head (C = 3) and the spherical-harmonic head of order 4
(C = 75), at 64 and 128 uniform steps.  Per head and step count, in ONE process with the routes alternated inside every repetition and
warmed up first (voxel_fine_bench.timed_both: device events over `inner` calls, and wall time around a synchronise per call):
    dense      ops.voxel_*_render_rayts on rows that all equal the uniform row (the parent's lanes-per-ray kernel)
    shared     ops.voxel_render / voxel_sh_render on the row itself (the thread-per-ray kernel NeRFVoxel.forward runs without a table)
    sparse     ops.voxel_sparse_render on the same rows, with three tables:
                 all      thresh 0: every voxel live -- the price of the test and the compaction, shown whatever it is
                 half     the table of a THICKER shell around the same surface, grown until about half of the table is live: a superset
                          of the natural table, so the image is the natural one (the shell's density has two values only: no threshold on
                          it leaves half)
                 natural  NeRFVoxel.sparsify(1e-2) of the shell itself
Before any time is quoted every route's image is compared against the dense 1024-step render (PSNR over the tile, and over the rays that
meet the shell: on the others the reference's 1e10-long closing interval paints a fog that a positive threshold removes), the live
fractions of voxels and of samples are counted, and with the table of ones the sparse launch is checked bit for bit against the dense one.  Then the training step
(forward + backward on `make voxel`'s 40 x 40 x 10 crop) with and without the natural table.  The parent process never opens the GPU."""
import argparse
import json
import math
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import voxel_fine_bench as B  # noqa: E402

HEADS = (("rgb", -1), ("sh", 4))
STEPS = (64, 128)
SIZE, TILE, VIEWS, SIDE = 64, (0, 0, 64, 64), 10, 40


def thick_shell_table(ops, dev, want=0.5):
    """the table of the shell | |p| - 0.8 | < w with w grown by bisection until `want` of the table is live"""
    import torch
    c = (torch.arange(B.S, dtype=torch.float64) + 0.5) * (2 * B.GR / B.S) - B.GR
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    r = (x * x + y * y + z * z).sqrt()
    lo, hi = 0.05, 1.5
    for _ in range(20):
        w = 0.5 * (lo + hi)
        den = torch.where((r - 0.8).abs() < w, 40.0, -20.0)[..., None].float().to(dev)
        live, count = ops.voxel_live_table(den, 1e-2)
        lo, hi = (w, hi) if int(count) < want * live.numel() else (lo, w)
    return live


def child(a):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "a GPU measurement: no fallback"
    from nerf_atlas_amd import ops
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    rows, images = [], []
    focal = 0.5 * SIZE / math.tan(0.5 * FOV_X)
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(VIEWS)])).float().to(dev)
    rays = ops.raygen(c2w[:1], focal, SIZE, TILE)
    lo = (SIZE - SIDE) // 2
    crop = ops.raygen(c2w, focal, SIZE, (lo, lo, SIDE, SIDE))
    R = rays.numel() // 6
    for head, order in HEADS:
        den, rgb = B.shell_grids(head, order, dev)
        name = f"{head}{order if order >= 0 else ''}"
        natural, _ = ops.voxel_live_table(den, 1e-2)
        tables = {"all": ops.voxel_live_table(den, 0)[0], "half": thick_shell_table(ops, dev), "natural": natural}
        assert bool(tables["all"].all()) and bool((tables["half"] >= natural).all())

        def shared(ts):
            if head == "sh":
                return ops.voxel_sh_render(rays, ts, den, rgb, order, B.GR, "upshifted", "black")
            return ops.voxel_render(rays, ts, den, rgb, B.GR, "upshifted", "black")

        def dense(rows_):
            if head == "sh":
                return ops.voxel_sh_render_rayts(rays, rows_, den, rgb, order, B.GR, "upshifted", "black")
            return ops.voxel_render_rayts(rays, rows_, den, rgb, B.GR, "upshifted", "black")

        def sparse(rows_, live):
            return ops.voxel_sparse_render(head, rays, rows_, den, rgb, live, B.GR, order, "upshifted", "black")

        want, _, w_ref = shared(torch.linspace(2.0, 6.0, B.REF_STEPS, device=dev))
        # the closing interval is 1e10 |d| long: outside the shell sigma = softplus(-21) = 7.6e-10 still gives the LAST step alpha 1 - e^-7.6 on
        # every ray that misses the shell, a sample sparsify(1e-2) calls dead.  Both errors are quoted: over the tile, and over the rays whose
        # closing step carries no weight in the reference (the rays that meet the shell)
        hit = w_ref[-1] < 1e-3
        mse = lambda x, m: float(-10 * torch.log10((x - want)[m].square().mean().clamp(min=1e-20)))
        psnr = lambda x: dict(psnr_db=mse(x, torch.ones_like(hit)), psnr_hit_db=mse(x, hit))
        for steps in STEPS:
            ts = torch.linspace(2.0, 6.0, steps, device=dev)
            rows_ = ts.expand(tuple(rays.shape[:-1]) + (steps,)).contiguous()
            img = dense(rows_)
            assert torch.equal(img[0], shared(ts)[0])
            assert all(torch.equal(x, y) for x, y in zip(sparse(rows_, tables["all"]), img))   # a table of ones: the dense bits
            sides = {"dense per-ray-step renderer": lambda: dense(rows_), "dense shared-step renderer (thread per ray)": lambda: shared(ts)}
            info = {k: psnr(img[0]) for k in sides}
            for k, live in tables.items():
                got = sparse(rows_, live)
                flags = ops.voxel_live_samples(live, B.GR, rays=rays, ts=ts)
                label = f"sparse, {k} table"
                info[label] = dict(psnr(got[0]), live_voxels=float(live.float().mean()), live_samples=float(flags.float().mean()),
                                   max_abs_against_dense=float((got[0] - img[0]).abs().max()))
                sides[label] = (lambda l: lambda: sparse(rows_, l))(live)
                sides[f"sparse, {k} table, shared row"] = (lambda l: lambda: sparse(ts, l))(live)
                info[f"sparse, {k} table, shared row"] = info[label]
            images.append(dict(head=name, steps=steps, rays=R, rays_that_meet_the_shell=int(hit.sum()), routes=info))
            for k, v in info.items():
                print(f"[{name} {steps} steps] {k:46s} PSNR {v['psnr_db']:6.2f} dB, {v['psnr_hit_db']:6.2f} dB over the {int(hit.sum())} rays that meet the shell" + (f"  live voxels {v['live_voxels']:.3f} samples "
                      f"{v['live_samples']:.3f}  max |sparse - dense| {v['max_abs_against_dense']:.2e}" if "live_voxels" in v else ""), flush=True)
            t = B.timed_both(sides, a.reps, a.inner)
            for k, v in t.items():
                rows.append(B.row(k, f"tile R={R} M={steps} {name}", *v, **info[k]))

        # ---- training crop: forward + backward with and without the natural table (the lookups and scatters still visit dead samples)
        target = torch.full(tuple(crop.shape[:-1]) + (3,), 0.5, device=dev)
        plain, marked = B.build_model(head, order, 64, 0, den, rgb, True), B.build_model(head, order, 64, 0, den, rgb, True)
        marked.live = natural

        def step(m):
            def run():
                m.densities.grad = m.rgb.grad = None
                (m(crop) - target).square().mean().backward()
            return run
        t = B.timed_both({"no table": step(plain), "natural table": step(marked)}, a.reps, max(1, a.inner // 2))
        for k, v in t.items():
            rows.append(B.row(f"training forward + backward, {k}", f"crop R={crop.numel() // 6} M=64 {name}", *v))
        del plain, marked
    print("ROWS " + json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rows=rows, images=images)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_sparse"))
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.reps >= 5
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--inner", str(a.inner)], capture_output=True,
                       text=True, timeout=900)
    sys.stdout.write("\n".join(l for l in r.stdout.splitlines() if not l.startswith("ROWS ")) + "\n")
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"the timed process failed with exit status {r.returncode}: nothing further is started")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.tag + ".json"), "w") as f:
        json.dump(dict(library=os.environ.get("NA_LIB_PATH", "shipped"), reps=a.reps, inner=a.inner, **res), f, indent=1)


if __name__ == "__main__":
    main()
