#!/usr/bin/env python3
"""Uniform sampling against coarse -> fine sampling of --model voxel at EQUAL sample count (csrc/voxel_fine.hip, `--voxel-steps-fine`;
DESIGN.md 3v), written to profiles/voxel_fine/bench.json.

    python tools/voxel_fine_bench.py [--reps 7] [--inner 10] [--no-trace] [--out profiles/voxel_fine]

Geometries: `make voxel`'s (--size 64, 64 steps: the 64 x 64 test frame is one tile; training crop 40 x 40 x 10 views) and `make dyn_voxel`'s
(--size 128, 80 steps, --test-crop-size 64: a 64 x 64 tile; training crop 44 x 44 x 2 views), near 2 / far 6, S = 64, rays from the project's ray
generator.  Heads: the per-voxel RGB head (C = 3) and the spherical-harmonic head of order 4 (C = 75).  Per geometry, head and shape, in
ONE process with the two routes alternated inside every repetition and warmed up first:
    uniform        NeRFVoxel.forward at --steps T + N                                   (test tile: eval, one launch; crop: training step fwd + bwd)
    coarse-fine    NeRFVoxel.forward at --steps T --voxel-steps-fine N  (T = N)         (the same)
    its launches   ops.voxel_proposal, ops.resample_ts, ops.voxel_*_render_rayts separately (test tiles)
Each as device-event time over `inner` back-to-back calls AND as wall time around a synchronise per call (launch overheads included).
The kernels' own times come from a separate run of the same routes under `rocprofv3 --kernel-trace --stats` (never in the timed process).
Before any time is quoted the outputs of both routes on the same inputs are compared against a --steps 1024 uniform render of one seeded
analytic grid -- a thin dense shell of radius 0.8, generated here -- and both image errors are printed: the comparison that matters is
the time at equal ERROR, not at equal sample count.  Also: every lane count of the per-ray-step kernel (ops.voxel_fine_lanes) on
`make voxel`'s tile, next to the thread-per-ray shared-step renderer at the same step count.  The parent process never opens the GPU."""
import argparse
import csv
import glob
import json
import math
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

S, GR, REF_STEPS = 64, 1.3, 1024
# name, --size, total steps, test tile (crop of the frame), training crop (views, side)
GEOMETRIES = (("voxel", 64, 64, (0, 0, 64, 64), (10, 40)), ("dyn_voxel", 128, 80, (32, 32, 64, 64), (2, 44)))
HEADS = (("rgb", -1), ("sh", 4))
KERNELS = ("voxel_fine_kernel", "resample_ts_kernel", "plv_render_kernel")


def shell_grids(head, order, dev, seed=8100):
    """one seeded analytic scene: density logit +40 inside the shell | |p| - 0.8 | < 0.05 and -20 elsewhere (sigma = softplus(d - 1): 39 per
    unit length against 1e-9), colour parameters a smooth function of the position plus seeded noise; SH: that colour in the constant
    coefficient and seeded higher orders"""
    import torch
    g = torch.Generator().manual_seed(seed)
    c = (torch.arange(S, dtype=torch.float64) + 0.5) * (2 * GR / S) - GR
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    r = (x * x + y * y + z * z).sqrt()
    den = torch.where((r - 0.8).abs() < 0.05, 40.0, -20.0)[..., None].float()
    col = torch.stack([2 * x, 2 * y, 2 * z], dim=-1).float() + 0.3 * torch.randn(S, S, S, 3, generator=g)
    if head == "rgb":
        return den.to(dev), col.contiguous().to(dev)
    nk = (order + 1) ** 2
    co = 0.2 * torch.randn(S, S, S, 3, nk, generator=g)
    co[..., 0] = col / 0.28209479177387814
    return den.to(dev), co.reshape(S, S, S, 3 * nk).contiguous().to(dev)


def build_model(head, order, steps, steps_fine, den, rgb, train=False):
    import torch
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=steps, bg="black", sigmoid_kind="upshifted")
    if head == "sh":
        m.set_refl(refl.SphericalHarmonic(act="upshifted", latent_size=0, out_features=3, order=order, voxel_order=order))
    else:
        m.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    m.set_sigmoid("upshifted")
    m = m.to(den.device)
    with torch.no_grad():
        m.densities.copy_(den)
        m.rgb.copy_(rgb)
    m.steps_fine = steps_fine
    return m.train() if train else m.eval()


def timed_both(sides, reps, inner):
    """{name: (event ms per call [reps], wall ms per call around a synchronise [reps])}; the sides alternate inside every repetition"""
    import torch
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ev, wall = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ev[k].append(a.elapsed_time(b) / inner)
        for k, fn in sides.items():
            w = []
            for _ in range(inner):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                w.append((time.perf_counter() - t0) * 1e3)
            wall[k].append(statistics.median(w))
    return {k: (ev[k], wall[k]) for k in sides}


def row(name, shape, ev, wall, **extra):
    r = dict(name=name, shape=shape, ms_median=statistics.median(ev), ms_min=min(ev), ms_max=max(ev), wall_ms_median=statistics.median(wall),
             wall_ms_min=min(wall), wall_ms_max=max(wall), reps=len(ev), **extra)
    print(f"{name:52s} {shape:30s} events {r['ms_median']:8.4f} ms ({r['ms_min']:.4f} .. {r['ms_max']:.4f})   wall {r['wall_ms_median']:8.4f} ms", flush=True)
    return r


def routes(ops, head, order, rays, den, rgb, T, N):
    """the launches of both eval routes on explicit operators (what NeRFVoxel._render / forward_coarse_fine run)"""
    import torch
    ts_u = torch.linspace(2.0, 6.0, T + N, device=rays.device)
    ts_c = torch.linspace(2.0, 6.0, T, device=rays.device)

    def shared(ts):
        if head == "sh":
            return ops.voxel_sh_render(rays, ts, den, rgb, order, GR, "upshifted", "black")
        return ops.voxel_render(rays, ts, den, rgb, GR, "upshifted", "black")

    def fine(ts_ray, lanes=None):
        if lanes is not None:
            return ops.voxel_fine_lanes(head, lanes, rays, ts_ray, den, rgb, GR, order, "upshifted", "black")
        if head == "sh":
            return ops.voxel_sh_render_rayts(rays, ts_ray, den, rgb, order, GR, "upshifted", "black")
        return ops.voxel_render_rayts(rays, ts_ray, den, rgb, GR, "upshifted", "black")
    return ts_u, ts_c, shared, fine


def child(a):
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "a GPU measurement: no fallback"
    from nerf_atlas_amd import ops
    from tools.make_scene import FOV_X, look_at_origin
    dev = torch.device("cuda")
    rows, errors = [], []
    for head, order in HEADS:
        if a.head and a.head != head:
            continue
        den, rgb = shell_grids(head, order, dev)
        for gname, size, total, tile, (views, side) in GEOMETRIES:
            T = N = total // 2
            focal = 0.5 * size / math.tan(0.5 * FOV_X)
            c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(views)])).float().to(dev)
            rays = ops.raygen(c2w[:1], focal, size, tile)
            lo = (size - side) // 2
            crop = ops.raygen(c2w, focal, size, (lo, lo, side, side))
            R = rays.numel() // 6
            ts_u, ts_c, shared, fine = routes(ops, head, order, rays, den, rgb, T, N)
            uni, cf = build_model(head, order, T + N, 0, den, rgb), build_model(head, order, T, N, den, rgb)

            # ---- the two routes' outputs on the same inputs, against the 1024-step render
            with torch.no_grad():
                want = shared(torch.linspace(2.0, 6.0, REF_STEPS, device=dev))[0]
                got_u, got_c = uni(rays), cf(rays)
            assert cf.ts_ray.shape[-1] == T + N and uni.ts_ray is None and uni.weights.shape[0] == T + N
            err = lambda x: dict(mean_abs=float((x - want).abs().mean()), max_abs=float((x - want).abs().max()),
                                 psnr_db=float(-10 * torch.log10((x - want).square().mean().clamp(min=1e-20))))
            e = dict(geometry=gname, head=f"{head}{order if order >= 0 else ''}", rays=R, steps=T + N, uniform=err(got_u), coarse_fine=err(got_c))
            errors.append(e)
            print(f"[{gname} {e['head']}] image error against {REF_STEPS} uniform steps at {T + N} samples per ray: uniform mean |err| "
                  f"{e['uniform']['mean_abs']:.5f} (PSNR {e['uniform']['psnr_db']:.2f} dB), coarse-fine {T} + {N} mean |err| "
                  f"{e['coarse_fine']['mean_abs']:.5f} (PSNR {e['coarse_fine']['psnr_db']:.2f} dB)", flush=True)
            if a.trace_only:
                with torch.no_grad():
                    for _ in range(a.inner):
                        uni(rays)
                        cf(rays)
                torch.cuda.synchronize()
                continue

            # ---- test tile, eval mode
            shape = f"{gname} tile R={R} {T}+{N} {e['head']}"
            _, w = ops.voxel_proposal(rays, ts_c, den, GR)
            ts_ray = ops.resample_ts(ts_c, w, N)

            def nograd(fn):
                def run():
                    with torch.no_grad():
                        return fn()
                return run
            t = timed_both({"uniform": nograd(lambda: uni(rays)), "coarse-fine": nograd(lambda: cf(rays)),
                            "proposal": lambda: ops.voxel_proposal(rays, ts_c, den, GR), "resample": lambda: ops.resample_ts(ts_c, w, N),
                            "fine": lambda: fine(ts_ray)}, a.reps, a.inner)
            rows.append(row("uniform route, eval forward", shape, *t["uniform"]))
            rows.append(row("coarse-fine route, eval forward", shape, *t["coarse-fine"]))
            for k, n in (("proposal", "  voxel_proposal"), ("resample", "  resample_ts"), ("fine", "  per-ray-step render")):
                rows.append(row(n, shape, *t[k]))

            # ---- lanes per ray (the tile of `make voxel`)
            if gname == "voxel":
                want_f = fine(ts_ray)
                sides = {"thread per ray (shared-step renderer)": lambda: shared(ts_u)}
                for lanes in ops.VOXEL_FINE_LANES:
                    assert all(torch.equal(x, y) for x, y in zip(fine(ts_ray, lanes), want_f))
                    sides[f"{lanes} lanes per ray"] = (lambda l: lambda: fine(ts_ray, l))(lanes)
                    if head == "rgb":
                        sides[f"proposal, {lanes} lanes per ray"] = (lambda l: lambda: ops.voxel_fine_lanes("density", l, rays, ts_c, den, None, GR))(lanes)
                t = timed_both(sides, a.reps, a.inner)
                for k, v in t.items():
                    rows.append(row(f"lanes: {k}", f"R={R} M={T + N} {e['head']}", *v))

            # ---- time at equal ERROR (the tile of `make voxel`): uniform rows of other lengths through both uniform kernels, other splits
            if gname == "voxel":
                sides, errs = {}, {}
                for steps in (16, 24, 32, 48, 64, 96, 128):
                    ts_s = torch.linspace(2.0, 6.0, steps, device=dev)
                    rows_s = ts_s.expand(tuple(rays.shape[:-1]) + (steps,)).contiguous()
                    img = shared(ts_s)[0]
                    assert torch.equal(img, fine(rows_s)[0])
                    errs[f"uniform {steps}: shared-step renderer"] = errs[f"uniform {steps}: per-ray-step kernel on equal rows"] = err(img)
                    sides[f"uniform {steps}: shared-step renderer"] = (lambda t_: lambda: shared(t_))(ts_s)
                    sides[f"uniform {steps}: per-ray-step kernel on equal rows"] = (lambda r_: lambda: fine(r_))(rows_s)
                for tc, nf in ((16, 48), (32, 32), (48, 16), (64, 64)):
                    ts_k = torch.linspace(2.0, 6.0, tc, device=dev)

                    def three(ts_k=ts_k, nf=nf):
                        return fine(ops.resample_ts(ts_k, ops.voxel_proposal(rays, ts_k, den, GR)[1], nf))
                    errs[f"coarse-fine {tc} + {nf}: three launches"] = err(three()[0])
                    sides[f"coarse-fine {tc} + {nf}: three launches"] = three
                t = timed_both(sides, a.reps, a.inner)
                for k, v in t.items():
                    rows.append(row(f"error sweep: {k}", f"PSNR {errs[k]['psnr_db']:.2f} dB mean|err| {errs[k]['mean_abs']:.5f} {e['head']}", *v, error=errs[k]))

            # ---- training crop: forward + backward of both routes
            Rc = crop.numel() // 6
            ut, ct = build_model(head, order, T + N, 0, den, rgb, True), build_model(head, order, T, N, den, rgb, True)
            target = torch.full(tuple(crop.shape[:-1]) + (3,), 0.5, device=dev)

            def step(m):
                def run():
                    m.densities.grad = m.rgb.grad = None
                    (m(crop) - target).square().mean().backward()
                return run
            t = timed_both({"uniform": step(ut), "coarse-fine": step(ct)}, a.reps, max(1, a.inner // 2))
            shape = f"{gname} crop R={Rc} {T}+{N} {e['head']}"
            rows.append(row("uniform route, training forward + backward", shape, *t["uniform"]))
            rows.append(row("coarse-fine route, training forward + backward", shape, *t["coarse-fine"]))
            del ut, ct, uni, cf
    print("ROWS " + json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, rows=rows, errors=errors)))


def kernel_stats(a, head):
    """AverageNs per kernel of both eval routes on the test tiles, from one run under rocprofv3 --kernel-trace --stats"""
    work = tempfile.mkdtemp(prefix="voxel_fine_trace_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", work, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--trace-only", "--head", head, "--inner", str(a.inner)]
        r = subprocess.run(cmd, cwd=work, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(work, "**", "*kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"the kernel trace of head {head} failed with exit status {r.returncode}: nothing further is started")
        out = []
        for f in files:
            for line in csv.DictReader(open(f)):
                if any(k in line["Name"] for k in KERNELS):
                    out.append(dict(kernel=line["Name"], calls=int(line["Calls"]), average_us=float(line["AverageNs"]) / 1e3,
                                    min_us=float(line["MinNs"]) / 1e3, max_us=float(line["MaxNs"]) / 1e3))
        for k in out:
            print(f"[trace {head}] {k['average_us']:10.2f} us x {k['calls']:4d}  {k['kernel'][:120]}", flush=True)
        return out
    finally:
        shutil.rmtree(work, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 runs")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel_fine"))
    ap.add_argument("--tag", default="bench")
    ap.add_argument("--head", default="", help=argparse.SUPPRESS)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    assert a.reps >= 5
    if a.child:
        return child(a)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--inner", str(a.inner)], capture_output=True,
                       text=True, timeout=1100)
    sys.stdout.write("\n".join(l for l in r.stdout.splitlines() if not l.startswith("ROWS ")) + "\n")
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"the timed process failed with exit status {r.returncode}: nothing further is started")
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("ROWS ")][-1][5:])
    res["kernel_trace"] = {} if a.no_trace else {f"{h}{k if k >= 0 else ''}": kernel_stats(a, h) for h, k in HEADS}
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.tag + ".json"), "w") as f:
        json.dump(dict(library=os.environ.get("NA_LIB_PATH", "shipped"), reps=a.reps, inner=a.inner, **res), f, indent=1)


if __name__ == "__main__":
    main()
