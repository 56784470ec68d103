#!/usr/bin/env python3
"""Times of --model voxel on the GPU (csrc/voxel.hip), written to profiles/voxel/bench.json.

    python tools/voxel_bench.py [--reps 9] [--inner 20] [--frame 800] [--out profiles/voxel]

Device events around `inner` back-to-back calls, every shape warmed up first, the sides of a comparison alternated inside one
repetition, the median of `reps` repetitions with the spread (min .. max) next to it.  Next to each time: the bytes the algorithm
needs from the shapes (NOT the bytes the gathers move through the caches), and for the scatter the added bytes over the time
against the 1.3 TB/s chip-wide rate of global float atomics.

Shapes: `make voxel`'s training batch (makefile:30-34: --size 64 --crop-size 40 --batch-size 10, near 2 / far 6 -- one 40 x 40 crop of
10 pinhole views on the radius-4 sphere x 64 steps = 1 024 000 samples, S = 64) and one 800 x 800 x 64 frame of the first view in
eval mode.  The rays come from the project's ray generator (ops.raygen), so neighbouring rays are neighbouring pixels.  "torch" rows are a plain-PyTorch restatement of the lookup written for this tool (advanced indexing + autograd:
what a user would otherwise run), not a kernel of this project.
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
sys.path.insert(0, os.path.join(REPO, "tests"))

ATOMIC_RATE = 1.3e12   # added bytes per second, global float atomics (chip-wide, measured shape: 256 contiguous bytes per wave)


def torch_lookup(pts, densities, rgb, grid_radius):
    """the lookup in plain torch on the device, per axis like tests/voxel_ref.py (what a user would otherwise run); raw [..., 4]"""
    S = densities.shape[0]
    step = grid_radius * 2 / S
    last = grid_radius - step / 2

    def centre(n):
        return ((torch.floor(n.clamp(-grid_radius, grid_radius) / step + 1e-10) + 0.5) * step).clamp(-last, last)
    lo, hi = centre(pts - 0.5 * step), centre(pts + 0.5 * step)                      # [..., 3]
    frac = (pts - lo) / step
    index = lambda c: (torch.floor(c / step + 1e-10) + S / 2).long().clamp(0, S - 1)
    idx, wgt = (index(lo), index(hi)), (1 - frac, frac)
    grid = torch.cat([densities, rgb], dim=-1)
    out = 0
    for u in range(8):
        b = [(u >> i) & 1 for i in range(3)]
        w = wgt[b[0]][..., 0] * wgt[b[1]][..., 1] * wgt[b[2]][..., 2]
        out = out + w[..., None] * grid[idx[b[0]][..., 0], idx[b[1]][..., 1], idx[b[2]][..., 2]]
    return out


def timed(sides, reps, inner):
    """{name: [ms per call] * reps}: the sides alternate inside every repetition"""
    for fn in sides.values():
        fn()
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / inner)
    return out


def row(name, ms, shape, bytes_alg=None, note=None, atomic_bytes=None):
    med = statistics.median(ms)
    r = dict(name=name, shape=shape, ms_median=med, ms_min=min(ms), ms_max=max(ms), reps=len(ms))
    if bytes_alg is not None:
        r.update(algorithmic_bytes=bytes_alg, algorithmic_GBps=bytes_alg / med / 1e6)
    if atomic_bytes is not None:
        r.update(added_bytes=atomic_bytes, added_TBps=atomic_bytes / med / 1e9, share_of_atomic_rate=atomic_bytes / (med * 1e-3) / ATOMIC_RATE)
    if note:
        r["note"] = note
    print(f"{name:44s} {shape:28s} {med:9.4f} ms  ({min(ms):.4f} .. {max(ms):.4f})"
          + (f"  {r['algorithmic_GBps']:8.1f} GB/s algorithmic" if bytes_alg is not None else "")
          + (f"  {r['added_TBps']:.3f} TB/s added = {r['share_of_atomic_rate']:.2f} of the atomic rate" if atomic_bytes is not None else ""))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "voxel"))
    ap.add_argument("--only-scatter", action="store_true", help="stop after the gather and scatter rows (A/B builds of csrc/voxel.hip under NA_LIB_PATH)")
    ap.add_argument("--tag", default="bench", help="name of the json file")
    a = ap.parse_args()
    assert a.reps >= 7 and torch.cuda.is_available(), "a GPU measurement: no fallback"
    import voxel_ref as V
    from nerf_atlas_amd import config, nerf, ops, refl, train
    dev = torch.device("cuda")
    S, T, gr = 64, 64, 1.3
    den, rgb = (t.to(dev) for t in V.grid_values(S))
    grid_bytes = 4 * 4 * S ** 3
    rows = []

    # ---- the training batch of `make voxel`
    from tools.make_scene import FOV_X, look_at_origin
    c2w = torch.from_numpy(np.stack([look_at_origin(0.7 * i, 0.3 + 0.04 * i)[:3] for i in range(10)])).float().to(dev)
    focal = lambda size: 0.5 * size / math.tan(0.5 * FOV_X)
    rays = ops.raygen(c2w, focal(64), 64, (12, 12, 40, 40))
    assert rays.shape == (10, 40, 40, 6)
    ts = torch.linspace(2.0, 6.0, T, device=dev)
    R, N = rays.numel() // 6, T * rays.numel() // 6
    shape = f"N={N} S={S}"
    pts = ops.compute_pts(rays, ts)
    g_raw = torch.from_numpy(V.proc_uniform((N, 4), 4801, 1.0)).to(dev)
    io = R * 24 + T * 4 + N * 16 + grid_bytes
    t = timed({"hip": lambda: ops.voxel_sample(den, rgb, gr, rays=rays, ts=ts),
               "hip_pts": lambda: ops.voxel_sample(den, rgb, gr, pts=pts),
               "torch": lambda: torch_lookup(pts, den, rgb, gr)}, a.reps, a.inner)
    rows.append(row("voxel_sample (rays x ts)", t["hip"], shape, io))
    rows.append(row("voxel_sample (explicit pts)", t["hip_pts"], shape, io + N * 12 - R * 24))
    rows.append(row("torch lookup, forward", t["torch"], shape, io + N * 12 - R * 24, note="plain-torch restatement written for this tool"))

    dr, rr = den.clone().requires_grad_(True), rgb.clone().requires_grad_(True)

    def torch_fwd_bwd():
        dr.grad = rr.grad = None
        torch_lookup(pts, dr, rr, gr).backward(g_raw.reshape(pts.shape[:-1] + (4,)))

    def scatter():   # (the mode is process-wide: config.set_deterministic around the timed calls)
        ops.voxel_sample_backward(g_raw, S, gr, rays=rays, ts=ts)
    added = N * 8 * 16
    t = timed({"atomics": scatter}, a.reps, a.inner)
    rows.append(row("voxel_sample_backward, fp32 atomics", t["atomics"], shape, R * 24 + N * 16 + 2 * grid_bytes, atomic_bytes=added,
                    note="added bytes = every contribution as if it went to memory on its own; the kernel sums on chip first.  The time includes "
                         "allocating and zeroing the two gradient tensors (4 MiB) in ops.voxel_sample_backward"))
    config.set_deterministic(True)
    try:
        t = timed({"fixed": scatter}, a.reps, a.inner)
    finally:
        config.set_deterministic(False)
    rows.append(row("voxel_sample_backward, 2^-40 fixed point", t["fixed"], shape, R * 24 + N * 16 + 2 * grid_bytes + 2 * 8 * 4 * S ** 3,
                    atomic_bytes=added))
    if a.only_scatter:
        return finish(a, rows)
    t = timed({"torch": torch_fwd_bwd}, a.reps, max(1, a.inner // 4))
    rows.append(row("torch lookup, forward + backward", t["torch"], shape, note="plain-torch restatement written for this tool"))

    def operator_route(rays_, ts_):
        raw = ops.voxel_sample(den, rgb, gr, rays=rays_, ts=ts_)
        return ops.composite(raw[..., 0].contiguous(), ops.sigmoid(raw[..., 1:].contiguous(), "upshifted"), ts_, rays_)
    t = timed({"render": lambda: ops.voxel_render(rays, ts, den, rgb, gr, "upshifted", "black"),
               "operators": lambda: operator_route(rays, ts)}, a.reps, a.inner)
    rows.append(row("voxel_render (one launch)", t["render"], f"R={R} T={T} S={S}", R * 24 + T * 4 + 2 * N * 4 + R * 12 + grid_bytes))
    rows.append(row("operator route (sample, act, composite)", t["operators"], f"R={R} T={T} S={S}"))

    # ---- one frame in eval mode
    F = a.frame
    rays_f = ops.raygen(c2w[:1], focal(F), F, (0, 0, F, F))
    Rf = F * F
    t = timed({"render": lambda: ops.voxel_render(rays_f, ts, den, rgb, gr, "upshifted", "black"),
               "render_out_only": lambda: ops.voxel_render(rays_f, ts, den, rgb, gr, "upshifted", "black", want_weights=False),
               "operators": lambda: operator_route(rays_f, ts)}, a.reps, max(1, a.inner // 4))
    rows.append(row("voxel_render frame", t["render"], f"{F}x{F}x{T} S={S}", Rf * 24 + T * 4 + 2 * T * Rf * 4 + Rf * 12 + grid_bytes))
    rows.append(row("voxel_render frame, no alpha / weights", t["render_out_only"], f"{F}x{F}x{T} S={S}", Rf * 24 + T * 4 + Rf * 12 + grid_bytes))
    rows.append(row("operator route frame", t["operators"], f"{F}x{F}x{T} S={S}"))

    # ---- a whole training step: forward, loss, backward, one-launch Adam
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    m.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    m = m.to(dev).train()
    opt = train.NaAdam(m.parameters(), lr=1e-2)
    target = torch.full(tuple(rays.shape[:-1]) + (3,), 0.5, device=dev)

    def step():
        opt.zero_grad()
        (m(rays) - target).square().mean().backward()
        opt.step()
    t = timed({"step": step}, a.reps, a.inner)
    rows.append(row("training step (fwd, l2, bwd, Adam)", t["step"], shape))

    finish(a, rows)


def finish(a, rows):
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, a.tag + ".json"), "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, library=os.environ.get("NA_LIB_PATH", "shipped"),
                       reps=a.reps, inner=a.inner, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
