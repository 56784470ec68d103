"""One 800 x 800 x 128 frame of PlainNeRF + the spherical-harmonic head (`--refl-kind sph-har`, order 2, procedural weights) rendered in
slabs of 24 image rows, through both routes of refl.SphericalHarmonic in the same process:

  hoisted  per-ray view terms (ops.sh_view_terms) + seven row Linears over the latent columns + ops.sh_shade   (what inference takes)
  plain    [N, 322] init rows through SkipConnMLP's exact-fp32 Linears + ops.sh_shade                         (forced here)

One warm frame per route, then `iters` frames; the median frame time is reported (HIP events around each frame), next to the head alone
on one slab (the MLP `first` and the compositing are the same kernels on both routes).  Writes profiles/sh_head/bench.json (or --out PATH).

    python tools/sh_head_bench.py [iters] [--frames-only] [--out PATH]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/sh_head_bench.py 1 --frames-only      # the per-kernel split
"""
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import nerf_atlas_amd.nerf as nerf  # noqa: E402
import nerf_atlas_amd.refl as refl  # noqa: E402
from nerf_atlas_amd import config, ops  # noqa: E402
from oracle.procedural import proc_param  # noqa: E402

SIZE, T, SLAB, ORDER = 800, 128, 24, 2


def procedural_(m):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if v.numel() and v.dtype == torch.float32 and not k.endswith("primes"):
                t = torch.from_numpy(proc_param(k, tuple(v.shape)))
                v.copy_(t * 32.0 if k.endswith("basis") else t)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    args = sys.argv[1:]
    out_path = os.path.join(REPO, "profiles", "sh_head", "bench.json")
    if "--out" in args:
        i = args.index("--out")
        out_path = args[i + 1]
        del args[i:i + 2]
    argv = [a for a in args if not a.startswith("--")]
    iters = int(argv[0]) if argv else 5
    frames_only = "--frames-only" in args
    dev = torch.device("cuda:0")
    focal = 0.5 * SIZE / math.tan(0.5 * 0.6911)
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]], device=dev)
    config.set_precision("bf16x3")
    m = nerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted", bg="black")
    m.set_refl(refl.refl_kinds["sph-har"](latent_size=64, act="upshifted", out_features=3, order=ORDER))
    m = m.to(dev).eval()
    procedural_(m)
    head = m.refl
    slabs = [ops.raygen(c2w, focal, SIZE, (r0, 0, min(SLAB, SIZE - r0), SIZE)) for r0 in range(0, SIZE, SLAB)]

    def frame():
        for rays in slabs:
            m(rays)

    def set_route(route):
        if route == "plain":
            head._hoistable = lambda *a: False
        elif "_hoistable" in head.__dict__:
            del head._hoistable

    res = {"workload": f"{SIZE} x {SIZE} x {T}, slabs of {SLAB} rows ({len(slabs)} per frame), order {ORDER}, first in bf16x3",
           "iters": iters, "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        frames = {}
        for route in ("hoisted", "plain"):
            set_route(route)
            frame()  # warm: allocator, packed streams, the head's cached latent-column matrices
            torch.cuda.synchronize()
            ms = [event_ms(frame) for _ in range(iters)]
            frames[route] = ms
            res[f"frame_ms_{route}"] = round(statistics.median(ms), 2)
            res[f"frame_ms_{route}_all"] = [round(x, 2) for x in ms]
            print(f"{route}: frame {statistics.median(ms):.2f} ms (median of {iters}: {[round(x, 1) for x in ms]})", flush=True)
        if not frames_only:
            # the head alone on one full slab: latent = first's 64 intermediate columns, by pitch, as PlainNeRF hands them over
            rays = slabs[0]
            pts, ts, r_o, r_d, _ = nerf.compute_pts_ts(rays, 2.0, 6.0, T)
            first_out = m.first(pts, None)
            view = r_d.unsqueeze(0).expand_as(pts)
            lat = first_out[..., 1:]
            n = pts.numel() // 3
            for route in ("hoisted", "plain"):
                set_route(route)
                fn = lambda: head(x=pts, view=view, latent=lat)  # noqa: E731
                fn()
                torch.cuda.synchronize()
                ms = statistics.median(event_ms(fn) for _ in range(iters))
                res[f"head_slab_ms_{route}"] = round(ms, 3)
                res[f"head_Msamples_s_{route}"] = round(n / ms / 1e3, 1)
                print(f"{route}: head alone on {n} samples {ms:.3f} ms", flush=True)
            set_route("hoisted")
            ms = statistics.median(event_ms(lambda: m.first(pts, None)) for _ in range(iters))
            res["first_slab_ms"] = round(ms, 3)
            a = head(x=pts, view=view, latent=lat)
            set_route("plain")
            b = head(x=pts, view=view, latent=lat)
            res["routes_max_abs_diff"] = float((a - b).abs().max())
        set_route("hoisted")
    res["speedup_frame"] = round(res["frame_ms_plain"] / res["frame_ms_hoisted"], 3)
    print(json.dumps(res), flush=True)
    if not frames_only:
        try:  # (the per-kernel split of a trace run, added to the record by hand, survives a re-measurement)
            with open(out_path) as fh:
                res["kernel_split"] = json.load(fh)["kernel_split"]
        except (OSError, ValueError, KeyError):
            pass
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
