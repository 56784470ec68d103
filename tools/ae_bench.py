"""One 800 x 800 x 128 frame of NeRFAE (`--model ae`, E = I = 32, procedural weights) rendered in slabs of image rows, per precision,
through two routes in the same process:

  fused    ops.ae_front (both narrow networks, one launch) + ops.render_view_ls(beta=None) (View head + compositing, one launch)
  generic  the route built from the per-layer kernels only: fourier_encode + 14 exact-fp32 Linears (na_linear_f32) + the generic
           View MLP + na_composite, on slabs small enough for its [N, 387] rows, reported per sample

Per route: two warm frames (allocator, packed streams, clocks), then `iters` timed frames (HIP events around each frame), median and
spread.  The two kernels of the fused route are also timed alone on one slab (many launches each).  FLOP / sample by the shape rule
(2 x (185 472 + 28 736) front, 596 480 head), fractions against the nominal dense bf16 MFMA peak (the kernels issue three bf16 products
per multiply: the fraction of the matrix pipe they occupy is three times the algorithmic one), algorithmic HBM bytes per sample.
Prints one JSON line and writes it to profiles/ae/bench.json (or --out PATH).

    python tools/ae_bench.py [iters] [--out PATH] [--generic-frames N]
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
from nerf_atlas_amd import config, ops  # noqa: E402
from oracle.procedural import proc_param  # noqa: E402

SIZE, T, E, I = 800, 128, 32, 32
SLAB, SLAB_GENERIC = 16, 2            # image rows per launch: 1.6 M samples (fused), 0.2 M (generic: [N, 387] fp32 rows)
FLOP_FRONT, FLOP_HEAD = 2 * (185472 + 28736), 596480
PEAK_BF16 = 2.5e15                    # nominal dense bf16 MFMA rate of one MI355X


def procedural_(m):
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if v.numel() and v.dtype == torch.float32 and not k.endswith("primes"):
                t = torch.from_numpy(proc_param(k, tuple(v.shape)))
                v.copy_(t * 32.0 if k.endswith("basis") else t)


def event_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def clock_mhz():
    try:
        return int(torch.cuda.clock_rate())
    except Exception:  # noqa: BLE001  (no SMI binding in this environment: the figure is a note, not an input)
        return None


def main():
    args = sys.argv[1:]
    out_path = os.path.join(REPO, "profiles", "ae", "bench.json")
    gen_frames = 1
    for flag in ("--out", "--generic-frames"):
        if flag in args:
            i = args.index(flag)
            if flag == "--out":
                out_path = args[i + 1]
            else:
                gen_frames = int(args[i + 1])
            del args[i:i + 2]
    iters = int(args[0]) if args else 7
    dev = torch.device("cuda:0")
    focal = 0.5 * SIZE / math.tan(0.5 * 0.6911)
    c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]], device=dev)
    m = nerf.NeRFAE(steps=T, t_near=2.0, t_far=6.0, intermediate_size=I, encoding_size=E, sigmoid_kind="upshifted", bg="black").to(dev).eval()
    procedural_(m)
    slabs = [ops.raygen(c2w, focal, SIZE, (r0, 0, min(SLAB, SIZE - r0), SIZE)) for r0 in range(0, SIZE, SLAB)]
    small = [ops.raygen(c2w, focal, SIZE, (r0, 0, SLAB_GENERIC, SIZE)) for r0 in range(0, SIZE, SLAB_GENERIC)]
    n_frame = SIZE * SIZE * T
    y_ld = 1 + E + I
    res = {"workload": f"{SIZE} x {SIZE} x {T}, E = I = {E}, fused slabs of {SLAB} rows, generic slabs of {SLAB_GENERIC} rows",
           "device": torch.cuda.get_device_name(0), "clock_mhz_before": clock_mhz(), "iters": iters,
           "flop_per_sample": {"front": FLOP_FRONT, "head": FLOP_HEAD, "total": FLOP_FRONT + FLOP_HEAD},
           "hbm_bytes_per_sample": {"front": round(24.0 / T + 4 * y_ld, 1), "head": round(4 * y_ld + (24.0 + 12.0) / T, 1),
                                    "generic_front_rows": 4 * sum(a + b for a, b in [(259, 128), (387, 128), (128, 128), (128, 128), (387, 128),
                                                                                      (128, 128), (128, E), (E, 64), (64 + E, 64), (64, 64),
                                                                                      (64, 64), (64 + E, 64), (64, 64), (64, 1 + I)])},
           "precisions": {}}
    with torch.no_grad():
        for prec in ("bf16x3", "f16x", "bf16"):
            config.set_precision(prec)
            r = {}

            def frame():
                for rays in slabs:
                    m(rays)
            frame(); frame()
            torch.cuda.synchronize()
            ms = [event_ms(frame) for _ in range(iters)]
            r["fused_frame"] = stats(ms)
            r["fused_Msamples_s"] = round(n_frame / statistics.median(ms) / 1e3, 1)
            # the two kernels alone on one slab
            rays = slabs[len(slabs) // 2]
            _, _, ts, _ = nerf.compute_ts(rays, 2.0, 6.0, T)
            n = rays.numel() // 6 * T
            kp = config.kernel_precision(has_f16x=True)
            rows = m.front_rows(rays, ts)
            front = lambda: m.front_rows(rays, ts)  # noqa: E731
            head = lambda: ops.render_view_ls(rays, ts, rows, None, m.packed_view_ls(kp), kp, m.refl.act_kind, "black", True)  # noqa: E731
            for name, fn, flop in (("front", front, FLOP_FRONT), ("head", head, FLOP_HEAD)):
                fn(); fn()
                torch.cuda.synchronize()
                ks = [event_ms(fn, reps=10) for _ in range(iters)]
                t = statistics.median(ks)
                r[name + "_slab"] = dict(stats(ks), samples=n, Msamples_s=round(n / t / 1e3, 1), tflops=round(n * flop / t / 1e9, 1),
                                         fraction_of_bf16_peak=round(n * flop / (t * 1e-3) / PEAK_BF16, 4))
            res["precisions"][prec] = r
            print(f"{prec}: fused frame {r['fused_frame']['median_ms']} ms ({r['fused_Msamples_s']} Msamples/s), front alone "
                  f"{r['front_slab']['median_ms']} ms, head alone {r['head_slab']['median_ms']} ms on {n} samples", flush=True)
        # the generic route: per-layer kernels only (what the parent commit could have launched for these shapes)
        config.set_precision("bf16x3")
        m._front_ok = lambda pts: False

        def gframe():
            for rays in small:
                m(rays)
        for rays in small[:20]:
            m(rays)
        torch.cuda.synchronize()
        ms = [event_ms(gframe) for _ in range(gen_frames)]
        del m._front_ok
        res["generic_frame"] = dict(stats(ms), frames=gen_frames)
        res["generic_Msamples_s"] = round(n_frame / statistics.median(ms) / 1e3, 1)
    res["clock_mhz_after"] = clock_mhz()
    res["speedup_fused_over_generic_bf16x3"] = round(res["generic_frame"]["median_ms"] / res["precisions"]["bf16x3"]["fused_frame"]["median_ms"], 2)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
