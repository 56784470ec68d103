"""Compositing over per-ray steps with a backward (csrc/composite_rayts.hip): na_compute_pts_rayts, na_composite_rayts,
na_composite_rayts_backward.

  1. rows equal to shared steps give the bits of na_compute_pts / na_composite / na_composite_backward: the per-step arithmetic is
     restated operation for operation and the backward picks the same decomposition by T (T <= 128);
  2. per-ray rows against the fp64 reference of tests/composite_ref.py inside ITS derived per-element bounds (none invented here):
     ties and the 1e-5 floor (input F), merged rows of na_resample_ts, walls on the segment edges of rows of 193 and 256 steps in
     every backward form, and one row beyond the segmented form's 256 steps (the sequential kernel takes it);
  3. non-finite inputs: the criterion of tests/test_gpu_composite.py::h_check -- NaN exactly where the reference's own forward is
     NaN, every other ray bit for bit the clean run.  A NaN density or step makes the reference's ray NaN: out and the gradients
     are then non-finite.  An infinite DENSITY is finite in the reference (an opaque / an empty sample, alpha exactly 1 / 0) and
     stays so; an infinite step is an infinitely long interval -- alpha 1, a finite pixel -- whose chain factor dist * e = Inf * 0
     makes the gradients non-finite;
  4. two backward launches give the same bits (no atomics)."""
import numpy as np
import pytest
import torch

import composite_ref as CR
from oracle.procedural import proc_uniform
from test_gpu_coarse_fine import _weights

pytestmark = pytest.mark.gpu

KINDS = ("softplus", "relu")
BGS = ("black", "white", "random")
SAME_T = tuple(sorted(set(CR.A_SIZES + (16, 17, 128))))
FORMS_OF = lambda T: ("auto", "seq") + (("seg",) if 16 < T <= 256 else ())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def forward(ops, c, kind, bg, feat, rand, want=True):
    got = ops.composite_rayts(c["density"].cuda(), feat.cuda(), c["ts"].cuda(), CR.rays_of(c).cuda(), kind == "softplus", bg, want,
                              rand.cuda() if bg == "random" else None)
    return tuple(None if t is None else t.cpu() for t in got)


def backward(ops, c, kind, bg, feat, rand, g_out, form="auto"):
    gd, gf = ops.composite_rayts_backward(c["density"].cuda(), feat.cuda(), c["ts"].cuda(), CR.rays_of(c).cuda(), g_out.cuda(),
                                          kind == "softplus", bg, rand.cuda() if bg == "random" else None, form=form)
    return gd.cpu(), gf.cpu()


# ------------------------------------------------------------------------------------------------ 1. shared rows: the same bits
@pytest.mark.parametrize("T", SAME_T)
def test_rows_equal_to_shared_steps_give_the_shared_kernels_bits(ops, T):
    c = CR.input_a(T)                                     # 70 rays: more than one 64-ray tile, a ragged second one
    R = c["density"].shape[1]
    ts, rays = c["ts"].cuda(), CR.rays_of(c).cuda()
    ts_ray = ts.expand(R, T).contiguous()
    wide = _t(0.5 + 0.5 * proc_uniform((T, R, 8), 6400 + T, 1.0))
    rand = CR.rand_of(c).cuda()
    d = c["density"].cuda()
    for kind in KINDS:
        sp = kind == "softplus"
        for bg in BGS:
            rd = rand if bg == "random" else None
            for C in range(1, 9):                          # every C na_composite takes
                feat = wide[..., :C].contiguous().cuda()
                want = ops.composite(d, feat, ts, rays, sp, bg, True, rd)
                got = ops.composite_rayts(d, feat, ts_ray, rays, sp, bg, True, rd)
                for k, a, b in zip(("out", "alpha", "weights"), got, want):
                    assert torch.equal(a, b), (T, kind, bg, C, k)
                bare = ops.composite_rayts(d, feat, ts_ray, rays, sp, bg, False, rd)
                assert bare[1] is None and bare[2] is None and torch.equal(bare[0], want[0]), (T, kind, bg, C, "without weights")
            for C in (1, 3):                               # every C na_composite_backward takes
                feat = wide[..., :C].contiguous().cuda()
                g_out = _t(proc_uniform((R, C), 7100, 1.0)).cuda()
                want = ops.composite_backward(d, feat, ts, rays, g_out, sp, bg, rd)
                got = ops.composite_rayts_backward(d, feat, ts_ray, rays, g_out, sp, bg, rd)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (T, kind, bg, C, "backward")


@pytest.mark.parametrize("T,shape", [(1, (70,)), (33, (2, 5, 7)), (64, (65,)), (193, (130,))])
def test_positions_over_shared_rows_are_compute_pts(ops, T, shape):
    R = int(np.prod(shape))
    rays = _t(proc_uniform((R, 6), 6500 + T, 2.0)).reshape(shape + (6,)).cuda()
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    ts_ray = ts.expand(shape + (T,)).contiguous()
    got = ops.compute_pts_rayts(rays, ts_ray)
    assert got.shape == (T,) + shape + (3,) and torch.equal(got, ops.compute_pts(rays, ts))
    # per-ray rows: o + t d with one rounding per operation, whatever the row
    rows = (ts_ray + _t(proc_uniform(shape + (T,), 6501, 0.5)).cuda()).contiguous()
    want = rays[None, ..., :3] + rows.movedim(-1, 0)[..., None] * rays[None, ..., 3:]
    assert torch.equal(ops.compute_pts_rayts(rays, rows), want)


# ------------------------------------------------------------------------------------------------ 2. per-ray rows against fp64
def walls(T):
    """CR.input_b on per-ray rows: ray i has ONE opaque sample (+22 over steps of 0.95 .. 1.05 times |d| >= 1: e < 2^-24, alpha = 1
    in fp32) at the i-th of the steps 15, 16 (the first segment edge), 127, 128 (where the shared-step launcher stops segmenting),
    191, 192 (64 + 128), T - 2, T - 1 (the closing interval), and -40 everywhere else"""
    steps = sorted({s for s in (15, 16, 127, 128, 191, 192, T - 2, T - 1) if 0 <= s < T})
    R = len(steps)
    d = np.full((T, R), -40.0)
    for i, s in enumerate(steps):
        d[s, i] = 22.0
    ts = np.arange(T)[None] + 1.0 + 0.05 * proc_uniform((R, T), 6200 + T, 1.0)
    return dict(density=_t(d), ts=_t(ts), dirs=CR._dirs(R, 6201, norm=np.linspace(1.0, 1.5, R)), feat=CR._colours(T, R, 6202), kind="softplus")


def merged(ops, T, N, R):
    """rows of na_resample_ts (random draws) on the weight profiles of tests/test_gpu_coarse_fine.py, generic logits in [-6, 6]"""
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    w = _weights(T, max(R, 4), 7 * T + N)
    w = (w[:, 1:2] if R == 1 else w[:, :R]).contiguous()   # (one ray: the single-surface profile)
    u = torch.rand(N, R, generator=torch.Generator().manual_seed(N))
    rows = ops.resample_ts(ts, w.cuda(), N, u.cuda()).cpu()
    TT = T + N
    assert rows.shape == (R, TT) and bool((rows[:, 1:] >= rows[:, :-1]).all())
    return dict(density=_t(proc_uniform((TT, R), 6300 + TT, 6.0)), ts=rows, dirs=CR._dirs(R, 6301 + TT), feat=CR._colours(TT, R, 6302 + TT),
                kind="softplus")


def check_against_fp64(ops, c, tag, variants=(("black", 3), ("white", 3), ("random", 3), ("white", 1))):
    T, R = c["density"].shape
    assert c["ts"].shape == (R, T)
    rand = CR.rand_of(c)
    worst = {}
    for kind in KINDS:
        eps, eps_libm = CR.eps_sigma_of(c["density"], kind), CR.eps_sigma_of(c["density"], kind, libm=True)
        for bg, C in variants:
            feat = c["feat"][..., :C].contiguous()
            ref = CR.reference(c, kind, bg, rand, feat)
            b = CR.forward_bounds(ref, eps, feat, bg=bg, rand=rand)
            out, alpha, weights = forward(ops, c, kind, bg, feat, rand)
            r = dict(alpha=CR.worst_ratio(alpha, ref["alpha"], b["alpha"]), weights=CR.worst_ratio(weights, ref["weights"], b["weights"]),
                     out=CR.worst_ratio(out, ref["out"], b["out"]))
            g_out = _t(proc_uniform((R, C), 7100, 1.0))
            rd, rf = CR.composite_grads(c["density"], feat, c["ts"], c["dirs"], g_out, kind, bg, rand)
            b_d, b_f = CR.backward_bounds(ref, eps_libm, c["density"], feat, g_out, kind, bg, rand)
            for form in FORMS_OF(T):
                gd, gf = backward(ops, c, kind, bg, feat, rand, g_out, form)
                assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gf).all()), (tag, kind, bg, C, form)
                r[f"g_density {form}"], r[f"g_feat {form}"] = CR.worst_ratio(gd, rd, b_d), CR.worst_ratio(gf, rf, b_f)
            for k, v in r.items():
                worst[k] = max(worst.get(k, 0.0), v)
            print(f"[composite_rayts {tag} {kind} {bg} C={C}] error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
            assert all(v <= 1.0 for v in r.values()), (tag, kind, bg, C, r)
    print(f"\n[composite_rayts {tag}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_ties_and_the_interval_floor(ops):
    check_against_fp64(ops, CR.input_f(), "F")


@pytest.mark.parametrize("T,N,R", [(2, 5, 5), (33, 7, 65), (24, 40, 130), (64, 128, 70), (100, 156, 1)])
def test_merged_rows_of_the_resampler(ops, T, N, R):
    check_against_fp64(ops, merged(ops, T, N, R), f"merged {T}+{N}x{R}", variants=(("white", 3), ("random", 3), ("black", 1)))


@pytest.mark.parametrize("T", [193, 256])
def test_walls_on_the_segment_edges_of_long_rows(ops, T):
    check_against_fp64(ops, walls(T), f"walls {T}")


def test_a_row_beyond_the_segmented_form(ops):
    """257 steps: the segmented form is refused by name, the launcher's choice (the sequential kernel) meets the same bounds"""
    from nerf_atlas_amd._lib import NaError
    c = merged(ops, 100, 157, 67)
    check_against_fp64(ops, c, "merged 100+157x67", variants=(("white", 3),))
    feat = c["feat"]
    with pytest.raises(NaError, match="segmented"):
        backward(ops, c, "softplus", "white", feat, None, torch.ones(67, 3), form="seg")
    check_against_fp64(ops, walls(257), "walls 257", variants=(("white", 3),))


def test_empty_batch(ops):
    e = lambda *s: torch.empty(*s, device="cuda")
    out, a, w = ops.composite_rayts(e(9, 0), e(9, 0, 3), e(0, 9), e(0, 6))
    assert out.shape == (0, 3) and a.shape == (9, 0) and w.shape == (9, 0)
    gd, gf = ops.composite_rayts_backward(e(9, 0), e(9, 0, 3), e(0, 9), e(0, 6), e(0, 3))
    assert gd.shape == (9, 0) and gf.shape == (9, 0, 3)
    assert ops.compute_pts_rayts(e(0, 6), e(0, 9)).shape == (9, 0, 3)


# ------------------------------------------------------------------------------------------------ 3. non-finite inputs
NF_T, NF_RAY = 65, 37
NF_VALUES = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}


def nf_clean():
    c = dict(CR.input_a(NF_T))
    R = c["density"].shape[1]
    c["ts"] = torch.sort(c["ts"][None] + _t(0.02 * proc_uniform((R, NF_T), 6600, 1.0)), dim=1).values.contiguous()   # per-ray rows
    assert bool((c["ts"][:, 1:] > c["ts"][:, :-1]).all())
    return c


@pytest.mark.parametrize("where,value", [("density", "nan"), ("density", "+inf"), ("density", "-inf"), ("step", "nan"), ("step", "+inf")])
@pytest.mark.parametrize("step", (0, 31, 32, NF_T - 1))
def test_non_finite_inputs_stay_loud_and_in_their_ray(ops, where, value, step):
    clean = nf_clean()
    c = dict(clean)
    bad = clean["density" if where == "density" else "ts"].clone()
    if where == "density":
        bad[step, NF_RAY] = NF_VALUES[value]
        c["density"] = bad
    else:
        bad[NF_RAY, step] = NF_VALUES[value]
        c["ts"] = bad
    R = c["density"].shape[1]
    others = torch.arange(R) != NF_RAY
    rand = CR.rand_of(c)
    g_out = _t(proc_uniform((R, 3), 7100, 1.0))
    for kind in KINDS:
        for bg in ("white", "random"):
            ref = CR.composite_ref(c["density"], c["feat"], c["ts"], c["dirs"], kind, bg, rand)   # the reference's own fp32 forward
            pat = {k: torch.isnan(ref[k]) for k in ("alpha", "weights")}
            pat_out = bool(torch.isnan(ref["out"][NF_RAY]).any())
            got, base = forward(ops, c, kind, bg, c["feat"], rand), forward(ops, clean, kind, bg, clean["feat"], rand)
            tag = (where, value, step, kind, bg)
            for k, g, cl in (("alpha", got[1], base[1]), ("weights", got[2], base[2])):
                assert torch.equal(torch.isnan(g[:, NF_RAY]), pat[k][:, NF_RAY]), (tag, k, "NaN pattern")
                assert bool(torch.isfinite(g[:, NF_RAY][~pat[k][:, NF_RAY]]).all()), (tag, k, "not finite where the reference is")
                assert torch.equal(g[:, others], cl[:, others]), (tag, k, "another ray changed")
            assert bool(torch.isnan(got[0][NF_RAY]).all()) == pat_out and (pat_out or bool(torch.isfinite(got[0][NF_RAY]).all())), (tag, "out")
            assert torch.equal(got[0][others], base[0][others]), (tag, "out of another ray changed")
            if value == "nan":
                assert pat_out, (tag, "the reference's pixel is NaN")
            if where == "density" and value != "nan" and kind == "softplus":   # a finite result must be the RIGHT one: opaque / empty
                assert float(got[1][step, NF_RAY]) == (1.0 if value == "+inf" else 0.0), tag
            for form in FORMS_OF(NF_T):
                gd, gf = backward(ops, c, kind, bg, c["feat"], rand, g_out, form)
                cd, cf = backward(ops, clean, kind, bg, clean["feat"], rand, g_out, form)
                assert torch.equal(gd[:, others], cd[:, others]) and torch.equal(gf[:, others], cf[:, others]), (tag, form, "another ray's gradient changed")
                # (an infinite FIRST step only makes interval 0 negative, i.e. 1e-5 long: nothing is non-finite, in the reference either)
                if pat_out or (where == "step" and step > 0):
                    assert not bool(torch.isfinite(gd[:, NF_RAY]).all()), (tag, form, "g_density of the poisoned ray is finite")
                if pat_out:
                    assert not bool(torch.isfinite(gf[:, NF_RAY]).all()), (tag, form, "g_feat of the poisoned ray is finite")


# ------------------------------------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("T", [16, 100, 192, 300])
def test_backward_is_bitwise_reproducible(ops, T):
    R = 1000
    d = _t(proc_uniform((T, R), 6700 + T, 6.0)).cuda()
    feat = CR._colours(T, R, 6701).cuda()
    rows = torch.sort(2.0 + 4.0 * torch.rand(R, T, generator=torch.Generator().manual_seed(T)), dim=1).values.cuda()
    rays = torch.cat([torch.zeros(R, 3), CR._dirs(R, 6702)], -1).cuda()
    g_out = _t(proc_uniform((R, 3), 6703, 1.0)).cuda()
    rand = _t(0.5 + 0.5 * proc_uniform((R, 1), 6704, 1.0)).cuda()
    for form in FORMS_OF(T):
        a = ops.composite_rayts_backward(d, feat, rows, rays, g_out, True, "random", rand, form=form)
        torch.empty(T * R * 5, device="cuda").fill_(-7.0)          # (what a recycled allocation would hold)
        b = ops.composite_rayts_backward(d, feat, rows, rays, g_out, True, "random", rand, form=form)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (T, form)
        assert bool(torch.isfinite(a[0]).all()) and bool(torch.isfinite(a[1]).all())
