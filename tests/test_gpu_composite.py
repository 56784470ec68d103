"""Alpha compositing at its edges in every kernel that composites, against the fp64 reference and the derived per-element bounds
of tests/composite_ref.py: the standalone forward (csrc/basic_ops.hip), both backward kernels (csrc/backward.hip), the
layer-synchronous composite / combine pair (csrc/ls_kernel.h) behind steerable weights in na_render_view_ls, na_render_tiny_ls,
na_render_plain_view_ls(_rayts), and the register engine (csrc/render_fused.hip).  Non-finite logits must stay loud.

Worst error / bound measured on the MI355X when these tests were written (alpha, weights, out; the tests print them):
  input   na_composite     view_ls = tiny_ls = plain_view_ls   register engine   other
  A       .44 .44 .47      .44 .44 .13                         .44 .44 .13
  B       .12 .00 .00      .12 .00 .01                         .12 .00 .01
  C       .43 .18 .01      .43 .18 .01                         .43 .18 .01
  D       .49 .48 .03      .49 .48 .02                         .47 .47 .02
  E       .21 .21 .06      .21 .21 .03                         .21 .21 .03
  F       .19 .19 .02      .17 .17 .01                         .17 .17 .01       plain_view_ls_rayts .19 .19 .03
  G       .30 .15 .07      view_ls (sdf mode) .30 .15 .04
(the three layer-synchronous renderers agree to the last digit in every precision: their alpha is bit-identical, the colours are
the same constants); backward (g_density, g_feat), the kernel picked by T and the sequential one alike to three digits:
A .14 .45, B .03 .00, C .11 .28, D .19 .48, G .04 .21."""
import os
import subprocess
import sys

import pytest
import torch

import composite_ref as CR

pytestmark = pytest.mark.gpu

LS_PRECS = ("bf16x3", "f16x", "f16", "bf16")
REG_PRECS = ("bf16x3", "bf16")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def rays_split(c):
    """the input as a list of (columns, ts) launches: one for shared steps, one per ray for per-ray steps"""
    if c["ts"].dim() == 1:
        return [(slice(None), c["ts"])]
    return [(slice(r, r + 1), c["ts"][r]) for r in range(c["ts"].shape[0])]


def check(tag, got, ref, bound, worst):
    r = CR.worst_ratio(got, ref, bound)
    worst[tag] = max(worst.get(tag, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------------ standalone forward
def standalone(ops, c, density, softplus, bg, C, rand, want=True):
    outs, alphas, weights = [], [], []
    feat = c["feat"][..., :C].contiguous()
    rays = CR.rays_of(c)
    for cols, ts in rays_split(c):
        o, a, w = ops.composite(density[:, cols].contiguous().cuda(), feat[:, cols].contiguous().cuda(), ts.cuda(), rays[cols].contiguous().cuda(),
                                softplus, bg, want, None if rand is None else rand[cols].contiguous().cuda())
        outs.append(o.cpu())
        alphas.append(None if a is None else a.cpu())
        weights.append(None if w is None else w.cpu())
    if not want:
        return torch.cat(outs), None, None
    return torch.cat(outs), torch.cat(alphas, dim=1), torch.cat(weights, dim=1)


@pytest.mark.parametrize("name", CR.CASES)
def test_standalone_forward_meets_the_bounds(ops, name):
    """na_composite / na_composite_random_bg / na_sky_random / na_integrate: alpha, weights, out per element inside the bounds for
    both density kinds (the Laplace density of input G through na_laplace_density), three backgrounds, C = 1 and 3; without alpha /
    weights the same out bit for bit; the weights in front of the closing interval and the sky sum to one."""
    c = CR.case(name)
    T, R = c["density"].shape
    rand = CR.rand_of(c)
    kinds = ("laplace",) if c["kind"] == "laplace" else ("softplus", "relu")
    worst = {}
    for kind in kinds:
        if kind == "laplace":
            density = ops.laplace_density(c["density"].cuda(), torch.tensor([c["beta"]], device="cuda")).cpu()
        else:
            density = c["density"]
        eps = CR.eps_sigma_of(c["density"], kind, c.get("beta"))
        for C in (3, 1):
            feat = c["feat"][..., :C].contiguous()
            for bg in ("black", "white", "random"):
                ref = CR.reference(c, kind, bg, rand, feat)
                b = CR.forward_bounds(ref, eps, feat, bg=bg, rand=rand)
                out, alpha, weights = standalone(ops, c, density, kind == "softplus", bg, C, rand if bg == "random" else None)
                ra = check(f"{kind} alpha", alpha, ref["alpha"], b["alpha"], worst)
                rw = check(f"{kind} weights", weights, ref["weights"], b["weights"], worst)
                ro = check(f"{kind} out", out, ref["out"], b["out"], worst)
                assert all(v <= 1.0 for v in (ra, rw, ro)), (name, kind, C, bg, ra, rw, ro)
                bare, _, _ = standalone(ops, c, density, kind == "softplus", bg, C, rand if bg == "random" else None, want=False)
                assert torch.equal(bare, out), (name, kind, C, bg)
                if bg == "black":
                    keep = (out, weights)
                if bg == "random" and c["ts"].dim() == 1:   # the same sky from the kept weights, behind the black-background out
                    late = ops.sky_random(keep[1].cuda(), rand.cuda(), keep[0].clone().cuda()).cpu()
                    rs = check(f"{kind} sky_random", late, ref["out"], b["out"] + CR.U * ref["out"].abs(), worst)
                    assert rs <= 1.0, (name, kind, C, rs)
                if bg == "white" and C == 1:
                    # out = sum w c + sky with c := 0 is the sky itself: sum_{t<T-1} w_t + sky = 1 to the roundings of the kernel's own sum
                    zero = dict(c, feat=torch.zeros_like(c["feat"]))
                    sky, _, w = standalone(ops, zero, density, kind == "softplus", "white", 1, None)
                    head = w[:-1].double().sum(0).unsqueeze(-1)
                    slack = (T + 1) * CR.U * head + CR.U * sky.double().abs() + CR.TINY
                    rs = CR.worst_ratio(head + sky.double(), torch.ones_like(head), slack)
                    worst[f"{kind} sum-to-one"] = max(worst.get(f"{kind} sum-to-one", 0.0), rs)
                    assert rs <= 1.0, (name, kind, rs)
                    assert CR.worst_ratio(sky, ref["sky"], b["sky"] + CR.U * ref["sky"].abs()) <= 1.0
            if c["ts"].dim() == 1:   # na_integrate on the kernel's own weights: any order of T products and sums
                w32 = keep[1]
                got = ops.integrate(w32.cuda(), feat.cuda()).cpu()
                exact = (w32.double()[..., None] * feat.double()).sum(0)
                mag = (w32.double().abs()[..., None] * feat.double().abs()).sum(0)
                ri = check(f"{kind} integrate", got, exact, (T + 1) * CR.U * mag + CR.TINY * T, worst)
                assert ri <= 1.0, (name, kind, C, ri)
    print(f"\n[composite {name}] worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------- backward
BWD_CASES = tuple(f"A{T}" for T in CR.A_SIZES) + ("B16", "B17", "B67", "B128", "B129", "C", "D", "D129") + tuple(f"G{b}" for b in CR.G_BETAS)


def bwd_input(name):
    """(input, kind): input G reaches the backward as the relu of its Laplace density (rounded to fp32: the kernel's input)"""
    c = CR.case(name)
    if c["kind"] == "laplace":
        c = dict(c, density=CR.sigma_of(c["density"].double(), "laplace", c["beta"]).float(), kind="relu")
    return c, c["kind"]


def bwd_variants(name):
    return (("black", 3), ("white", 3), ("random", 3), ("white", 1)) if name in ("A33", "B17", "B129") else (("white", 3), ("random", 3))


def g_out_of(c, C):
    return torch.from_numpy(CR.proc_uniform((c["density"].shape[1], C), 7100, 1.0))


def backward_all():
    """{(name, bg, C): (g_density, g_feat)} of the kernel this process selects (NA_COMPOSITE_BWD is read once per process)"""
    from nerf_atlas_amd import ops
    res = {}
    for name in BWD_CASES:
        c, kind = bwd_input(name)
        rand = CR.rand_of(c)
        for bg, C in bwd_variants(name):
            gd, gf = ops.composite_backward(c["density"].cuda(), c["feat"][..., :C].contiguous().cuda(), c["ts"].cuda(), CR.rays_of(c).cuda(),
                                            g_out_of(c, C).cuda(), kind == "softplus", bg, rand.cuda() if bg == "random" else None)
            res[(name, bg, C)] = (gd.cpu(), gf.cpu())
    return res


def check_backward(res, tag):
    for name in BWD_CASES:
        c, kind = bwd_input(name)
        rand = CR.rand_of(c)
        eps = CR.eps_sigma_of(c["density"], kind, libm=True)
        worst = [0.0, 0.0]
        for bg, C in bwd_variants(name):
            feat = c["feat"][..., :C].contiguous()
            g_out = g_out_of(c, C)
            gd, gf = res[(name, bg, C)]
            assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(gf).all()), (tag, name, bg, C)
            rd, rf = CR.composite_grads(c["density"], feat, c["ts"], c["dirs"], g_out, kind, bg, rand)
            ref = CR.reference(c, kind, bg, rand, feat)
            b_d, b_f = CR.backward_bounds(ref, eps, c["density"], feat, g_out, kind, bg, rand)
            r = (CR.worst_ratio(gd, rd, b_d), CR.worst_ratio(gf, rf, b_f))
            worst = [max(worst[0], r[0]), max(worst[1], r[1])]
            assert all(v <= 1.0 for v in r), (tag, name, bg, C, r)
        print(f"\n[composite backward {tag} {name}] worst error / bound: g_density {worst[0]:.3f} g_feat {worst[1]:.3f}")


def test_backward_meets_the_condition_number_bound(ops):
    """the kernel the launcher picks by T: the segmented one for 17 <= T <= 128, the sequential one for T <= 16 and T >= 129 --
    the switch-overs 16 / 17 and 128 / 129 with opaque samples on the segment edge 15 / 16 (input B); finite everywhere"""
    assert os.environ.get("NA_COMPOSITE_BWD") is None
    check_backward(backward_all(), "by T")


def test_sequential_backward_meets_the_same_bound(tmp_path):
    """NA_COMPOSITE_BWD=seq (read once per process: a child) sends every T through composite_backward_kernel"""
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "seq.pt")
    src = ("import sys, torch; sys.path[:0] = [%r, %r]; import test_gpu_composite as M; torch.save(M.backward_all(), sys.argv[1])"
           % (os.path.dirname(here), here))
    env = dict(os.environ, NA_COMPOSITE_BWD="seq")
    r = subprocess.run([sys.executable, "-c", src, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    check_backward(torch.load(out), "seq")


# ------------------------------------------------------------------------------------------ fused renderers, steered weights
THIN = "thin"


@pytest.fixture(scope="module")
def packs(ops):
    """the steered weight streams, packed once per precision"""
    plain, tiny = CR.steer_plain(), CR.steer_tiny()
    cu = lambda lists: tuple([t.cuda() for t in l] for l in lists)   # noqa: E731
    res = {"tables": torch.zeros(8, 65536, 4, device="cuda")}
    for prec in LS_PRECS:
        res["view", prec] = ops.render_view_ls_pack(prec, *cu(CR.mlp_lists(plain, "refl.mlp.")))
        res["tiny", prec] = ops.render_tiny_ls_pack(prec, *cu(CR.mlp_lists(tiny, "estim.")))
        res["plain", prec] = ops.render_ls_pack(prec, cu(CR.mlp_lists(plain, "first.")), cu(CR.mlp_lists(plain, "refl.mlp.")))
    d1 = ops.make_desc(3, "hash", 35, 0, 4, 256, 65, 3, "leaky_relu", "plain_first")
    d2 = ops.make_desc(5, "none", 0, 64, 4, 256, 3, 3, "sin", "plain_view")
    for prec in REG_PRECS:
        res["reg", prec] = (ops.mlp_pack(d1, prec, *cu(CR.mlp_lists(plain, "first."))), ops.mlp_pack(d2, prec, *cu(CR.mlp_lists(plain, "refl.mlp."))))
    return res


def fused(ops, packs, which, prec, c, bg, want=True, ld=65):
    """one steered renderer on an input (per ray when its steps are per ray) -> out [R,3], alpha, weights [T,R] on the host"""
    T = c["density"].shape[0]
    rays = CR.rays_of(c)
    outs, alphas, weights = [], [], []
    for cols, ts in rays_split(c):
        sub = {k: (v[:, cols].contiguous() if k in ("density", "feat") else v) for k, v in c.items()}
        ry, tsc = rays[cols].contiguous().cuda(), ts.cuda()
        if which == "view":
            beta = None if c["kind"] != "laplace" else torch.tensor([c["beta"]], device="cuda")
            o, a, w = ops.render_view_ls(ry, tsc, CR.view_feat(sub, ld).cuda(), beta, packs["view", prec], prec, THIN, bg, want)
        elif which == "tiny":
            o, a, w = ops.render_tiny_ls(ry, tsc, packs["tiny", prec], prec, THIN, bg, want, pts=CR.steer_pts(sub, tiny=True).cuda())
        elif which == "plain":
            o, a, w = ops.render_plain_view_ls(ry, tsc, packs["tables"], packs["plain", prec], prec, THIN, bg, want, pts=CR.steer_pts(sub).cuda())
        else:
            pf, pv = packs["reg", prec]
            o, a, w = ops.render_plain_view(ry, tsc, packs["tables"], pf, pv, prec, THIN, bg, want, pts=CR.steer_pts(sub).cuda())
        outs.append(o.cpu())
        alphas.append(None if a is None else a.cpu())
        weights.append(None if w is None else w.cpu())
    if not want:
        return torch.cat(outs), None, None
    return torch.cat(outs), torch.cat(alphas, dim=1), torch.cat(weights, dim=1)


FUSED_CASES = tuple(f"A{T}" for T in CR.A_SIZES) + ("B", "C", "D") + tuple(f"E{T}x{R}" for T, R in CR.E_SIZES) + ("F",)
RENDERERS = (("view", LS_PRECS), ("tiny", LS_PRECS), ("plain", LS_PRECS), ("reg", REG_PRECS))


def steered_reference(c, bg):
    colour = CR.colour_of(THIN)
    feat = colour.expand(c["density"].shape + (3,))
    ref = CR.reference(c, bg=bg, feat=feat)
    eps = CR.eps_sigma_of(c["density"], c["kind"], c.get("beta"))
    return ref, CR.forward_bounds(ref, eps, feat, err_c=CR.EPS_COLOUR_THIN * colour, bg=bg)


@pytest.mark.parametrize("name", FUSED_CASES + tuple(f"G{b}" for b in CR.G_BETAS))
def test_fused_renderers_meet_the_bounds_on_dictated_logits(ops, packs, name):
    """Every fused renderer, every precision it accepts, white and black: alpha, weights, out inside the bounds of the standalone
    kernel -- the logits are exact, there is no allowance for the MLP --; out bit-identical with and without alpha / weights;
    alpha bit-identical among the renderers that share csrc/ls_kernel.h (all precisions: the logits are the same numbers)."""
    c = CR.case(name, grid=True)
    sdf = c["kind"] == "laplace"
    worst = {}
    alpha0 = None
    for bg in ("white", "black"):
        ref, b = steered_reference(c, bg)
        for which, precs in ((("view", LS_PRECS),) if sdf else RENDERERS):
            for prec in precs:
                for ld in ((65, 77) if which == "view" else (65,)):
                    out, alpha, weights = fused(ops, packs, which, prec, c, bg, True, ld)
                    r = (CR.worst_ratio(alpha, ref["alpha"], b["alpha"]), CR.worst_ratio(weights, ref["weights"], b["weights"]),
                         CR.worst_ratio(out, ref["out"], b["out"]))
                    worst[which] = tuple(max(p, q) for p, q in zip(worst.get(which, (0, 0, 0)), r))
                    assert all(v <= 1.0 for v in r), (name, which, prec, bg, ld, r)
                    bare, _, _ = fused(ops, packs, which, prec, c, bg, False, ld)
                    assert torch.equal(bare, out), (name, which, prec, bg, ld, "want_weights changes out")
                    if which != "reg":
                        alpha0 = alpha if alpha0 is None else alpha0
                        assert torch.equal(alpha, alpha0), (name, which, prec, bg, "alpha differs among the layer-synchronous renderers")
    print(f"\n[fused {name}] worst error / bound (alpha, weights, out): " + ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f} {v[2]:.3f}" for k, v in worst.items()))


def test_per_ray_steps_with_ties(ops, packs):
    """na_render_plain_view_ls_rayts derives positions from the steps: rays without an x component keep p_x, hence the logit,
    constant along the ray (0: sigma = 0.31).  Input F's ties and near-ties reach the 1e-5 floor; fed shared steps the entry is
    bit-identical to na_render_plain_view_ls."""
    logit = 0.0
    c = CR.input_f(const_logit=logit)
    T, R = c["density"].shape
    rays = CR.rays_of(c)
    rays[:, 0] = logit - CR.LOGIT_BIAS
    worst = (0.0, 0.0, 0.0)
    for bg in ("white", "black"):
        ref, b = steered_reference(c, bg)
        for prec in LS_PRECS:
            out, alpha, weights = ops.render_plain_view_ls_rayts(rays.cuda(), c["ts"].cuda(), packs["tables"], packs["plain", prec], prec, THIN, bg, True)
            r = (CR.worst_ratio(alpha, ref["alpha"], b["alpha"]), CR.worst_ratio(weights, ref["weights"], b["weights"]),
                 CR.worst_ratio(out, ref["out"], b["out"]))
            worst = tuple(max(p, q) for p, q in zip(worst, r))
            assert all(v <= 1.0 for v in r), (prec, bg, r)
            bare, _, _ = ops.render_plain_view_ls_rayts(rays.cuda(), c["ts"].cuda(), packs["tables"], packs["plain", prec], prec, THIN, bg, False)
            assert torch.equal(bare, out)
    print(f"\n[fused F rayts] worst error / bound (alpha, weights, out): {worst[0]:.3f} {worst[1]:.3f} {worst[2]:.3f}")
    a = CR.case("A33")
    R = a["dirs"].shape[0]
    rays = CR.rays_of(a)
    rays[:, 3] = 0.0
    rays[:, 0] = 41.0 + torch.arange(R).float() % 13 * 0.5 - 3.0       # logits -3 .. 3 on the grid, one per ray
    for prec in LS_PRECS:
        shared = ops.render_plain_view_ls(rays.cuda(), a["ts"].cuda(), packs["tables"], packs["plain", prec], prec, THIN, "white", True)
        per_ray = ops.render_plain_view_ls_rayts(rays.cuda(), a["ts"][None].expand(R, -1).contiguous().cuda(), packs["tables"], packs["plain", prec],
                                                 prec, THIN, "white", True)
        for s, p in zip(shared, per_ray):
            assert torch.equal(s, p), prec


# ------------------------------------------------------------------------------------------------------------ non-finite
H_PRECS = ("bf16x3", "f16", "bf16")   # (f16x has a guard of its own: tests/test_gpu_range.py)


def h_check(tag, got, clean, pat, ray=CR.H_RAY):
    """NaN exactly where the reference's fp32 forward is NaN, finite elsewhere; every other ray bit-identical to the clean run"""
    out, alpha, weights = got
    others = torch.arange(out.shape[0]) != ray
    for k, g, cl in (("alpha", alpha, clean[1]), ("weights", weights, clean[2])):
        assert torch.equal(torch.isnan(g[:, ray]), pat[k][:, ray]), (tag, k, "NaN pattern", torch.isnan(g[:, ray]).nonzero().flatten().tolist())
        assert bool(torch.isfinite(g[:, ray][~pat[k][:, ray]]).all()), (tag, k, "not finite where the reference is")
        assert torch.equal(g[:, others], cl[:, others]), (tag, k, "another ray changed")
    assert bool(torch.isnan(out[ray]).all()) == bool(pat["out"][ray]) and bool(torch.isnan(out[ray]).any()) == bool(pat["out"][ray]), (tag, "out")
    assert bool(pat["out"][ray]) or bool(torch.isfinite(out[ray]).all()), (tag, "out not finite")
    assert torch.equal(out[others], clean[0][others]), (tag, "out of another ray changed")


@pytest.mark.parametrize("value", list(CR.H_VALUES))
@pytest.mark.parametrize("step", CR.H_STEPS)
def test_non_finite_logits_stay_loud(ops, packs, value, step):
    """One NaN / +Inf / -Inf logit in one ray of input A (T = 65), at the first step, either side of the block boundary or the
    closing interval: na_composite and na_render_view_ls take the logit itself and must do what the reference does (NaN poisons the
    ray from that step on; +Inf is an opaque, -Inf an empty sample: both finite and exactly 1 / 0).
    Before csrc/common.h fast_exp kept NaN and clamped from below, NaN came out as a finite, nearly opaque sample (fminf(NaN, 88) = 88),
    +Inf as NaN (fma(-inf, c, +inf)) and -Inf as alpha = -1.65e38; in na_render_view_ls the relu behind fast_softplus(NaN) (fmaxf(NaN, 0) = 0)
    then still made the NaN logit an empty sample."""
    c = CR.input_h(value, step)
    clean = CR.case(f"A{CR.H_T}")
    pat = CR.h_pattern(value, step)
    if value != "nan":   # a finite result must also be the RIGHT one: the reference's alpha at the bad sample is exactly 1 / 0
        want_alpha = 1.0 if value == "+inf" else 0.0
    for bg in ("white", "black"):
        got = standalone(ops, c, c["density"], True, bg, 3, None)
        h_check(f"composite {value}@{step} {bg}", got, standalone(ops, clean, clean["density"], True, bg, 3, None), pat)
        if value != "nan":
            assert float(got[1][step, CR.H_RAY]) == want_alpha
        for prec in H_PRECS:
            got = fused(ops, packs, "view", prec, c, bg)
            h_check(f"view_ls {prec} {value}@{step} {bg}", got, fused(ops, packs, "view", prec, clean, bg), pat)
            if value != "nan":
                assert float(got[1][step, CR.H_RAY]) == want_alpha


@pytest.mark.parametrize("value", list(CR.H_VALUES))
@pytest.mark.parametrize("step", CR.H_STEPS)
def test_non_finite_positions_stay_loud_in_tiny_ls(ops, packs, value, step):
    """Input H through the steerable weights of na_render_tiny_ls: p_x of one sample is NaN / +Inf / -Inf.  The reference's fp32
    TinyNeRF makes all three a NaN logit and NaN colours at that sample (0 x Inf in the units with zero weights): alpha NaN there,
    weights NaN from there on, a NaN pixel; every other ray keeps its bits.
    The LeakyReLU of csrc/mlp_engine.h was a bare median of three, which returns its finite bound (3e38; 65504 in f16) for NaN: the
    sample came out finite and opaque, the pixel white.  act_apply now keeps NaN, and the half clamp of NA_PREC_F16 lets NaN / Inf by."""
    c, pts = CR.tiny_h_pts(value, step)
    pat = CR.tiny_h_pattern(value, step)
    rays, ts = CR.rays_of(c).cuda(), c["ts"].cuda()
    clean_pts = CR.steer_pts(c, tiny=True).cuda()
    for prec in H_PRECS:
        for bg in ("white", "black"):
            got = [t.cpu() for t in ops.render_tiny_ls(rays, ts, packs["tiny", prec], prec, THIN, bg, True, pts=pts.cuda())]
            base = [t.cpu() for t in ops.render_tiny_ls(rays, ts, packs["tiny", prec], prec, THIN, bg, True, pts=clean_pts)]
            h_check(f"tiny_ls {prec} {value}@{step} {bg}", got, base, pat)


@pytest.mark.parametrize("step", (0, 31, 32))
def test_non_finite_relu_and_sdf_densities_stay_loud(ops, packs, step):
    """The other two density kinds: a NaN density of na_composite(softplus = False) (fmaxf(NaN, 0) used to make it an empty sample), a
    NaN signed distance through na_laplace_density and through the sdf mode of na_render_view_ls (fminf / fmaxf inside the Laplace
    cdf used to make it the finite density 0.5 / beta).  Reference: relu(NaN) = NaN, laplace_cdf(NaN) = NaN."""
    ray = 5
    clean = CR.case("G0.1")
    sdf = clean["density"].clone()
    sdf[step, ray] = float("nan")
    c = dict(clean, density=sdf)
    ref = CR.composite_ref(c["density"], c["feat"], c["ts"], c["dirs"], "laplace", "white", None, c["beta"])
    pat = dict(alpha=torch.isnan(ref["alpha"]), weights=torch.isnan(ref["weights"]), out=torch.isnan(ref["out"]).any(-1))
    assert int(pat["alpha"].sum()) == 1 and int(pat["out"].sum()) == 1
    beta = torch.tensor([c["beta"]], device="cuda")
    dens, dens_clean = ops.laplace_density(sdf.cuda(), beta).cpu(), ops.laplace_density(clean["density"].cuda(), beta).cpu()
    assert torch.equal(torch.isnan(dens), torch.isnan(sdf)) and torch.equal(dens[~torch.isnan(sdf)], dens_clean[~torch.isnan(sdf)])
    for bg in ("white", "black"):
        h_check(f"composite relu nan@{step} {bg}", standalone(ops, c, dens, False, bg, 3, None), standalone(ops, clean, dens_clean, False, bg, 3, None), pat, ray)
        for prec in H_PRECS:
            h_check(f"view_ls sdf {prec} nan@{step} {bg}", fused(ops, packs, "view", prec, c, bg), fused(ops, packs, "view", prec, clean, bg), pat, ray)


@pytest.mark.parametrize("value", ("nan", "+inf"))
def test_non_finite_ray_direction_stays_loud_in_tiny_ls(ops, packs, value):
    """What the compositing of na_render_tiny_ls reads per ray besides the logits is the direction: one non-finite component makes
    |d|, hence every interval of that ray, NaN or Inf.  NaN must poison the whole ray (1 - fast_exp(NaN) used to be -1.65e38), Inf
    makes every sample opaque (fast_exp(-inf) used to be NaN); the other rays keep their bits."""
    clean = CR.case(f"A{CR.H_T}", grid=True)
    dirs = clean["dirs"].clone()
    dirs[CR.H_RAY, 1] = CR.H_VALUES[value]
    c = dict(clean, dirs=dirs)
    colour = CR.colour_of(THIN).float()
    ref = CR.composite_ref(c["density"], colour.expand(c["density"].shape + (3,)), c["ts"], c["dirs"], "softplus", "white")
    pat = dict(alpha=torch.isnan(ref["alpha"]), weights=torch.isnan(ref["weights"]), out=torch.isnan(ref["out"]).any(-1))
    assert bool(pat["alpha"][:, CR.H_RAY].all()) == (value == "nan") and not bool(pat["alpha"][:, torch.arange(dirs.shape[0]) != CR.H_RAY].any())
    for prec in H_PRECS:
        for bg in ("white", "black"):
            got = fused(ops, packs, "tiny", prec, c, bg)
            h_check(f"tiny_ls {prec} {value} direction {bg}", got, fused(ops, packs, "tiny", prec, clean, bg), pat)
            if value != "nan":
                assert torch.equal(got[1][:, CR.H_RAY], torch.ones(CR.H_T))
