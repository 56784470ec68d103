"""CPU checks of tests/composite_ref.py: the fp64 reference against the oracle (values and autograd), the fp32 emulation of the
layer-synchronous order inside the derived bounds on every shared input, the steerable weights through the fp64 oracle, and the
reference's own non-finite pattern that tests/test_gpu_composite.py expects of the kernels."""
import math

import pytest
import torch

import composite_ref as CR
import oracle as O

BGS = ("black", "white", "random")


def close(a, b, rtol=1e-13, atol=1e-300):
    return bool(((a - b).abs() <= rtol * b.abs() + atol).all())


@pytest.mark.parametrize("name", ["A1", "A2", "A33", "B", "C", "D", "F", "G0.001", "G0.1", "G1.5"])
def test_reference_equals_the_oracle_in_fp64(name):
    c = CR.case(name)
    rand = CR.rand_of(c)
    for bg in BGS:
        for kind in ((c["kind"],) if c["kind"] == "laplace" else ("softplus", "relu")):
            ref = CR.reference(c, kind, bg, rand)
            alpha, weights, out, sky = CR.oracle_forward(c["density"].double(), c["feat"].double(), c["ts"].double(), c["dirs"].double(),
                                                         kind, bg, rand.double(), c.get("beta"))
            assert close(ref["alpha"], alpha) and close(ref["weights"], weights), (name, bg, kind)
            assert close(ref["out"], out, atol=1e-15) and close(ref["sky"], sky, atol=1e-15), (name, bg, kind)   # (1 - sum: cancellation)


@pytest.mark.parametrize("name", ["A2", "A33", "B17", "C", "D"])
def test_reference_gradients_equal_the_oracles_autograd(name):
    c = CR.case(name)
    T, R = c["density"].shape
    rand = CR.rand_of(c)
    g_out = torch.from_numpy(CR.proc_uniform((R, 3), 7000, 1.0))
    for bg in BGS:
        for kind in ("softplus", "relu"):
            gd, gf = CR.composite_grads(c["density"], c["feat"], c["ts"], c["dirs"], g_out, kind, bg, rand)
            d = c["density"].double().requires_grad_(True)
            f = c["feat"].double().requires_grad_(True)
            _, _, out, _ = CR.oracle_forward(d, f, c["ts"].double(), c["dirs"].double(), kind, bg, rand.double())
            (out * g_out.double()).sum().backward()
            assert close(gd, d.grad, 1e-11) and close(gf, f.grad, 1e-11), (name, bg, kind)
            assert bool(torch.isfinite(gd).all())


def test_alpha_bound_is_the_closed_form_of_the_issue():
    """|da| <= (eps_sigma + 6u) / e + EPS_EXP + u, since x e^-x <= 1 / e"""
    c = CR.case("A65")
    eps = CR.eps_sigma_of(c["density"], "softplus")
    b = CR.forward_bounds(CR.reference(c), eps, c["feat"])["alpha"]
    assert bool((b <= (eps + 6 * CR.U) / math.e + CR.EPS_EXP + CR.U + 2 * CR.TINY).all())
    assert float(b.max()) < 1.2e-6


@pytest.mark.parametrize("name", CR.CASES)
def test_layer_synchronous_association_stays_inside_the_bounds(name):
    """block scan, block product and carry in fp32 (libm: at most EPS_SOFTPLUS / EPS_EXP) on every input the GPU tests use"""
    c = CR.case(name)
    if name == "E160x1517":   # (the emulation walks the rays in Python: the first 140 rays hold every wall position of the input)
        c = {k: (v[:, :140] if k in ("density", "feat") else v[:140] if k == "dirs" else v) for k, v in c.items()}
    for bg in ("black", "white"):
        ref = CR.reference(c, bg=bg)
        b = CR.forward_bounds(ref, CR.eps_sigma_of(c["density"], c["kind"], c.get("beta")), c["feat"], bg=bg)
        alpha, weights, out = CR.emulate_ls(c["density"], c["feat"], c["ts"], c["dirs"], c["kind"], bg, c.get("beta"))
        r = [CR.worst_ratio(alpha, ref["alpha"], b["alpha"]), CR.worst_ratio(weights, ref["weights"], b["weights"]),
             CR.worst_ratio(out, ref["out"], b["out"])]
        print(f"\n[emulation {name} {bg}] worst error / bound: alpha {r[0]:.3f} weights {r[1]:.3f} out {r[2]:.3f}")
        assert max(r) <= 1.0, (name, bg, r)


def test_inputs_are_what_their_names_say():
    b = CR.reference(CR.case("B"))
    walls = CR.wall_steps(67)
    for i, s in enumerate(walls):
        assert float(b["alpha"].float()[s, i]) == 1.0 and float(b["alpha"][:s, i].max() if s else 0.0) < 1e-16
    c = CR.reference(CR.case("C"))["alpha"][-1]
    assert float(c.min()) > 2e-7 and float(c.max()) == 1.0 and int(((c > 1e-3) & (c < 0.999)).sum()) >= 15
    assert float(CR.reference(CR.case("C"))["alpha"][:-1].max()) < 1e-15
    d = CR.reference(CR.case("D"))["P"]
    assert float(d[-1].min()) < 1e-45 and float(d[-1].max()) > 0
    f = CR.case("F")
    gaps = (f["ts"][:, 1:] - f["ts"][:, :-1])
    assert int((gaps == 0).sum()) == 4 and int(((gaps > 0) & (gaps < 1e-5)).sum()) == 8 and int(((gaps > 1e-5) & (gaps < 1.2e-5)).sum()) == 4
    e = CR.case("E160x1517")
    assert int((e["density"] == 22).sum()) == 1517 and len(set((e["density"] == 22).float().argmax(0).tolist())) == 10
    assert len(CR.E_SIZES) == 12


def _sig_bits_ok(t, bits=8):
    m, _ = torch.frexp(t.double())
    return bool(((m * 2 ** bits) == (m * 2 ** bits).round()).all())


@pytest.mark.parametrize("model", ["plain", "tiny"])
def test_steerable_weights_dictate_the_logits_exactly(model):
    """the fp64 oracle forward returns the dictated logits bit for bit; every intermediate of the positive path fits 8 bits"""
    for name in ("A33", "B", "C"):
        c = CR.case(name, grid=True)
        pts = CR.steer_pts(c, tiny=(model == "tiny")).double()
        p = {k: v.double() for k, v in (CR.steer_tiny() if model == "tiny" else CR.steer_plain()).items()}
        collect = []
        if model == "tiny":
            y = O.skip_mlp(p, "estim.", pts, collect=collect)
            assert torch.equal(y[..., 1:], torch.tensor(CR.COLOUR_LOGITS, dtype=torch.float64).expand_as(y[..., 1:]))
        else:
            y = O.skip_mlp(p, "first.", pts, None, enc=lambda v: O.hash_encode(v, [p[f"first.enc.embs.{i}.weight"] for i in range(8)]), collect=collect)
            assert torch.equal(y[..., 1:], torch.zeros_like(y[..., 1:]))
            rgb = O.skip_mlp(p, "refl.mlp.", torch.zeros(4, 5, dtype=torch.float64), torch.zeros(4, 64, dtype=torch.float64), act="sin")
            assert torch.equal(rgb, torch.tensor(CR.COLOUR_LOGITS, dtype=torch.float64).expand_as(rgb))
        assert torch.equal(y[..., 0], c["density"].double()), (model, name)
        for h in collect:
            assert float(h.min()) >= 0 and float(h.max()) <= 63.5 and _sig_bits_ok(h), (model, name)
        assert _sig_bits_ok(y)
    assert len(set(CR.COLOUR_LOGITS)) == 3


def h_expected(value, step, T=CR.H_T):
    """what a non-finite logit does in the reference (stated here, checked below against its fp32 forward): NaN poisons the sample's
    alpha, every weight from it on and the pixel; softplus(+inf) = inf is an opaque sample, softplus(-inf) = 0 an empty one"""
    t = torch.arange(T)
    if value == "nan":
        return dict(alpha=(t == step), weights=(t >= step), out=True)
    return dict(alpha=torch.zeros(T, dtype=torch.bool), weights=torch.zeros(T, dtype=torch.bool), out=False)


@pytest.mark.parametrize("value", list(CR.H_VALUES))
@pytest.mark.parametrize("step", CR.H_STEPS)
def test_non_finite_pattern_of_the_reference(value, step):
    pat = CR.h_pattern(value, step)
    want = h_expected(value, step)
    assert torch.equal(pat["alpha"][:, CR.H_RAY], want["alpha"]) and torch.equal(pat["weights"][:, CR.H_RAY], want["weights"])
    assert bool(pat["out"][CR.H_RAY].all()) == want["out"] and bool(pat["out"][CR.H_RAY].any()) == want["out"]
    others = torch.arange(pat["out"].shape[0]) != CR.H_RAY   # no other ray is touched
    assert not bool(pat["alpha"][:, others].any()) and not bool(pat["weights"][:, others].any()) and not bool(pat["out"][others].any())
    if value != "nan":
        ref = CR.composite_ref(**CR.h_args(value, step))
        assert float(ref["alpha"][step, CR.H_RAY]) == (1.0 if value == "+inf" else 0.0)


@pytest.mark.parametrize("value", list(CR.H_VALUES))
@pytest.mark.parametrize("step", CR.H_STEPS)
def test_non_finite_position_pattern_of_the_reference_tiny_nerf(value, step):
    """a non-finite p_x in the steered TinyNeRF: NaN in the logit AND the colours of that sample for all three values"""
    pat = CR.tiny_h_pattern(value, step)
    want = h_expected("nan", step)
    assert torch.equal(pat["alpha"][:, CR.H_RAY], want["alpha"]) and torch.equal(pat["weights"][:, CR.H_RAY], want["weights"])
    others = torch.arange(pat["out"].shape[0]) != CR.H_RAY
    assert bool(pat["out"][CR.H_RAY]) and not bool(pat["out"][others].any()) and not bool(pat["weights"][:, others].any())


def test_worst_ratio_is_never_nan():
    ref, b = torch.zeros(3, dtype=torch.float64), torch.full((3,), 1e-6, dtype=torch.float64)
    assert CR.worst_ratio(torch.tensor([0.0, float("nan"), 0.0]), ref, b) == float("inf")
    assert CR.worst_ratio(torch.tensor([0.0, float("inf"), 0.0]), ref, b) == float("inf")
    assert CR.worst_ratio(torch.tensor([0.0, 5e-7, 0.0], dtype=torch.float64), ref, b) == 0.5
