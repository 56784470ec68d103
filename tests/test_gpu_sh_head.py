"""GPU parity of the spherical-harmonic colour head (`--refl-kind sph-har`; csrc/sh_head.hip, refl.SphericalHarmonic) with the reference
(src/refl.py:696-731, src/spherical_harmonics.py:55-106).  Expected values are fixtures recorded from the reference itself on the CPU
(tools/gen_golden.py g20, tools/ref_train_fixture.py nerf_sh), in fp32 AND fp64:

  * ops.sh_shade / autograd.ShShadeFn per entry within 4x the reference's own fp32-vs-fp64 deviation on that entry (floor 2e-6: another
    but equally valid fp32 summation order);
  * PlainNeRF + sph-har, orders 0..4: RGB, alpha and weights within 1e-4 of the FP64 values (the project's bar for every head; the
    reference's own fp32 run spends up to 3.3e-5 of it), on both routes of the head;
  * the hoisted route is the one inference takes (one sh_view_terms per forward, seven row Linears over <= 128 + 64 columns, no
    per-sample view features), the plain route the one gradients take; both agree on ragged shapes, explicit points, refl_latent columns;
  * whole-model gradients and the `make nerf-sh` training recipe at the bars of tests/test_gpu_backward.py / tests/test_gpu_train.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, golden_params

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from oracle.procedural import proc_param, proc_uniform  # noqa: E402
from tools.make_scene import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
E2E_TOL = {"fp32": 1.0, "bf16x3": 40.0}  # (tests/test_gpu_backward.py: x 1e-6 on the loss)


@pytest.fixture()
def na():
    assert torch.cuda.is_available()
    import nerf_atlas_amd.nerf as nerf
    import nerf_atlas_amd.refl as refl
    from nerf_atlas_amd import autograd, config, ops, utils

    class NS:
        pass
    ns = NS()
    ns.nerf, ns.refl, ns.config, ns.ops, ns.utils, ns.ag = nerf, refl, config, ops, utils, autograd
    keep, keep_t = config.precision, config.train_precision
    yield ns
    config.set_precision(keep)
    config.set_train_precision(keep_t)


def maxdiff(a, b):
    return float((a.detach().double().cpu() - torch.as_tensor(b).double()).abs().max())


def build(na, order, act="upshifted", bg="black", steps=16, near=2.0, far=6.0, n_rl=0):
    m = na.nerf.PlainNeRF(steps=steps, t_near=near, t_far=far, intermediate_size=64, sigmoid_kind=act, bg=bg)
    m.set_refl(na.refl.refl_kinds["sph-har"](latent_size=64 + n_rl, act=act, out_features=3, order=order))
    return m.cuda().eval()


def from_golden(na, h):
    m = build(na, int(h["order"]), str(h["act"]), str(h["bg"]), int(h["steps"]), float(h["near"]), float(h["far"]))
    sd = m.state_dict()
    params = golden_params(h)
    assert set(params) <= set(sd)
    for k, v in params.items():
        sd[k].copy_(v)
    return m


def procedural_(m):
    """the goldens' recipe for any model: oracle/procedural.py values, Fourier bases at the reference's sigma 32"""
    with torch.no_grad():
        for k, v in m.state_dict().items():
            if v.numel() and v.dtype == torch.float32 and not k.endswith("primes"):
                t = torch.from_numpy(proc_param(k, tuple(v.shape)))
                v.copy_(t * 32.0 if k.endswith("basis") else t)


class Spy:
    """counts the calls of nerf_atlas_amd.ops.<name> and keeps the shapes of their tensor arguments"""

    def __init__(self, monkeypatch, ops, names):
        self.calls = {n: [] for n in names}
        for n in names:
            monkeypatch.setattr(ops, n, self._wrap(getattr(ops, n), n))

    def _wrap(self, fn, name):
        def wrapped(*a, **k):
            self.calls[name].append([tuple(t.shape) for t in list(a) + list(k.values()) if torch.is_tensor(t)])
            return fn(*a, **k)
        return wrapped

    def n(self, name):
        return len(self.calls[name])


ROUTE_OPS = ["sh_view_terms", "linear_f32_rows", "linear_f32", "sh_shade", "fourier_encode", "view_elaz"]


# ------------------------------------------------------------------------------------------------ the expansion kernels
def _bar(ref32, ref64):
    """per entry: 4x the reference's own fp32-vs-fp64 deviation, floor 2e-6"""
    return (4.0 * (ref32.double() - ref64).abs()).clamp_min(2e-6)


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_sh_shade_against_the_reference_in_fp64(na, deg):
    h = load_golden("g20_sh_eval")
    kinds = h["kinds"].tolist()
    assert sorted(kinds) == sorted(na.ops.SIGMOID), "every kind of ops.SIGMOID is recorded"
    K = (deg + 1) ** 2
    dirs = h["dirs"].cuda()
    n = dirs.shape[0]
    co = torch.from_numpy(proc_uniform((n, 3 * K), int(h[f"coeffs_seed{deg}"]), 1.0)).float().cuda()
    wide = torch.zeros(n, 3 * K + 5, device="cuda")
    wide[:, 2:2 + 3 * K] = co
    worst = 0.0
    for i, kind in enumerate(kinds):
        ref32, ref64 = h[f"out32_{deg}"][i], h[f"out64_{deg}"][i]
        bar = _bar(ref32, ref64)
        with torch.no_grad():
            got = na.ops.sh_shade(co, dirs, deg, kind)
            got_p, pre = na.ops.sh_shade(wide[:, 2:2 + 3 * K], dirs, deg, kind, want_pre=True)  # coefficients passed by row pitch
        err = (got.double().cpu() - ref64).abs()
        print(f"[sh_shade deg {deg} {kind}] max |err| {float(err.max()):.2e} (reference fp32: {float((ref32.double() - ref64).abs().max()):.2e}), "
              f"worst err / bar {float((err / bar).max()):.3f}")
        worst = max(worst, float((err / bar).max()))
        assert bool((err <= bar).all()), (kind, float((err / bar).max()))
        assert torch.equal(got, got_p)
        if kind == "identity":
            assert torch.equal(pre, got)
    print(f"[sh_shade deg {deg}] worst err / bar over all kinds {worst:.3f}")
    # rows sample-major with one direction per RAY: row n takes ray n % R
    with torch.no_grad():
        R = 64
        rep = na.ops.sh_shade(co[:4 * R].reshape(4, R, 3 * K), dirs[:R], deg, "thin")
        for t in range(4):
            assert torch.equal(rep[t], na.ops.sh_shade(co[t * R:(t + 1) * R], dirs[:R], deg, "thin"))


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_sh_shade_gradient_against_the_reference_in_fp64(na, deg):
    h = load_golden("g20_sh_eval")
    K, rows = (deg + 1) ** 2, int(h["grad_rows"])
    dirs = h["dirs"][:rows].cuda()
    n = h["dirs"].shape[0]
    co = torch.from_numpy(proc_uniform((n, 3 * K), int(h[f"coeffs_seed{deg}"]), 1.0)).float()[:rows]
    probe = torch.from_numpy(proc_uniform((n, 3), int(h[f"probe_seed{deg}"]), 1.0)).float()[:rows].cuda()
    for i, kind in enumerate(h["kinds"].tolist()):
        c = co.clone().cuda().requires_grad_()
        out = na.ag.ShShadeFn.apply(c, dirs, deg, kind)
        assert out.requires_grad
        (out * probe).sum().backward()
        g32, g64 = h[f"grad32_{deg}"][i], h[f"grad64_{deg}"][i]
        err = (c.grad.double().cpu() - g64).abs()
        bar = _bar(g32, g64)
        print(f"[ShShadeFn deg {deg} {kind}] max |err| {float(err.max()):.2e}, worst err / bar {float((err / bar).max()):.3f}")
        assert bool((err <= bar).all()), (kind, float((err / bar).max()))
    d = dirs.clone().requires_grad_()
    out = na.ag.ShShadeFn.apply(co.clone().cuda().requires_grad_(), d, deg, "thin")
    with pytest.raises(NotImplementedError):  # directions carry no gradient
        out.sum().backward()


def test_sh_entry_points_reject_what_they_do_not_implement(na):
    co, d = torch.zeros(4, 27, device="cuda"), torch.ones(4, 3, device="cuda")
    with pytest.raises(NotImplementedError):
        na.ops.sh_shade(co, d, 2, "softmax")
    with pytest.raises(ValueError):
        na.ops.sh_shade(torch.zeros(4, 108, device="cuda"), d, 5, "thin")
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    rgb = torch.zeros(4, 3, device="cuda")
    assert lib.na_sh_shade(co.data_ptr(), 27, d.data_ptr(), 4, 4, 2, 99, rgb.data_ptr(), None, None) == -3  # NA_EUNSUPPORTED
    assert lib.na_sh_shade(co.data_ptr(), 27, d.data_ptr(), 4, 4, 5, 0, rgb.data_ptr(), None, None) == -1   # NA_EINVAL


# ------------------------------------------------------------------------------------------------ the per-ray kernels
def test_view_terms_and_row_linear_against_the_unhoisted_operators(na):
    """na_sh_view_terms = the view columns of the three wide Linears applied to [elaz | Fourier(elaz)] of every ray (features bit-identical
    to na_view_elaz + na_fourier_encode); na_linear_f32_rows with a per-ray bias + na_linear_f32 of the full rows agree to fp32 rounding."""
    torch.manual_seed(3)
    r = na.refl.refl_kinds["sph-har"](latent_size=64, act="upshifted", out_features=3, order=2).cuda()
    with torch.no_grad():
        for lin in (r.mlp.init, r.mlp.layers[0], r.mlp.layers[3]):
            lin.bias.uniform_(-0.5, 0.5)
    m = r.mlp
    for R, T in ((1, 3), (37, 5), (64, 1), (130, 2)):
        dirs = torch.randn(R, 3, device="cuda") * 1.3
        lat = torch.randn(T, R, 70, device="cuda")[..., 3:67]  # a column slice: row pitch 70
        with torch.no_grad():
            f = torch.cat([na.ops.view_elaz(dirs), na.ops.fourier_encode(na.ops.view_elaz(dirs), m.enc.basis.data)], dim=-1)  # [R, 258]
            terms = na.ops.sh_view_terms(dirs, m.enc.basis.data, 1.0, m.init.weight.data[:, :258], m.init.bias.data,
                                         m.layers[0].weight.data[:, 128:386], m.layers[0].bias.data,
                                         m.layers[3].weight.data[:, 128:386], m.layers[3].bias.data)
            assert terms.shape == (3, R, 128)
            f64 = f.double().cpu()
            for j, lin in enumerate((m.init, m.layers[0], m.layers[3])):
                w = lin.weight.data.double().cpu()
                w = w[:, :258] if j == 0 else w[:, 128:386]
                x = f64 if j == 0 else torch.nn.functional.leaky_relu(f64)
                want = x @ w.T + lin.bias.data.double().cpu()
                # 258 products of |f| <= pi, |w| <= 0.12 in fp32: the same bound as the unhoisted Linear's
                assert maxdiff(terms[j], want) <= 2e-5, (R, j, maxdiff(terms[j], want))
            # init Linear: hoisted = rows kernel over the latent columns + per-ray bias; unhoisted = full [N, 322] rows
            init_rows = torch.cat([f.unsqueeze(0).expand(T, R, 258), lat], dim=-1).reshape(T * R, 322).contiguous()
            full = na.ops.linear_f32(init_rows, m.init.weight.data, m.init.bias.data)
            hoisted = na.ops.linear_f32_rows(lat, m.init.weight.data[:, 258:].contiguous(), None, "none", b_rows=terms[0])
            assert maxdiff(hoisted, full.double().cpu()) <= 2e-5
            # without a per-ray bias and with contiguous rows the new entry point IS na_linear_f32
            x0 = torch.randn(T * R, 128, device="cuda")
            w, b = m.layers[1].weight.data, m.layers[1].bias.data
            assert torch.equal(na.ops.linear_f32_rows(x0, w, b, "leaky_relu"), na.ops.linear_f32(x0, w, b, pre_act="leaky_relu"))
            x1 = lat.reshape(T * R, 64)
            w2 = torch.randn(33, 192, device="cuda")
            assert torch.equal(na.ops.linear_f32_rows(x0, w2, None, "sin", x1=lat),
                               na.ops.linear_f32(x0, w2, None, pre_act="sin", x1=x1.contiguous()))
            # a ray's terms do not depend on how many rays the launch has or where the ray sits in it
            if R > 1:
                assert torch.equal(na.ops.sh_view_terms(dirs[R // 2:], m.enc.basis.data, 1.0, m.init.weight.data[:, :258], m.init.bias.data,
                                                        m.layers[0].weight.data[:, 128:386], m.layers[0].bias.data,
                                                        m.layers[3].weight.data[:, 128:386], m.layers[3].bias.data), terms[:, R // 2:])


# ------------------------------------------------------------------------------------------------ the model against the reference
@pytest.mark.parametrize("prec", ["bf16x3", "f16x"])
@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_reference_goldens_in_fp64(na, monkeypatch, order, prec):
    h = load_golden(f"g20_plain_sph-har_o{order}")
    m = from_golden(na, h)
    na.config.set_precision(prec)
    spy = Spy(monkeypatch, na.ops, ROUTE_OPS)
    noted = set(na.utils._noted)
    with torch.no_grad():
        out = m(h["rays"].cuda())
    assert spy.n("sh_view_terms") == 1 and spy.n("linear_f32_rows") == 7 and spy.n("sh_shade") == 1 and spy.n("linear_f32") == 0
    assert set(na.utils._noted) == noted, "a fallback note was printed for the head's own fast path"
    e = maxdiff(out, h["out64"])
    print(f"\n[sph-har o{order} {str(h['act'])}/{str(h['bg'])} {prec}] |out - fp64| {e:.2e}  |out - reference fp32| {maxdiff(out, h['out']):.2e}  "
          f"(reference fp32 vs fp64: {maxdiff(h['out'], h['out64']):.2e})  alpha {maxdiff(m.alpha, h['alpha64']):.2e}  "
          f"weights {maxdiff(m.weights, h['weights64']):.2e}")
    assert e <= 1e-4
    assert torch.equal(m.ts.cpu(), h["ts"])
    assert maxdiff(m.alpha, h["alpha64"]) <= 1e-4 and maxdiff(m.weights, h["weights64"]) <= 1e-4


@pytest.mark.parametrize("order", [0, 1, 2, 3, 4])
def test_routes_and_their_parity(na, monkeypatch, order):
    """eval mode: the hoisted route (per-ray terms once per forward, no per-sample view features, no [N, 322] rows); gradients enabled: the
    plain route.  Each within 1e-4 of the reference's fp64 values."""
    h = load_golden(f"g20_plain_sph-har_o{order}")
    m = from_golden(na, h)
    rays = h["rays"].cuda()
    T = int(h["steps"])
    R = rays.numel() // 6
    N = T * R
    spy = Spy(monkeypatch, na.ops, ROUTE_OPS)
    with torch.no_grad():
        hoisted = m(rays)
    assert spy.n("sh_view_terms") == 1 and spy.calls["sh_view_terms"][0][0] == (R, 3)
    assert spy.n("linear_f32_rows") == 7 and spy.n("linear_f32") == 0
    widths = [s[-1] for call in spy.calls["linear_f32_rows"] for s in call]
    assert max(widths) <= 192, widths  # x (128) and latent (64) columns, the [128, 192] matrices: nothing 322 or 450 wide
    for name in ("fourier_encode", "view_elaz"):  # no per-sample view features
        assert all(int(np.prod(s[:-1])) < N for call in spy.calls[name] for s in call), (name, spy.calls[name])
    assert spy.n("fourier_encode") == 0 and spy.n("view_elaz") == 0
    spy2 = Spy(monkeypatch, na.ops, ["sh_view_terms", "linear_f32_rows"])
    for tp in ("fp32", "bf16x3"):
        na.config.set_train_precision(tp)
        plain = m(rays)  # gradients enabled, parameters require them: the differentiable route
        assert plain.requires_grad and spy2.n("sh_view_terms") == 0 and spy2.n("linear_f32_rows") == 0
        print(f"\n[sph-har o{order} routes, train {tp}] hoisted vs fp64 {maxdiff(hoisted, h['out64']):.2e}, plain vs fp64 "
              f"{maxdiff(plain, h['out64']):.2e}, mutual {maxdiff(hoisted, plain.detach().cpu()):.2e}")
        assert maxdiff(plain, h["out64"]) <= 1e-4
    assert maxdiff(hoisted, h["out64"]) <= 1e-4
    # the plain route without gradients (per-sample directions handed to the head directly)
    with torch.no_grad():
        m.refl._hoistable = lambda *a: False
        plain_ng = m(rays)
        del m.refl._hoistable
    assert spy2.n("sh_view_terms") == 0 and maxdiff(plain_ng, h["out64"]) <= 1e-4


SHAPES = [((1, 7, 9), 48, 0, False), ((2, 16, 16), 128, 0, False), ((1, 33, 31), 70, 0, True), ((3,), 1, 0, False), ((5, 13), 33, 1, True),
          ((1, 4, 100), 24, 0, False), ((67,), 1, 1, True)]


@pytest.mark.parametrize("shape,T,n_rl,warp", SHAPES)
def test_hoisted_against_plain_route_on_ragged_shapes(na, shape, T, n_rl, warp):
    """ragged ray counts (R not a multiple of 64 / 32), T = 1, T not a multiple of 32, explicit warped points through from_pts, a refl_latent
    column (a column slice of a wider tensor, as DynamicNeRF hands it over); two renders each within 1e-4 of the truth: 2e-4 apart"""
    order = (len(shape) + T) % 5
    m = build(na, order, act="thin" if n_rl else "upshifted", bg="white" if T == 70 else "black", steps=T, n_rl=n_rl)
    procedural_(m)
    g = torch.Generator().manual_seed(7 + T)
    o = torch.tensor([0.1, -0.2, 4.0]) + 0.05 * torch.randn(shape + (3,), generator=g)
    d = torch.nn.functional.normalize(torch.tensor([0.0, 0.05, -1.0]) + 0.15 * torch.randn(shape + (3,), generator=g), dim=-1) * 1.1
    rays = torch.cat([o, d], dim=-1).cuda()
    wide = (0.7 * torch.randn((T,) + shape + (n_rl + 2,), generator=g)).cuda()
    rl = wide[..., 1:1 + n_rl] if n_rl else None

    def render():
        if warp or n_rl:
            pts, ts, r_o, r_d, _ = na.nerf.compute_pts_ts(rays, m.t_near, m.t_far, m.steps)
            pts = (pts + 0.02 * torch.sin(pts * 3.0)).contiguous() if warp else pts
            out = m.from_pts(pts, ts, r_o, r_d, refl_latent=rl, rays=rays)
        else:
            out = m(rays)
        return out.clone(), m.alpha.clone(), m.weights.clone()
    with torch.no_grad():
        hoisted = render()
        again = render()
        m.refl._hoistable = lambda *a: False
        plain = render()
        del m.refl._hoistable
    for a, b, c in zip(hoisted, plain, again):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, c), "a repeated render is bit-identical"
        assert maxdiff(a, b.cpu()) <= 2e-4, maxdiff(a, b.cpu())
    assert hoisted[0].shape == shape + (3,) and float(hoisted[0].abs().max()) > 0
    print(f"\n[sph-har o{order} {shape} T={T} n_rl={n_rl}] hoisted vs plain route: {maxdiff(hoisted[0], plain[0].cpu()):.2e}")


def test_dynamic_nerf_with_a_refl_latent_column(na):
    """DynamicNeRF over PlainNeRF + sph-har: explicit (spline-warped) points, and the deformation network's refl_latent column is one more
    latent column of the head (latent_size 65)"""
    T = 24
    canon = na.nerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
    m = na.nerf.DynamicNeRF(canonical=canon, spline=4, refl_latent=1)
    m.set_refl(na.refl.refl_kinds["sph-har"](latent_size=m.intermediate_size, act="upshifted", out_features=3, order=3))
    m = m.cuda().eval()
    procedural_(m)
    head = m.canonical.refl
    assert head.mlp.latent_size == 65 and head.mlp.init.in_features == 2 + 256 + 65
    g = torch.Generator().manual_seed(21)
    shape = (2, 5, 7)
    o = torch.tensor([0.0, 0.1, 4.0]) + 0.05 * torch.randn(shape + (3,), generator=g)
    d = torch.tensor([0.0, 0.0, -1.0]) + 0.1 * torch.randn(shape + (3,), generator=g)
    rays = torch.cat([o, d], dim=-1).cuda()
    times = torch.tensor([0.25, 0.8]).cuda()
    with torch.no_grad():
        hoisted = m((rays, times)).clone()
        head._hoistable = lambda *a: False
        plain = m((rays, times)).clone()
        del head._hoistable
    assert torch.isfinite(hoisted).all() and hoisted.shape == shape + (3,)
    assert maxdiff(hoisted, plain.cpu()) <= 2e-4


def test_row_band_equals_the_slab_and_renders_repeat(na):
    m = build(na, 2, act="leaky_relu", bg="white", steps=40)
    procedural_(m)
    g = torch.Generator().manual_seed(33)
    o = torch.tensor([0.1, -0.2, 4.0]) + 0.05 * torch.randn((1, 12, 37, 3), generator=g)
    d = torch.tensor([0.0, 0.05, -1.0]) + 0.15 * torch.randn((1, 12, 37, 3), generator=g)
    rays = torch.cat([o, d], dim=-1).cuda()
    with torch.no_grad():
        slab = m(rays).clone()
        w_slab = m.weights.clone()
        assert torch.equal(m(rays), slab)
        band = m(rays[:, 5:8].contiguous())
        assert torch.equal(band, slab[:, 5:8]) and torch.equal(m.weights, w_slab[:, :, 5:8])


# ------------------------------------------------------------------------------------------------ gradients and training
def rel(a, b):
    b = torch.as_tensor(b)
    return float((a.detach().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-12))


def rel_l2(a, b):
    b = torch.as_tensor(b).double()
    return float((a.detach().cpu().double() - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("train_prec", ["fp32", "bf16x3"])
def test_whole_model_gradients_against_the_reference_in_fp64(na, train_prec):
    """d(sum(out * probe))/d(parameters) of PlainNeRF + sph-har (order 2) through the HIP backward kernels against the reference's own fp64
    autograd (g20_plain_sph-har_grads): relative 2e-3 per tensor -- L-inf of the largest entry with exact-fp32 GEMMs, L2 with split bf16,
    as tests/test_gpu_backward.py::check_grads measures the two modes -- and 1e-6 x E2E_TOL on the loss."""
    h = load_golden("g20_plain_sph-har_grads")
    m = from_golden(na, h)
    na.config.set_train_precision(train_prec)
    out = m(h["rays"].cuda())
    assert out.requires_grad
    loss = (out.double() * h["probe"].cuda()).sum()
    loss.backward()
    d_loss = abs(float(loss.detach()) - float(h["loss"]))
    named = dict(m.named_parameters())
    worst = 0.0
    for k in h["grad_names"].tolist():
        g, want = named[k].grad, h["grad_" + k]
        assert g is not None and float(g.abs().max()) > 0, k
        e = rel(g, want) if train_prec == "fp32" else rel_l2(g, want)
        print(f"[sph-har grads/{train_prec}] {k}: {e:.2e}")
        worst = max(worst, e)
    print(f"[sph-har grads/{train_prec}] |loss - reference fp64| {d_loss:.2e}; worst per-tensor gradient error {worst:.2e}")
    assert d_loss <= 1e-6 * E2E_TOL[train_prec]
    assert worst <= 2e-3
    assert len(h["grad_names"]) == 5


def procedural_init(model):
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("primes") or t.numel() == 0 or name == "scale" or name.endswith(".scale"):
                continue
            v = torch.from_numpy(proc_param(name, tuple(t.shape)))
            if name.endswith("basis"):
                v = v * 32.0
            t.copy_(v.to(t.dtype))


@pytest.mark.parametrize("train_prec", ["fp32", "bf16x3"])
def test_make_nerf_sh_training_tracks_the_reference(na, train_prec, tmp_path):
    """`make nerf-sh` (reference makefile:64-72) on the analytic scene, replaying the reference's random stream, at the bars
    tests/test_gpu_train.py holds the static recipes to: first 5 and first 10 losses within 2e-4, every test view within 0.1 dB (split
    bf16 GEMMs) / 0.01 dB (exact fp32 GEMMs) of the reference's run."""
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_nerf_sh.json")))
    import nerf_atlas_amd.train as T
    config = na.config
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    argv = [x for x in fx["argv"] if x not in ("-d", "--outdir")]
    args = T.args_from_argv(["-d", data] + argv)
    assert args.epochs == len(fx["losses"]) == 200 and args.refl_kind == "sph-har" and args.learning_rate == 1e-3
    config.set_precision("bf16x3")
    config.set_train_precision(train_prec)
    config.set_deterministic(True)
    try:
        res = T.fit(args, replay_reference_rng=True, init=procedural_init)
    finally:
        config.set_deterministic(False)
    assert isinstance(res["model"].refl, na.refl.SphericalHarmonic)
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    print(f"\n[nerf_sh/{train_prec}] |loss - ref| first 5: {np.abs(got[:5] - ref[:5]).max():.2e}, first 10: {np.abs(got[:10] - ref[:10]).max():.2e}, "
          f"all 200: {np.abs(got - ref).max():.2e}; test PSNR build {np.round(res['test_psnr'], 4).tolist()} vs reference "
          f"{np.round(fx['test_psnr'], 4).tolist()} (max diff {d.max():.4f} dB)")
    assert np.abs(got[:5] - ref[:5]).max() <= 2e-4, (got[:5], ref[:5])
    assert np.abs(got[:10] - ref[:10]).max() <= 2e-4, (got[:10], ref[:10])
    assert ref[-20:].mean() < 0.5 * ref[:20].mean(), "the recipe must actually learn"
    assert d.max() <= (0.01 if train_prec == "fp32" else 0.1), (res["test_psnr"], fx["test_psnr"])


def test_runner_cli_trains_and_renders_the_test_set(na, tmp_path):
    """python -m nerf_atlas_amd.runner with `make nerf-sh`'s flags (+ --refl-order): trains, renders the test set through the hoisted
    route, writes results.txt and a state_dict under the reference's keys"""
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2", "--steps", "24",
                       "--epochs", "12", "--quiet", "--model", "plain", "--refl-kind", "sph-har", "--refl-order", "3", "--sigmoid-kind",
                       "leaky_relu", "-lr", "1e-3", "--outdir", str(out), "--save", str(tmp_path / "m.pt")])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12 and all(np.isfinite(res["losses"]))
    sd = torch.load(tmp_path / "m.pt")
    assert tuple(sd["refl.mlp.out.weight"].shape) == (48, 128) and tuple(sd["refl.mlp.layers.3.weight"].shape) == (128, 450)
    assert "refl.mlp.enc.basis" in sd and "first.enc.embs.7.weight" in sd
