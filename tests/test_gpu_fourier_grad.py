"""The Fourier encoder's position gradient on the GPU (csrc/fourier_grad.hip) and the pairing it opens: D-NeRF over VolSDF's
Fourier-encoded MLP SDF network (`make dnerf_volsdf`, reference makefile:127-133).

Kernel level: against the reference's fp64 autograd (tests/golden/g22_fourier_grad.npz), in units of the ruler of tests/fourier_grad_ref.py
and within 2 x what the reference's OWN fp32 autograd costs there (`ref32_dev`); the init rows bit for bit against the operator chain.
Model level: the reference's DynamicNeRF(VolSDF(sdf.MLP)) in fp64 (g22_dnerf_volsdf_*), under tests/test_gpu_backward.py's D-NeRF rule.
Recipe level: the reference's own training run (train_parity_dnerf_volsdf.json) and its end-point ensemble."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import fourier_grad_ref as R
from conftest import GOLDEN, golden_params, load_golden
from oracle.procedural import proc_param, proc_uniform

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools.make_scene import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

NS = (1, 31, 32, 33, 64, 257)   # below / at / above one half-wave pair per wave, ragged tails, more than one workgroup (8 samples each)
# tests/test_gpu_backward.py's bars (imported where importable: that module is a test file, its names are restated here)
E2E_TOL = {"fp32": 1.0, "bf16x3": 40.0}
DNERF_LINF, DNERF_L2 = 2e-3, 0.3


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@pytest.fixture(params=["fp32", "bf16x3"])
def train_prec(request):
    from nerf_atlas_amd import config
    prev = config.train_precision
    config.set_train_precision(request.param)
    yield request.param
    config.set_train_precision(prev)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _latent(N, L, pitched):
    """[N, L] latent; pitched: a column slice of a wider buffer (row pitch L + 3, not contiguous)"""
    lat = _dev(proc_uniform((N, L + 3), 2230 + L, 1.0))
    return lat[:, 2:2 + L] if pitched else lat[:, 2:2 + L].contiguous()


# ------------------------------------------------------------------------------------------------- the kernels
def test_position_gradient_against_the_reference(ops):
    """gx of every case of g22_fourier_grad (F in {128, 4, 6} x D in {1, 2, 3} x scale in {1, 1.5} x sigma in {16, 32}, |x| <= 6) at
    N in {1, 31, 32, 33, 64, 257}, as the standalone encoder's gradient and as the init rows' (L in {0, 5}: pitch D + 2F + L, the
    features at column D, the raw columns' gradient added): |gx - fp64| / ruler <= 2 x ref32_dev(case), the factor being the freedom in
    the order of a 128-term cancelling sum.  The saved-rows variant reads the forward's own sin / cos: the same bits as recomputing.
    Measured on an MI355X: the worst entry is 0.51 of the bar, i.e. 1.02 x ref32_dev (F = 128, D = 1, scale 1, sigma 32, N = 64; the
    rows form gives the standalone form's bits; profiles/fourier_grad/README.md)."""
    worst, worst_case = 0.0, None
    for case in R.CASES:
        F, D, scale, sigma = case
        x, basis, g = R.case_inputs(*case)
        want, rule, bar = R.gx_ref(x, basis, scale, g), R.ruler(basis, scale, g), 2.0 * R.ref32_dev(*case)
        xb, bb, gb = _dev(x), _dev(basis), _dev(g)
        for N in NS:
            xs, gs = xb[:N].contiguous(), gb[:N].contiguous()
            got = ops.fourier_encode_backward_input(xs, bb, scale, gs)
            assert got.shape == (N, D)
            ratio = float((np.abs(got.cpu().numpy().astype(np.float64) - want[:N]) / rule[:N]).max())
            if ratio / bar > worst:
                worst, worst_case = ratio / bar, (case, N, "standalone")
            assert ratio <= bar, (case, N, ratio, bar)
            saved = ops.fourier_encode(xs, bb, scale)
            assert torch.equal(ops.fourier_encode_backward_input(xs, bb, scale, gs, saved=saved), got), (case, N)
            for L in (0, 5):
                lead = _dev(proc_uniform((N, D), 2240 + D, 1.0))
                rows_g = torch.cat([lead, gs, _dev(proc_uniform((N, L), 2250, 1.0))], dim=1).contiguous()
                got_r = ops.fourier_encode_backward_input(xs, bb, scale, rows_g, col0=D, lead=True)
                err = np.abs(got_r.cpu().numpy().astype(np.float64) - (want[:N] + lead.cpu().numpy().astype(np.float64)))
                ratio = float((err / rule[:N]).max())
                if ratio / bar > worst:
                    worst, worst_case = ratio / bar, (case, N, f"rows L={L}")
                assert ratio <= bar, (case, N, L, ratio, bar)
                # one summation order for every pitch: the rows form without a lead gradient gives the standalone form's bits
                rows_g[:, :D] = 0
                assert torch.equal(ops.fourier_encode_backward_input(xs, bb, scale, rows_g, col0=D, lead=True), got), (case, N, L)
    print(f"\n[fourier_grad] worst |gx - fp64| / ruler = {worst:.3f} x (2 x ref32_dev) at {worst_case}")


def test_rows_are_the_operator_chain_bit_for_bit(ops):
    """na_fourier_rows == cat([x, fourier_encode(x), latent]) for every case and N, L in {0, 5}, contiguous and pitched latent"""
    for case in R.CASES:
        F, D, scale, sigma = case
        x, basis, _ = R.case_inputs(*case)
        xb, bb = _dev(x), _dev(basis)
        for N in NS:
            xs = xb[:N].contiguous()
            enc = ops.fourier_encode(xs, bb, scale)
            assert torch.equal(ops.fourier_rows(xs, bb, scale), torch.cat([xs, enc], dim=1)), (case, N)
            for pitched in (False, True):
                lat = _latent(N, 5, pitched)
                assert lat.is_contiguous() != pitched or N == 1
                rows = ops.fourier_rows(xs, bb, scale, lat)
                assert rows.shape == (N, D + 2 * F + 5) and torch.equal(rows, torch.cat([xs, enc, lat], dim=1)), (case, N, pitched)


def test_backward_is_reproducible_and_refuses_bad_shapes(ops):
    from nerf_atlas_amd._lib import NaError
    x, basis, g = R.case_inputs(128, 3, 1.5, 16)
    xb, bb, gb = _dev(x), _dev(basis), _dev(g)
    a = ops.fourier_encode_backward_input(xb, bb, 1.5, gb)
    for _ in range(3):
        assert torch.equal(ops.fourier_encode_backward_input(xb, bb, 1.5, gb), a)
    # a batch of the training step's class: many workgroups, the grid-stride loop
    N = 70001
    xl, gl = _dev(proc_uniform((N, 3), 2260, 6.0)), _dev(proc_uniform((N, 259), 2261, 1.0))
    big = ops.fourier_encode_backward_input(xl, bb, 1.0, gl, col0=3, lead=True)
    assert torch.equal(ops.fourier_encode_backward_input(xl, bb, 1.0, gl, col0=3, lead=True), big)
    want = R.gx_ref(xl.cpu().numpy(), basis, 1.0, gl[:, 3:].cpu().numpy()) + gl[:, :3].cpu().numpy().astype(np.float64)
    ratio = float((np.abs(big.cpu().numpy() - want) / R.ruler(basis, 1.0, gl[:, 3:].cpu().numpy())).max())
    assert ratio <= 2.0 * R.ref32_dev(128, 3, 1.0, 16), ratio
    assert ops.fourier_encode_backward_input(xb[:0], bb, 1.0, gb[:0]).shape == (0, 3) and ops.fourier_rows(xb[:0], bb).shape == (0, 259)
    with pytest.raises((NaError, AssertionError)):
        ops.fourier_encode_backward_input(xb, bb, 1.0, gb[:, :255].contiguous())
    with pytest.raises((NaError, AssertionError)):
        ops.fourier_encode_backward_input(torch.zeros(4, 9, device="cuda"), torch.zeros(9, 4, device="cuda"), 1.0, torch.zeros(4, 8, device="cuda"))


def test_autograd_nodes(ops):
    """FourierEncodeFn / FourierInitFn: gradients w.r.t. the positions and the latent (a view of the rows' gradient), none for the basis"""
    import nerf_atlas_amd.autograd as ag
    case = (128, 3, 1.0, 16)
    x, basis, g = R.case_inputs(*case)
    N, bar = 64, 2.0 * R.ref32_dev(*case)
    xb, bb, gb = _dev(x[:N]).requires_grad_(), _dev(basis), _dev(g[:N])
    y = ag.FourierEncodeFn.apply(xb, bb, 1.0)
    assert torch.equal(y, ops.fourier_encode(xb.detach(), bb, 1.0))
    y.backward(gb)
    want, rule = R.gx_ref(x[:N], basis, 1.0, g[:N]), R.ruler(basis, 1.0, g[:N])
    assert float((np.abs(xb.grad.cpu().numpy() - want) / rule).max()) <= bar
    lat = _latent(N, 5, False).requires_grad_()
    x2 = _dev(x[:N]).requires_grad_()
    rows = ag.FourierInitFn.apply(x2, bb, 1.0, lat)
    g_rows = _dev(proc_uniform((N, 3 + 256 + 5), 2270, 1.0))
    g_rows[:, 3:259] = gb
    rows.backward(g_rows)
    assert torch.equal(lat.grad, g_rows[:, 259:])
    err = np.abs(x2.grad.cpu().numpy() - (want + g_rows[:, :3].cpu().numpy().astype(np.float64)))
    assert float((err / rule).max()) <= bar
    # only the latent needs a gradient: the position kernel is not run, the rows still are
    rows = ag.FourierInitFn.apply(_dev(x[:N]), bb, 1.0, lat)
    assert rows.requires_grad


@pytest.mark.parametrize("N", [300, 2304])
@pytest.mark.parametrize("act", ["leaky_relu"])
def test_skip_layer_gradient_of_a_259_wide_second_source(ops, N, act, train_prec):
    """The skip layers of sdf.MLP are y = W . act([h (256) | init (259)]) + b; under a deformation field the SECOND source needs its
    gradient too, 259 columns: wider than the one-pass backward's narrow sources (<= 128) and no multiple of four.  LinearFn then takes
    linear_dgrad for both sources (the K-staged kernel below 2 048 rows, the packed layer-synchronous one from there on; exact-fp32:
    the f32 Linear on W^T and act_backward) and linear_wgrad.  Bar: tests/test_gpu_backward.py::test_linear_backward's 2e-4 of the
    largest entry."""
    from nerf_atlas_amd.autograd import LinearFn
    in0, in1, out = 256, 259, 256
    x0 = torch.from_numpy(proc_uniform((N, in0), 2281, 2.0))
    x1 = torch.from_numpy(proc_uniform((N, in1), 2282, 1.0))
    W = torch.from_numpy(proc_uniform((out, in0 + in1), 2283, (6.0 / (in0 + in1)) ** 0.5))
    b = torch.from_numpy(proc_uniform((out,), 2284, 0.1))
    gy = torch.from_numpy(proc_uniform((N, out), 2285, 1.0))
    r = [t.double().requires_grad_() for t in (x0, x1, W, b)]
    (torch.nn.functional.linear(torch.nn.functional.leaky_relu(torch.cat([r[0], r[1]], -1), 0.01), r[2], r[3]) * gy.double()).sum().backward()
    q = [t.cuda().requires_grad_() for t in (x0, x1, W, b)]
    packs = None
    if train_prec == "bf16x3" and ops.train_gemm_packed_ok(N, out) and ops.train_gemm_packed_ok(N, in0 + in1):
        f, t = ops.train_pack_many([(q[2], False), (q[2], True)])
        packs = (f, t)
    assert (packs is not None) == (train_prec == "bf16x3" and N >= 2048)
    y = LinearFn.apply(q[0], q[1], q[2], q[3], act, packs)
    (y * gy.cuda()).sum().backward()
    for a, ref, name in zip(q, r, ("x0", "x1", "W", "b")):
        e = float((a.grad.cpu().double() - ref.grad).abs().max() / ref.grad.abs().max())
        assert e <= 2e-4, (name, e)


# ------------------------------------------------------------------------------------------------- the model
def _build(h, na):
    kind, spline = str(h["refl_kind"]), int(h["spline"])
    s = na.sdf.SDF(na.sdf.MLP(intermediate_size=64), na.refl.View(latent_size=64, act="upshifted", out_features=3), isect=None,
                   t_near=float(h["near"]), t_far=float(h["far"]))
    canon = na.nerf.VolSDF(sdf=s, steps=int(h["steps"]), t_near=float(h["near"]), t_far=float(h["far"]), sigmoid_kind="upshifted")
    m = na.nerf.DynamicNeRF(canonical=canon, spline=spline)
    m.set_refl(na.refl.refl_kinds[kind](latent_size=m.intermediate_size, act="upshifted", out_features=3))
    m = m.cuda().eval()
    sd = m.state_dict()
    for k, v in golden_params(h).items():
        sd[k].copy_(v)
    sd["canonical.scale"].fill_(float(h["scale"]))
    return m


@pytest.mark.parametrize("name", ["view_s4", "plv_s6"])
def test_dnerf_over_volsdf_against_the_reference(ops, name, train_prec):
    """DynamicNeRF(VolSDF(sdf.MLP)) with the View and the PosLinearView head, live warp (delta_estim.out non-zero), 2 views x 4 x 4 rays
    x 8 steps, against the reference's fp64 run: out / alpha / weights / dp / rigidity within 1e-4, the l2 loss within 1e-6 x E2E_TOL,
    every parameter gradient under tests/test_gpu_backward.py's D-NeRF rule (exact-fp32 GEMMs: L-inf of the tensor's largest entry;
    split bf16: relative L2 0.3), evaluated on the entries the fixture keeps (<= 1000 per tensor, evenly spaced; hash tables: over the
    touched entries).

    The fp32 L-inf bar is the rule's 2e-3 wherever the fixture allows it, and otherwise derived from the fixture's own deviation on the
    same inputs: max(2e-3, 2 x own_linf), own_linf being the reference's OWN fp32 autograd against its fp64 run at the recorded frame
    times (0.25 / 0.8 for both cases, no draw picked), worst tensor, in units of the tensor's largest entry.  view_s4: own_linf 3.2e-5,
    bar 2e-3.  plv_s6: own_linf 5.2e-2, bar 0.103 -- on these 256 samples the reference's fp32 run crosses hash-cell faces and LeakyReLU
    kinks its fp64 run does not (the sigma = 16 SDF network holds ~70 of 65 536 pre-activations within 2e-5 of the kink in each of its
    later layers; one flip moves a sum over 256 samples by 1 / 256 = 3.9e-3), and an fp32 implementation that rounds differently is
    held to twice what the reference's costs.  Measured on an MI355X with exact-fp32 GEMMs, worst tensor: view_s4 3.5e-5,
    plv_s6 2.3e-2 (less than half the reference's own 5.2e-2); split bf16, relative L2: 1.6e-2 / 4.0e-2.  The recipe test below is the
    sharper statement on the gradient: with exact-fp32 GEMMs its first ten losses follow the reference's to 3.7e-9.  A wrong or
    missing term of the position gradient is an O(1) error of every delta_estim gradient.
    The deformation network's gradients are non-zero: the position gradient flows through the Fourier encoder."""
    import nerf_atlas_amd as na
    import nerf_atlas_amd.nerf, nerf_atlas_amd.refl, nerf_atlas_amd.sdf  # noqa: F401,E401
    h = load_golden("g22_dnerf_volsdf_" + name)
    m = _build(h, na)
    target = torch.from_numpy(proc_uniform(tuple(h["rays"].shape[:-1]) + (3,), int(h["target_seed"]), 0.5)) + 0.5
    out = m((h["rays"].cuda(), h["times"].cuda()))
    assert out.requires_grad
    loss = torch.nn.functional.mse_loss(out, target.cuda())
    loss.backward()
    fwd = {"out": out, "alpha": m.canonical.alpha, "weights": m.canonical.weights, "dp": m.dp, "rigidity": m.rigidity}
    for k, v in fwd.items():
        e = float((v.detach().cpu().double().reshape(h[k + "64"].shape) - h[k + "64"]).abs().max())
        print(f"\n[dnerf_volsdf {name}/{train_prec}] {k}: {e:.2e} off fp64", end="")
        assert e <= 1e-4, (k, e)
    dl = abs(float(loss.detach()) - float(h["loss64"]))
    print(f"\n[dnerf_volsdf {name}/{train_prec}] loss {float(loss.detach()):.7f}, {dl:.2e} off fp64")
    assert dl <= 1e-6 * E2E_TOL[train_prec], dl
    named = dict(m.named_parameters())
    linf_bar = max(DNERF_LINF, 2.0 * float(h["own_linf"]))
    worst, checked = 0.0, 0
    for k in h["grad_names"].tolist():
        gp = named[k].grad
        assert gp is not None, k
        sel = gp.detach().cpu().double().reshape(-1)[h["idx." + k].long()]
        ref = h["grad64." + k]
        if train_prec == "fp32":
            e = float((sel - ref).abs().max() / h["max64." + k].clamp_min(1e-12))
            assert e <= linf_bar, (k, e, linf_bar)
        else:
            e = float((sel - ref).norm() / ref.norm().clamp_min(1e-30))
            assert e <= DNERF_L2, (k, e)
        worst, checked = max(worst, e), checked + 1
    print(f"[dnerf_volsdf {name}/{train_prec}] worst per-tensor gradient error {worst:.2e} over {checked} tensors (fp32 L-inf bar {linf_bar:.3f})")
    assert checked == len(h["grad_names"]) >= 50
    assert m.canonical.sdf.underlying.mlp.enc.basis.grad is None
    for k in ("delta_estim.init.weight", "delta_estim.out.weight", "delta_estim.enc.embs.0.weight"):
        assert float(named[k].grad.abs().max()) > 0, k  # the deformation network really received a gradient through the encoder


# ------------------------------------------------------------------------------------------------- the recipe
def procedural_init(model):
    """tests/test_gpu_train.py's (restated: that module is a test file)"""
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith("primes") or t.numel() == 0 or name == "scale" or name.endswith(".scale"):
                continue
            if name.startswith("delta_estim.out."):
                continue  # the deformation head keeps the reference's zero initialisation (src/nerf.py:1256)
            v = torch.from_numpy(proc_param(name, tuple(t.shape)))
            if name.endswith("basis"):
                v = v * (16.0 if "sdf" in name else 32.0)
            t.copy_(v.to(t.dtype))


def _recipe(tmp_path):
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_dnerf_volsdf.json")))
    import nerf_atlas_amd.train as T
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    argv = [x for x in fx["argv"] if x not in ("-d", "--outdir")]
    return fx, T, T.args_from_argv(["-d", data] + argv)


def test_make_dnerf_volsdf_training_tracks_the_reference(train_prec, tmp_path):
    """`make dnerf_volsdf` (makefile:127-133) without its --sdf-eikonal, 30 iterations on the 16 x 16 scene (crop 8, 8 steps), replaying
    the reference's random stream.  The deformation head starts at zero (src/nerf.py:1256), so iteration 1 pins the forward and every
    later one the gradient that reached the deformation network through the Fourier encoder.

    The reference's own runs at 8, 4, 3, 2 and 1 threads (tests/golden/train_spread_dnerf_volsdf.json) agree to 9e-7 over the first 10
    iterations and are 1e-3 apart from iteration 27 on, their end points span 0.11 dB on a view and 0.07 dB on the mean: the rule of
    tests/test_gpu_train.py::test_training_tracks_the_reference for its chaotic recipes, bar for bar -- first 5 losses within 2e-4,
    first 10 within 1e-3, the 20-iteration smoothed curve within 0.35 of its maximum, the end point within 3 x the range the reference's
    runs span (capped by 1.3 / 0.9 dB) of their mean, per view and on the mean.  "Learns" is measured from the first three losses as
    that file does for volsdf_mlp, with the 0.7 of its short-budget recipes.  Measured on an MI355X (exact fp32 / split bf16): first 5
    losses 3.7e-9 / 7.7e-5, first 10 3.7e-9 / 2.6e-4, all 30 1.6e-4 / 8.5e-4, smoothed curve 0.0003 / 0.0039, end point 0.06 / 0.08 dB
    per view and 0.02 / 0.02 dB on the mean from the ensemble mean (bars 0.34 / 0.21 dB)."""
    fx, T, args = _recipe(tmp_path)
    from nerf_atlas_amd import config, nerf
    assert args.epochs == len(fx["losses"]) == 30
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        res = T.fit(args, replay_reference_rng=True, init=procedural_init)
    finally:
        config.set_deterministic(False)
    assert type(res["model"]) is nerf.DynamicNeRF and type(res["model"].canonical) is nerf.VolSDF
    assert float(res["model"].delta_estim.out.weight.abs().max()) > 0, "the deformation head has left its zero initialisation"
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    k = 20
    sm = lambda v: np.convolve(v, np.ones(k) / k, mode="valid")
    dev = np.abs(sm(got) - sm(ref)).max() / sm(ref).max()
    print(f"\n[dnerf_volsdf/{train_prec}] |loss - ref| first 5: {np.abs(got[:5] - ref[:5]).max():.2e}, first 10: {np.abs(got[:10] - ref[:10]).max():.2e}, "
          f"all 30: {np.abs(got - ref).max():.2e}; smoothed-curve deviation {dev:.4f}; test PSNR {np.round(res['test_psnr'], 4).tolist()} vs the "
          f"reference's 8-thread run {np.round(fx['test_psnr'], 4).tolist()}")
    assert np.abs(got[:5] - ref[:5]).max() <= 2e-4, (got[:5], ref[:5])
    assert np.abs(got[:10] - ref[:10]).max() <= 1e-3, (got[:10], ref[:10])
    assert dev <= 0.35, dev
    assert ref[-k:].mean() < 0.7 * ref[:3].mean(), "the recipe must actually learn"
    assert got[-k:].mean() < 0.7 * got[:3].mean(), "and so must this build's run of it"
    sp = json.load(open(os.path.join(GOLDEN, "train_spread_dnerf_volsdf.json")))["dnerf_volsdf"]
    assert sp["reference_runs"][0]["test_psnr"] == fx["test_psnr"]
    ref_runs = np.array([r["test_psnr"] + [r["test_psnr_mean"]] for r in sp["reference_runs"]])
    assert len(ref_runs) >= 3
    rng_ = ref_runs.max(axis=0) - ref_runs.min(axis=0)
    bar_view, bar_mean = min(1.3, 3.0 * rng_[:-1].max()), min(0.9, 3.0 * rng_[-1])
    dev_view = np.abs(np.array(res["test_psnr"]) - ref_runs[:, :-1].mean(axis=0)).max()
    dev_mean = abs(res["test_psnr_mean"] - ref_runs[:, -1].mean())
    print(f"[dnerf_volsdf/{train_prec}] end point vs the reference's own ensemble (n = {len(ref_runs)}): bars {bar_view:.3f} / {bar_mean:.3f} dB; "
          f"this run {dev_view:.3f} / {dev_mean:.3f} dB from the ensemble mean")
    assert dev_view <= bar_view and dev_mean <= bar_mean, (res["test_psnr"], ref_runs.tolist(), bar_view, bar_mean)


def test_rows_and_chain_paths_train_alike_and_deterministically(tmp_path, monkeypatch):
    """The rows path (FourierInitFn) and the operator chain cat([p, FourierEncodeFn(p)]) (NA_TRAIN_ROWS=0) of a tiny fit: the first 3
    losses bit for bit, the bar of tests/test_gpu_backward.py's rows-vs-chain test (same features, same gradient kernel, one summation
    order for both pitches).  Deterministic mode: two runs of 5 iterations leave the same parameters bit for bit."""
    fx, T, args = _recipe(tmp_path)
    from nerf_atlas_amd import config
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        args.epochs = 3
        losses = []
        for flag in ("1", "0"):
            monkeypatch.setenv("NA_TRAIN_ROWS", flag)
            losses.append(T.fit(args, replay_reference_rng=True, init=procedural_init)["losses"])
        assert losses[0] == losses[1] and len(losses[0]) == 3, losses
        monkeypatch.delenv("NA_TRAIN_ROWS")
        args.epochs = 5
        runs = []
        for _ in range(2):
            res = T.fit(args, replay_reference_rng=True, init=procedural_init)
            runs.append((res["losses"], {k: v.detach().clone() for k, v in res["model"].state_dict().items()}))
        assert runs[0][0] == runs[1][0]
        for k, v in runs[0][1].items():
            assert torch.equal(v, runs[1][1][k]), k
        assert float(runs[0][1]["delta_estim.out.weight"].abs().max()) > 0
    finally:
        config.set_deterministic(False)


def test_refusals(tmp_path):
    fx, T, args = _recipe(tmp_path)
    from nerf_atlas_amd import neural_blocks
    args.epochs, args.sdf_eikonal = 2, 1e-5   # the makefile's line as shipped: the reference raises a TypeError at runner.py:804-808
    with pytest.raises(NotImplementedError, match="runner.py:804-808"):
        T.fit(args, init=procedural_init)
    x = torch.zeros(4, 3, device="cuda", requires_grad=True)
    with pytest.raises(NotImplementedError, match="PositionalEncoder"):
        neural_blocks.PositionalEncoder(input_dims=3).cuda()(x)
    with pytest.raises(NotImplementedError, match="LearnedFourierEncoder"):
        neural_blocks.LearnedFourierEncoder(input_dims=3).cuda()(x)
