"""csrc/image_loss.hip on the GPU: na_image_loss / na_image_loss_backward against the fp64 restatement of
tests/image_loss_ref.py within its derived bounds, against the reference's recorded fp32 results (tests/golden/g30_image_loss.npz)
within bound + g_dev, the definition's exact cases, NaN, bitwise reproducibility, and the entry points' contract."""
import ctypes as C

import numpy as np
import pytest
import torch

import image_loss_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu

ALL_SPACES = ("rgb", "hsv", "luminance", "xyz")
# 1, 2; around a wave; around a workgroup (257 is one above the most a single workgroup takes); g30's size; and one above the 65536
# pixels at which the grid stops growing (256 workgroups of 256): partial rows of every workgroup, a second pixel for one thread
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1025, R.BLOCK * R.MAX_BLOCKS + 1)


@pytest.fixture(scope="module")
def ops():
    from nerf_atlas_amd import ops
    return ops


def run(ops, got, ref, combo, g_up=1.0):
    """(loss, grad [P,3]) as numpy fp64 from one forward and one backward launch"""
    x, y = torch.from_numpy(got).cuda(), torch.from_numpy(ref).cuda()
    loss, stats = ops.image_loss(x, y, *combo)
    g = ops.image_loss_backward(x, y, stats, torch.tensor(g_up, device="cuda"), *combo)
    return float(loss), g.cpu().numpy().astype(np.float64), stats.cpu().numpy()


def ratios(loss, grad, r, extra=(0.0, 0.0)):
    """(worst |error| / bound of the loss and of the gradient's elements; an element whose bound is 0 must be exact)"""
    gb = r["grad_bound"] + extra[1]
    d = np.abs(grad - r["grad"])
    assert (d[gb == 0] == 0).all(), "an element whose gradient is exactly 0 by the definition came out non-zero"
    return abs(loss - r["loss"]) / (r["loss_bound"] + extra[0]), float((d[gb > 0] / gb[gb > 0]).max(initial=0.0))


@pytest.mark.parametrize("P", SIZES)
def test_forward_and_backward_within_the_derived_bounds(ops, P):
    got, ref = R.kink_free_draw(P, 100 + P)
    worst = (0.0, 0.0)
    for combo in R.COMBOS:
        loss, grad, stats = run(ops, got, ref, combo)
        r = R.restate(got, ref, *combo)
        rl, rg = ratios(loss, grad, r)
        worst = (max(worst[0], rl), max(worst[1], rg))
        assert rl <= 1 and rg <= 1, (P, R.combo_name(combo), rl, rg)
        assert np.abs(stats - r["stats"]).max() <= 1e-5 * np.abs(r["stats"]).max() + 1e-12
    print(f"[image loss] P = {P}: worst error / bound over {len(R.COMBOS)} combinations: loss {worst[0]:.3f}, gradient {worst[1]:.3f}")


def test_g30_the_references_recorded_results(ops):
    g = load_golden("g30_image_loss")
    assert g["combos"].tolist() == [R.combo_name(c) for c in R.COMBOS]
    worst = (0.0, 0.0)
    for si, name in enumerate(("draw", "edge")):
        got, ref = g[f"{name}_got"].numpy(), g[f"{name}_ref"].numpy()
        for ci, combo in enumerate(R.COMBOS):
            loss, grad, _ = run(ops, got, ref, combo)
            r = R.restate(got, ref, *combo)
            rec = dict(r, loss=float(g[f"{name}_loss"][ci]), grad=g[f"{name}_grad"][ci].numpy().astype(np.float64))
            rl, rg = ratios(loss, grad, rec, extra=tuple(g["g_dev"][ci, si].numpy()))
            worst = (max(worst[0], rl), max(worst[1], rg))
            assert rl <= 1 and rg <= 1, (name, R.combo_name(combo), rl, rg)
    print(f"[image loss] g30: worst |kernel - recorded| / (bound + g_dev): loss {worst[0]:.3f}, gradient {worst[1]:.3f}")


@pytest.mark.parametrize("gamma, tone", [(1.0, False), (0.5, False), (0.7, True), (1.0, True)])
def test_equal_images_give_zero_and_the_clamped_rmse(ops, gamma, tone):
    got, _ = R.kink_free_draw(300, 7)
    for fn, want in (("l2", 0.0), ("l1", 0.0), ("rmse", float(np.sqrt(np.float32(1e-10))))):
        loss, grad, _ = run(ops, got, got.copy(), ((fn,), ALL_SPACES, tone, gamma))
        assert loss == want and (grad == 0).all(), (fn, loss)
    assert float(np.float32(1e-5)) == float(np.sqrt(np.float32(1e-10)))


@pytest.mark.parametrize("gamma", [0.5, 0.7])
def test_the_gamma_clamp_below_at_and_above(ops, gamma):
    got = np.array([[5e-11, 0.4, 0.7], [1e-10, 0.2, 0.9], [2e-10, 0.8, 0.3]], dtype=np.float32)
    ref = np.array([[0.1, 0.2, 0.3], [0.5, 0.1, 0.3], [0.3, 0.3, 0.6]], dtype=np.float32)
    assert got[0, 0] < np.float32(1e-10) == got[1, 0] < got[2, 0]
    for combo in ((("l2",), ("rgb",), False, gamma), (("l2", "rmse"), ("rgb", "xyz", "hsv"), True, gamma)):
        loss, grad, _ = run(ops, got, ref, combo)
        r = R.restate(got, ref, *combo)
        assert grad[0, 0] == 0.0 and np.isfinite(grad).all() and grad[1, 0] != 0 and grad[2, 0] != 0
        assert max(ratios(loss, grad, r)) <= 1


def test_gamma_one_does_not_clamp(ops):
    got = np.array([[-0.25, 0.8, 0.3], [0.5, -0.5, 0.25]], dtype=np.float32)
    ref = np.array([[0.25, 0.5, 0.75], [0.5, 0.5, 0.5]], dtype=np.float32)
    loss, grad, _ = run(ops, got, ref, (("l2",), ("rgb",), False, 1.0))
    d = got.astype(np.float64) - ref
    assert loss == pytest.approx((d * d).mean(), rel=1e-6) and np.allclose(grad, 2 * d / 6, rtol=1e-6, atol=0) and grad[0, 0] < 0
    loss, grad, _ = run(ops, got, ref, (("l2", "l1"), ALL_SPACES, True, 1.0))
    assert max(ratios(loss, grad, R.restate(got, ref, ("l2", "l1"), ALL_SPACES, True, 1.0))) <= 1


def test_a_tied_arg_max_takes_the_lowest_index(ops):
    got = np.array([[0.6, 0.6, 0.1], [0.2, 0.7, 0.7], [0.5, 0.5, 0.5], [0.1, 0.3, 0.9]], dtype=np.float32)
    ref = np.full((4, 3), 0.125, dtype=np.float32)
    for gamma, tone in ((1.0, False), (0.5, True)):
        _, grad, _ = run(ops, got, ref, (("l2",), ("hsv",), tone, gamma))
        assert (grad != 0).tolist() == [[True, False, False], [False, True, False], [True, False, False], [False, False, True]]


def test_luminance_alone_means_over_P(ops):
    got, ref = R.kink_free_draw(5, 11)
    lum = lambda v: v.astype(np.float64) @ R.LUM
    d = lum(got) - lum(ref)
    loss, _, stats = run(ops, got, ref, (("l2",), ("luminance",), False, 1.0))
    assert loss == pytest.approx((d * d).sum() / 5, rel=1e-5) and stats[2] == pytest.approx(loss) and stats[0] == stats[1] == stats[3] == 0


@pytest.mark.parametrize("space", ALL_SPACES)
@pytest.mark.parametrize("gamma, tone", [(1.0, False), (0.5, True), (2.2, True)])
def test_a_nan_channel_makes_the_loss_nan(ops, space, gamma, tone):
    got, ref = R.kink_free_draw(300, 13)
    got[17] = (0.25, np.nan, 0.75)   # (not the pixel's largest channel: hsv's maximum must keep it)
    for fns in (("l2",), ("l1",), ("rmse",), ("l2", "rmse")):
        loss, _ = ops.image_loss(torch.from_numpy(got).cuda(), torch.from_numpy(ref).cuda(), fns, (space,), tone, gamma)
        assert torch.isnan(loss).item(), (space, fns, gamma, tone)


def test_two_runs_bit_for_bit_in_every_mode(ops):
    from nerf_atlas_amd import config
    got, ref = R.kink_free_draw(R.BLOCK * R.MAX_BLOCKS + 1, 5)
    x, y = torch.from_numpy(got).cuda(), torch.from_numpy(ref).cuda()
    combo = (("l2", "rmse"), ("rgb", "xyz", "hsv"), True, 0.5)

    def once():
        loss, stats = ops.image_loss(x, y, *combo)
        return loss.clone(), stats.clone(), ops.image_loss_backward(x, y, stats, torch.ones((), device="cuda"), *combo)
    a, b = once(), once()
    config.set_deterministic(True)
    try:
        c = once()
    finally:
        config.set_deterministic(False)
    for other in (b, c):
        assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, other))


def test_autograd_scaling_shapes_and_strides(ops):
    from nerf_atlas_amd import autograd as ag
    got, ref = (torch.from_numpy(v).cuda() for v in R.kink_free_draw(2 * 18 * 18, 3))
    combo = (("l2", "rmse"), ("rgb", "xyz", "hsv"), True, 0.5)
    flat = got.clone().requires_grad_(True)
    loss = ag.ImageLossFn.apply(flat, ref, *combo)
    (3.0 * loss).backward()
    _, stats = ops.image_loss(got, ref, *combo)
    assert torch.equal(flat.grad, ops.image_loss_backward(got, ref, stats, torch.tensor(3.0, device="cuda"), *combo))
    # g_up = 3 against 3 x (g_up = 1): both sit within their bounds of the exact gradient, so they differ by at most the two bounds' sum
    r3 = R.restate(got.cpu().numpy(), ref.cpu().numpy(), *combo, g_up=3.0)
    within = lambda a, b: bool(((a.double() - b.double()).abs().cpu().numpy() <= 2 * r3["grad_bound"]).all())
    assert within(flat.grad, 3 * ops.image_loss_backward(got, ref, stats, torch.tensor(1.0, device="cuda"), *combo))
    assert max(ratios(float(loss.detach()), flat.grad.cpu().numpy().astype(np.float64), r3)) <= 1
    # [B,h,w,3], and a transposed (non-contiguous) view of it, through the function load_loss_fn returns
    import nerf_atlas_amd.train as T
    fn = T.load_loss_fn(T.make_args(loss_fns=["l2", "rmse"], color_spaces=["rgb", "xyz", "hsv"], tone_map=True, gamma_correct_loss=0.5))
    img = got.view(2, 18, 18, 3).clone().requires_grad_(True)
    l4 = fn(img, ref.view(2, 18, 18, 3))
    l4.backward()
    assert torch.equal(l4.detach(), loss.detach()) and within(img.grad.view(-1, 3) * 3, flat.grad)
    imgT = got.view(2, 18, 18, 3).transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)
    assert not imgT.is_contiguous()
    lT = fn(imgT, ref.view(2, 18, 18, 3).transpose(1, 2).contiguous().transpose(1, 2))
    lT.backward()
    assert torch.equal(lT.detach(), l4.detach()) and torch.equal(imgT.grad, img.grad)


def test_return_codes_and_an_untouched_output(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    P = 300
    got, ref = (torch.from_numpy(v).cuda() for v in R.kink_free_draw(P, 9))
    out, stats = torch.full((1,), 7.0, device="cuda"), torch.full((8,), 7.0, device="cuda")
    nbytes = int(lib.na_image_loss_workspace_bytes(P))
    assert nbytes == 64 + 2 * 8 * 4 and lib.na_image_loss_workspace_bytes(0) == 0 and lib.na_image_loss_workspace_bytes(-1) == 0
    ws = torch.zeros(nbytes // 4, device="cuda")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())

    def fwd(got=got, ref=ref, P=P, spaces=1, fns=1, gamma=1.0, out=out, stats=stats, ws=ws, nbytes=nbytes):
        return lib.na_image_loss(p(got), p(ref), P, spaces, fns, gamma, 0, p(out), p(stats), p(ws), nbytes, None)

    def bwd(got=got, ref=ref, P=P, spaces=1, fns=1, gamma=1.0, stats=stats, g_up=out, g=torch.empty(P, 3, device="cuda")):
        return lib.na_image_loss_backward(p(got), p(ref), P, spaces, fns, gamma, 0, p(stats), p(g_up), p(g), None)
    EINVAL, ENULL, EWORKSPACE = -1, -2, -5
    for kw in (dict(got=None), dict(ref=None), dict(out=None), dict(stats=None), dict(ws=None)):
        assert fwd(**kw) == ENULL, kw
    for kw in (dict(got=None), dict(ref=None), dict(stats=None), dict(g_up=None), dict(g=None)):
        assert bwd(**kw) == ENULL, kw
    for call in (fwd, bwd):
        for kw in (dict(P=0), dict(P=-3), dict(spaces=0), dict(fns=0), dict(spaces=16), dict(fns=8), dict(gamma=0.0), dict(gamma=-1.0),
                   dict(gamma=float("nan")), dict(gamma=float("inf"))):
            assert call(**kw) == EINVAL, kw
    assert fwd(nbytes=nbytes - 1) == EWORKSPACE and fwd(nbytes=0) == EWORKSPACE
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (stats == 7.0).all() and (ws == 0).all(), "a refused call wrote something"
    assert fwd() == 0
    torch.cuda.synchronize()
    assert float(out) == pytest.approx(float(((got - ref) ** 2).mean()), rel=1e-6) and ws.view(torch.int32)[0].item() == 0
    with pytest.raises(ValueError, match="lab"):
        ops.image_loss(got, ref, ("l2",), ("lab",))
    with pytest.raises(ValueError, match="empty"):
        ops.image_loss(got, ref, (), ("rgb",))
