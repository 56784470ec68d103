"""The grid operators on the GPU (csrc/grid_ops.hip): total variation and its gradient in both accumulation modes and the trilinear
upsampling against tests/grid_ref.py and its derived bounds; NeRFVoxel.upsample, the --voxel-tv-* terms and --voxel-upsample in
training; the total-variation recipe against the recorded reference."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import grid_ref as G
import voxel_ref as V
from oracle.procedural import proc_param, proc_uniform

pytestmark = pytest.mark.gpu

NA_EWORKSPACE = -5   # include/nerf_atlas_amd.h
SQRT_MIN = float(np.sqrt(np.float32(1e-10), dtype=np.float32))   # sqrtf(fp32(1e-10))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def mode(det):
    """the deterministic mode is process-wide: always switched off again"""
    from nerf_atlas_amd import config
    if det:
        config.set_deterministic(True)
    try:
        yield
    finally:
        if det:
            config.set_deterministic(False)


class Spy:
    def __init__(self, monkeypatch, ops, names=("grid_tv", "grid_tv_backward", "grid_upsample")):
        self.calls = {n: 0 for n in names}
        for n in names:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, n, fn):
        def f(*a, **k):
            self.calls[n] += 1
            return fn(*a, **k)
        return f


def run_tv(ops, grid, idxs, g=1.0):
    gc, ic = grid.cuda(), idxs.cuda()
    value = ops.grid_tv(gc, ic)
    grad = ops.grid_tv_backward(gc, ic, torch.tensor(g, device="cuda"))
    assert value.dim() == 0 and grad.shape == grid.shape
    return value.cpu(), grad.cpu()


def check_tv(ops, grid, idxs, ref, det, what, g=1.0):
    value, grad = run_tv(ops, grid, idxs, g)
    n, C = idxs.numel(), grid.shape[-1]
    err, vb = abs(float(value.double()) - float(ref["value"])), G.value_bound(ref["value"], n, C, det)
    ratio = G.worst_ratio(grad, ref["grad"], G.grad_bound(ref, det))
    print(f"[grid_tv {what} {'det' if det else 'atomic'}] value |err| / bound {err / vb:.3f}, gradient worst |err| / bound {ratio:.3f}, "
          f"most addends in one entry {int(ref['cnt'].max())}")
    assert err <= vb, (what, det, err, vb)
    assert ratio <= 1.0, (what, det, ratio)


# ------------------------------------------------------------------------------------------------------------ total variation
@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("name", tuple(G.TV_GRIDS))
def test_tv_value_and_every_gradient_entry_inside_their_bounds(ops, name, det):
    """(a) every grid shape x every sample count"""
    grid = G.tv_grid(name)
    with mode(det):
        for n in G.TV_COUNTS:
            check_tv(ops, grid, G.tv_idxs(n, grid[..., 0].numel()), G.tv_reference(name, n), det, f"{name} n={n}")


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_tv_duplicates_add_up(ops, det):
    """(b) 256 copies of one index; a face-neighbour pair interleaved, so that one row is both voxel and neighbour"""
    with mode(det):
        for what, grid, idxs in G.duplicate_cases():
            ref = G.tv_ref(grid, idxs)
            assert int(ref["cnt"].max()) >= 128
            check_tv(ops, grid, idxs, ref, det, what)


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_tv_exact_cases(ops, det):
    """(c) a constant grid and a step below the clamp give sqrtf(fp32(1e-10)) bitwise and no gradient; a step of 2^-16 is above it.
    (Bitwise wherever the sum of K equal values is exact in the kernel's order -- K a power of two, at most two waves; at a ragged
    count the mean of equal values is held to the value bound like any other.)"""
    with mode(det):
        for C, n in ((1, 1), (1, 64), (1, 128), (4, 128)):
            value, grad = run_tv(ops, torch.full((4, 6, 2, C), 0.375), G.tv_idxs(n, 48))
            assert float(value) == SQRT_MIN and int(grad.count_nonzero()) == 0, (C, n, float(value))
        value, grad = run_tv(ops, torch.full((4, 6, 2, 5), 0.375), G.tv_idxs(257, 48))
        assert abs(float(value) - SQRT_MIN) <= G.value_bound(SQRT_MIN, 257, 5, det) and int(grad.count_nonzero()) == 0
        for step, above in ((2.0 ** -17, False), (2.0 ** -16, True)):
            grid = torch.zeros(2, 2, 2, 1)
            grid[1, 0, 0, 0] = step
            value, grad = run_tv(ops, grid, torch.tensor([0]))    # voxel (0, 0, 0); its x-neighbour holds the step
            want = torch.zeros(2, 2, 2, 1)
            if above:                                              # dx = -2^-16, t = 2^-16, K = 1
                want[0, 0, 0, 0], want[1, 0, 0, 0] = -1.0, 1.0
            assert float(value) == (step if above else SQRT_MIN), (step, float(value))
            assert torch.equal(grad, want), (step, grad.flatten().tolist())
        # K = 2 x 1: the entries are -1 / K and +1 / K
        grid = torch.zeros(2, 2, 2, 1)
        grid[1, 0, 0, 0] = 2.0 ** -16
        value, grad = run_tv(ops, grid, torch.tensor([0, 7]))      # (1, 1, 1) and its neighbours are all zero: below the clamp
        assert float(value) == float(np.float32((np.float64(2.0 ** -16) + np.float64(np.float32(SQRT_MIN))) / 2))
        assert grad.flatten().tolist() == [-0.5, 0, 0, 0, 0.5, 0, 0, 0]


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
def test_tv_non_finite_voxels_stay_loud(ops, det):
    """(d) a NaN and an Inf voxel among the sampled rows: a non-finite value, NaN gradients at exactly the reference's entries"""
    base = G.tv_grid("462x5")
    idxs = torch.arange(48, dtype=torch.int64)
    with mode(det):
        for bad, at in ((float("nan"), (1, 2, 0, 3)), (float("inf"), (3, 5, 1, 0)), (float("-inf"), (0, 0, 0, 4))):
            grid = base.clone()
            grid[at] = bad
            ref = G.tv_ref(grid, idxs, clean=False)
            value, grad = run_tv(ops, grid, idxs)
            assert not bool(torch.isfinite(value)) and not bool(torch.isfinite(ref["value"]))
            nan = torch.isnan(ref["grad"])
            assert 2 <= int(nan.sum()) <= 8 and not bool(nan[..., [c for c in range(5) if c != at[3]]].any())
            assert torch.equal(torch.isnan(grad), nan)
            assert G.worst_ratio(grad, ref["grad"], G.grad_bound(ref, det)) <= 1.0


def test_tv_deterministic_mode_is_independent_of_run_and_index_order(ops):
    """(e)"""
    for name, n in (("16x28", 32768), ("64x3", 32768), ("462x5", 257)):
        grid = G.tv_grid(name)
        idxs = G.tv_idxs(n, grid[..., 0].numel())
        order = torch.from_numpy(proc_uniform((n,), 5310, 1.0)).argsort()
        with mode(True):
            (va, a), (vb, b), (_, c) = run_tv(ops, grid, idxs), run_tv(ops, grid, idxs), run_tv(ops, grid, idxs[order])
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32)), name
        assert torch.equal(va.view(torch.int32), vb.view(torch.int32)), name


def test_tv_a_too_small_deterministic_workspace_is_refused(ops):
    """(f)"""
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    grid = G.tv_grid("16x28").cuda()
    idxs = G.tv_idxs(65, 4096).cuda()
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        with pytest.raises(_lib.NaError) as err:
            ops.grid_tv_backward(grid, idxs, torch.ones((), device="cuda"))
        assert err.value.code == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 28 * 4096} bytes" in str(err.value), str(err.value)
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0
    finally:
        config.set_deterministic(False)


def test_tv_argument_checks(ops, monkeypatch):
    """(g) all ValueError before any launch"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    launched = []
    for name in ("na_grid_tv", "na_grid_tv_backward"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: launched.append(_n) or 0)
    grid, idxs, one = G.tv_grid("4x3").cuda(), G.tv_idxs(8, 64).cuda(), torch.ones((), device="cuda")
    bad = (
        (grid.cpu(), idxs.cpu()),                                  # host tensors
        (grid, idxs.cpu()),
        (torch.zeros(4, 4, 4, 33).cuda(), idxs),                   # C = 33
        (grid, idxs.int()),                                        # int32 indices
        (grid, torch.tensor([0, 64]).cuda()),                      # an explicit index of n_elem
        (grid, torch.tensor([-1]).cuda()),
        (grid[..., 0], idxs),                                      # not 4-D
        (grid.permute(1, 0, 2, 3), idxs),                          # not contiguous
        (grid.double(), idxs),                                     # not fp32
        (torch.zeros(1, 4, 4, 3).cuda(), torch.tensor([0]).cuda()),
    )
    for g_, i_ in bad:
        with pytest.raises(ValueError):
            ops.grid_tv(g_, i_)
        with pytest.raises(ValueError):
            ops.grid_tv_backward(g_, i_, one)
    assert launched == []
    monkeypatch.undo()
    # the C entry points check on their own, and clamp an index they are given anyway: the last voxel, not an address outside
    out = torch.zeros(2).cuda()
    assert lib.na_grid_tv(ops._ptr(grid), 4, 4, 4, 33, ops._ptr(idxs), 8, ops._ptr(out), ops._stream()) == -1
    assert lib.na_grid_tv(ops._ptr(grid), 4, 4, 4, 3, None, 8, ops._ptr(out), ops._stream()) == -2
    far = torch.tensor([1 << 40, -5]).cuda()
    assert torch.equal(ops.grid_tv(grid, far, trusted=True), ops.grid_tv(grid, torch.tensor([63, 0]).cuda()))


def test_tv_through_autograd(ops, monkeypatch):
    """(h) GridTVFn scaled by a weight; one launch forward, one backward; nerf.total_variation draws through utils.randint"""
    from nerf_atlas_amd import autograd as ag, nerf, utils
    grid = G.tv_grid("462x5")
    idxs = G.tv_idxs(257, 48)
    ref = G.tv_ref(grid, idxs, g=0.3)
    spy = Spy(monkeypatch, ops)
    p = grid.cuda().requires_grad_(True)
    loss = 0.3 * ag.GridTVFn.apply(p, idxs.cuda(), False)
    assert spy.calls == {"grid_tv": 1, "grid_tv_backward": 0, "grid_upsample": 0}
    loss.backward()
    assert spy.calls == {"grid_tv": 1, "grid_tv_backward": 1, "grid_upsample": 0}
    assert abs(float(loss) / 0.3 - float(ref["value"])) <= G.value_bound(ref["value"], 257, 5, False)
    assert G.worst_ratio(p.grad, ref["grad"], G.grad_bound(ref, False)) <= 1.0
    # the public function: explicit indices are the same node; a draw comes from the random source, at the reference's position
    p.grad = None
    (0.3 * nerf.total_variation(p, idxs=idxs.cuda())).backward()
    assert G.worst_ratio(p.grad, ref["grad"], G.grad_bound(ref, False)) <= 1.0
    with pytest.raises(ValueError):
        nerf.total_variation(p, idxs=torch.tensor([48]).cuda())
    prev = utils.random_source
    try:
        utils.set_random_source(utils.ReferenceStreamRandom())
        torch.manual_seed(11)
        drawn = nerf.total_variation(p.detach(), samples=257)
        torch.manual_seed(11)
        want = G.tv_ref(grid, torch.randint(0, 48, (257,)))["value"]
    finally:
        utils.set_random_source(prev)
    assert abs(float(drawn) - float(want)) <= G.value_bound(want, 257, 5, False)


# ------------------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("S,R,C", G.UP_CASES)
def test_upsample_every_entry_inside_its_bound(ops, monkeypatch, S, R, C):
    grid, ref, bound = G.up_reference(S, R, C)
    spy = Spy(monkeypatch, ops)
    got = ops.grid_upsample(grid.cuda(), R)
    assert spy.calls["grid_upsample"] == 1 and got.shape == (R, R, R, C) and got.is_contiguous()
    ratio = G.worst_ratio(got, ref, bound)
    print(f"[grid_upsample {S} -> {R} x {C}] worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, (S, R, C, ratio)


def test_upsample_exact_cases_and_nan(ops):
    grid = G.up_grid(16, 3)
    assert torch.equal(ops.grid_upsample(grid.cuda(), 16).cpu(), grid)                      # R = S: bitwise the input
    ints = torch.from_numpy(np.rint(proc_uniform((8, 8, 8, 5), 5411, 8.0)).astype(np.float32))
    assert torch.equal(ops.grid_upsample(ints.cuda(), 16).cpu().double(), G.interpolate(ints.double(), 16))
    for S, R in ((4, 8), (4, 6), (6, 4), (4, 4)):
        bad = G.up_grid(S, 3).clone()
        bad[1, 2, 0, 1] = float("nan")
        bad[0, 0, 1, 2] = float("nan")     # next to the border: outputs that reach it with a weight of exactly zero
        got = ops.grid_upsample(bad.cuda(), R).cpu()
        want = G.interpolate(bad, R)
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and 0 < int(torch.isnan(want).sum()) < want.numel() // 2, (S, R)
    with pytest.raises(ValueError):
        ops.grid_upsample(grid, 32)                                                          # host tensor
    with pytest.raises(ValueError):
        ops.grid_upsample(grid.cuda(), 7)
    with pytest.raises(ValueError):
        ops.grid_upsample(torch.zeros(4, 6, 4, 1).cuda(), 8)


# ------------------------------------------------------------------------------------------------------------ the model
def voxel_model(S, seed=5500):
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=16)
    m.set_refl(refl.Positional(act="upshifted", latent_size=0, out_features=3))
    den, rgb = V.grid_values(S, seed)
    m.load_state_dict({"densities": den, "rgb": rgb})
    return m.cuda().eval()


@pytest.mark.parametrize("S,R", ((4, 16), (16, 8)))
def test_model_upsample(ops, monkeypatch, S, R):
    m = voxel_model(S)
    old = (m.densities, m.rgb)
    want = (G.interpolate(m.densities.detach().cpu().double(), R), G.interpolate(m.rgb.detach().cpu().double(), R))
    spy = Spy(monkeypatch, ops)
    m.upsample(R)
    assert spy.calls["grid_upsample"] == 2
    assert tuple(m.densities.shape) == (R, R, R, 1) and tuple(m.rgb.shape) == (R, R, R, 3) and m.resolution == R
    assert m.voxel_len == m.grid_radius * 2 / R
    assert all(isinstance(p, torch.nn.Parameter) and p.is_cuda and p.requires_grad for p in (m.densities, m.rgb))
    assert m.densities is not old[0] and m.rgb is not old[1] and sorted(k for k, _ in m.named_parameters()) == ["densities", "rgb"]
    assert float((m.densities.detach().cpu().double() - want[0]).abs().max()) <= 1e-5
    assert float((m.rgb.detach().cpu().double() - want[1]).abs().max()) <= 1e-5
    # both routes of forward on the new grids
    rays = V.generic_rays((3, 7), 5510)
    den, rgb = m.densities.detach().cpu(), m.rgb.detach().cpu()
    with torch.no_grad():
        out = m(rays.cuda())
    ts = m.ts.cpu()
    pts = V.pts_of(rays, ts)
    raw, _ = V.sample_ref(pts.reshape(-1, 3), den, rgb)
    ref = V.composite_ref(raw.reshape(pts.shape[:-1] + (4,)), ts, rays, "upshifted", "black")
    for route, got in (("eval", out), ("operator", m(rays.cuda()))):
        for g_, r_, n_ in zip((got, m.alpha, m.weights), ref, ("out", "alpha", "weights")):
            err = float((g_.detach().cpu().double() - r_).abs().max())
            print(f"[upsample {S} -> {R}, {route} route] {n_} max |err| {err:.2e}")
            assert err <= 1e-4, (route, n_, err)
    got.square().sum().backward()
    assert m.densities.grad.shape == (R, R, R, 1) and m.rgb.grad.shape == (R, R, R, 3)
    assert bool(torch.isfinite(m.rgb.grad).all()) and float(m.rgb.grad.abs().max()) > 0 and float(m.densities.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ training
def twenty_steps(tv_sigma, tv_rgb):
    """20 Adam steps towards a constant image from a density grid with noise on it (0.1 +- 0.5; the colour grid is uniform noise by the
    model's own initialisation) -> the image losses, the TV terms, TV(densities) and TV(rgb) after the run at one fixed set of indices.
    The noise is the point: NeRFVoxel's own densities start CONSTANT, the minimum of the term, and from there the term can only add
    variation in 20 steps -- Adam moves the untouched neighbours of every voxel the rays reach at the full rate (measured:
    TV(densities) 1.11e-1 with tv_sigma 0.5 against 9.72e-2 without)."""
    from nerf_atlas_amd import nerf, train
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos", "--near", "2", "--far", "6", "--steps", "16",
                                 "--voxel-tv-sigma", str(tv_sigma), "--voxel-tv-rgb", str(tv_rgb)])
    torch.manual_seed(0)
    m = train.load_model(args).train()
    with torch.no_grad():
        m.densities.add_(torch.from_numpy(proc_uniform((64, 64, 64, 1), 5530, 0.5)).cuda())
    opt = train.NaAdam(m.parameters(), lr=5e-2)
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    losses, terms = [], []
    for _ in range(20):
        opt.zero_grad()
        loss = (m(rays) - target).square().mean()
        losses.append(float(loss.detach()))
        if args.voxel_tv_sigma > 0:
            terms.append(nerf.total_variation(m.densities))
            loss = loss + args.voxel_tv_sigma * terms[-1]
        if args.voxel_tv_rgb > 0:
            terms.append(nerf.total_variation(m.rgb))
            loss = loss + args.voxel_tv_rgb * terms[-1]
        loss.backward()
        opt.step()
    idxs = G.tv_idxs(32768, 64 ** 3).cuda()
    tv_of = lambda p: float(nerf.total_variation(p.detach(), idxs=idxs))
    return losses, [float(t) for t in terms], tv_of(m.densities), tv_of(m.rgb)


def test_the_tv_terms_smooth_the_grid_while_the_loss_falls(ops):
    """(i)"""
    losses, terms, den_with, rgb_with = twenty_steps(0.5, 0.1)
    _, none, den_without, rgb_without = twenty_steps(0.0, 0.0)
    print(f"[voxel tv train] loss {losses[0]:.4f} -> {losses[-1]:.4f}; after the run TV(densities) {den_with:.3e} with the terms, "
          f"{den_without:.3e} without; TV(rgb) {rgb_with:.3e} / {rgb_without:.3e}")
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    assert len(terms) == 40 and none == [] and all(np.isfinite(terms)) and all(t > 0 for t in terms)
    assert den_with < den_without and rgb_with < rgb_without


def small_run(tmp_path, extra, epochs=12):
    from tools.make_scene import make_scene
    from nerf_atlas_amd import loaders, train as T
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    args = T.args_from_argv(["-d", data, "--size", "32", "--crop-size", "16", "--batch-size", "2", "--steps", "24", "--epochs", str(epochs),
                             "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2"] + extra)
    T.seed(args.seed)
    labels, cam, _ = loaders.load(args, training=True)
    return args, labels, cam.to("cuda")


def test_voxel_upsample_in_a_training_run(ops, tmp_path, monkeypatch):
    """(ii) --voxel-upsample 6:8 from a 4^3 model: the grids, the optimiser's state and the losses on both sides of the switch; the saved
    state_dict loads into a freshly built model through runner.load_state"""
    from nerf_atlas_amd import nerf, runner, train as T
    args, labels, cam = small_run(tmp_path, ["--voxel-upsample", "6:8", "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4"])
    model = T.load_model(args)
    model.load_state_dict({k: v for k, v in zip(("densities", "rgb"), V.grid_values(4, 5520))})
    assert model.resolution == 4 and model.densities.is_cuda
    opt = T.load_optim(args, model.parameters())
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=args.epochs, eta_min=args.sched_min)
    seen = []
    spy = Spy(monkeypatch, ops)
    losses = T.train(model, cam, labels, opt, args, sched=sched, on_iter=lambda i, l: seen.append((i, model.resolution)))
    assert spy.calls == {"grid_upsample": 2, "grid_tv": 24, "grid_tv_backward": 24}
    assert [r for _, r in seen] == [4] * 6 + [8] * 6 and len(losses) == 12 and all(np.isfinite(losses))
    sd = model.state_dict()
    assert tuple(sd["densities"].shape) == (8, 8, 8, 1) and tuple(sd["rgb"].shape) == (8, 8, 8, 3) and model.voxel_len == 1.3 * 2 / 8
    params = [p for g in opt.param_groups for p in g["params"]]
    assert len(params) == 2 and {id(p) for p in params} == {id(model.densities), id(model.rgb)} == {id(p) for p in opt.state}
    assert all(float(st["step"]) == 6 and st["exp_avg"].shape == p.shape for p, st in opt.state.items())
    assert len(T.train.last_tv_terms) == 12 and all(np.isfinite(float(v)) for row in T.train.last_tv_terms for v in row)
    path = tmp_path / "m.pt"
    torch.save(sd, path)
    fresh = T.load_model(args)
    assert fresh.resolution == 64
    fresh.load_state_dict(runner.load_state(str(path)))
    assert fresh.resolution == 8 and torch.equal(fresh.rgb, model.rgb) and fresh.rgb.is_cuda


def test_runner_cli_with_the_tv_flags_and_an_upsample(tmp_path, capsys):
    """python -m nerf_atlas_amd.runner --model voxel --refl-kind pos --voxel-tv-sigma 1e-3 --voxel-tv-rgb 1e-4 --voxel-upsample ITER:RESO"""
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2", "--steps", "24",
                       "--epochs", "12", "--quiet", "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2", "--outdir", str(out),
                       "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4", "--voxel-tv-bezier", "1", "--voxel-upsample", "8:32",
                       "--save", str(tmp_path / "m.pt")])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12 and len(res["tv_terms"]) == 12
    assert "[warn]: model does not have bezier control points or rigidity for static scene" in capsys.readouterr().out
    assert tuple(torch.load(tmp_path / "m.pt")["rgb"].shape) == (32, 32, 32, 3)


# ------------------------------------------------------------------------------------------------------------ training against the reference
def test_training_with_the_tv_terms_tracks_the_reference(tmp_path):
    """tests/golden/train_parity_voxel_tv.json: the `voxel` recipe of tools/ref_train_fixture.py plus --voxel-tv-sigma / --voxel-tv-rgb, the
    reference's runner.main replayed with its random stream -- two draws of 32^3 indices per iteration from torch's CPU generator.  The
    fixture carries the reference's trajectory WITHOUT the terms too: the two must be ten bars apart within the first 50 iterations, so
    that parity pins the terms and not only the stream position.  Bars of tests/test_gpu_voxel.py: first 10 losses within 2e-4, the
    smoothed curve within 0.1, every test view within 0.01 dB."""
    from conftest import GOLDEN
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    fx = json.load(open(os.path.join(GOLDEN, "train_parity_voxel_tv.json")))
    ref, without = np.array(fx["losses"]), np.array(fx["losses_without_tv"])
    sep = np.abs(ref[:50] - without[:50]).max()
    print(f"[voxel tv parity] the reference with and without the terms: {sep:.2e} apart within 50 iterations")
    assert sep >= 10 * 2e-4
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")])
    assert args.epochs == len(ref) == 200 and args.model == "voxel" and 0 < args.voxel_tv_sigma <= 1 and 0 < args.voxel_tv_rgb <= 1

    def procedural_init(model):
        with torch.no_grad():
            for k, v in model.state_dict().items():
                v.copy_(torch.from_numpy(proc_param(k, tuple(v.shape))))
    config.set_precision("bf16x3")
    config.set_deterministic(True)
    try:
        res = T.fit(args, replay_reference_rng=True, init=procedural_init)
    finally:
        config.set_deterministic(False)
    got = np.array(res["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    sm = lambda v: np.convolve(v, np.ones(20) / 20, mode="valid")
    dev = np.abs(sm(got) - sm(ref)).max() / sm(ref).max()
    tv_got, tv_ref = np.array(res["tv_terms"]), np.array(fx["tv_terms"])
    print(f"[voxel tv parity] |loss - ref| first 10 {np.abs(got[:10] - ref[:10]).max():.2e}, all 200 {np.abs(got - ref).max():.2e}; smoothed "
          f"curve {dev:.2e}; test PSNR {np.round(res['test_psnr'], 4).tolist()} vs {np.round(fx['test_psnr'], 4).tolist()} ({d.max():.5f} dB); "
          f"TV values first 10 {np.abs(tv_got[:10] - tv_ref[:10]).max():.2e}")
    assert np.abs(got[:10] - ref[:10]).max() <= 2e-4 and dev <= 0.1 and d.max() <= 0.01
    assert tv_got.shape == tv_ref.shape == (200, 2)
    assert ref[-20:].mean() < 0.5 * ref[:20].mean(), "the recipe must actually learn"
