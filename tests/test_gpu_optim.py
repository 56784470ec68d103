"""--opt-kind sgd / rmsprop / adamw and --decay as one-launch steps (csrc/optim.hip, train.NaSGD / NaRMSprop / NaAdamW / NaAdam) against
torch's own foreach optimiser of the same kind on the same device -- that is the oracle, bit for bit -- and against the reference's
recorded runs (tests/golden/train_parity_voxel_{rmsprop,adamw,sgd}.json, tools/ref_train_fixture.py)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.procedural import proc_param

pytestmark = pytest.mark.gpu

SIZES = [(1,), (3,), (4,), (5,), (1023,), (1024,), (1025,), (2049,), (256, 294)]
MISALIGNED = 777   # elements of the parameter that starts one float into its storage
STEPS = 12
# kind: (class name, torch class name, hyperparameters, lr, [(attribute, masks to walk)])
KINDS = {
    "sgd": ("NaSGD", "SGD", {}, 2e-2, [("FMA_MASK", (0, 8))]),
    "rmsprop": ("NaRMSprop", "RMSprop", dict(eps=1e-7), 2e-2, [("FMA_MASK", (0, 2, 4, 6))]),
    "adamw": ("NaAdamW", "AdamW", dict(eps=1e-7), 5e-3, [("FMA_MASK", tuple(range(8)))]),
    "adam_decay": ("NaAdam", "Adam", dict(eps=1e-7, weight_decay=0.01), 5e-3, [("FMA_MASK", tuple(range(8))), ("DECAY_FMA", (0, 8))]),
}


def same(a, b):
    """equal, NaN at the same places (torch.equal calls NaN unequal to itself)"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def make_params():
    torch.manual_seed(12)
    ps = [torch.nn.Parameter(torch.randn(*s, device="cuda") * 0.1) for s in SIZES]
    base = torch.randn(MISALIGNED + 1, device="cuda") * 0.1
    ps.append(torch.nn.Parameter(base[1:]))   # a contiguous view one float into its storage
    assert ps[-1].is_contiguous() and ps[-1].data_ptr() % 16 == 4
    return ps


_grad_cache = {}


def grads(step):
    """one gradient per parameter: magnitudes 1e-6 .. 1e2 element by element, a tenth of the elements exactly zero, one NaN (step 2) and
    one Inf (step 3) element.  Computed once per step, never modified (the optimisers get clones)."""
    if step not in _grad_cache:
        gen = torch.Generator(device="cuda").manual_seed(100 + step)
        out = []
        for i, s in enumerate(SIZES + [(MISALIGNED,)]):
            g = torch.randn(*s, device="cuda", generator=gen) * 10.0 ** torch.randint(-6, 3, s, device="cuda", generator=gen).float()
            g = g * (torch.rand(*s, device="cuda", generator=gen) > 0.1)
            if step == 2 and i == 6:
                g.view(-1)[1024] = float("nan")
            if step == 3 and i == 7:
                g.view(-1)[2048] = float("inf")
            out.append(g)
        _grad_cache[step] = out
    return _grad_cache[step]


def groups(ps, lr):
    half = len(ps) // 2
    return [dict(params=ps[:half]), dict(params=ps[half:], lr=lr * 0.25)]


def trajectory(cls, hyper, lr):
    """STEPS steps; two groups with different rates, the rate changed at step 6, parameter 1 without a gradient before step 4.  Returns
    the optimiser and, per step, clones of every parameter and every state tensor."""
    ps = make_params()
    opt = cls(groups(ps, lr), lr=lr, **hyper)
    snaps = []
    for step in range(STEPS):
        for i, (p, g) in enumerate(zip(ps, grads(step))):
            p.grad = None if (i == 1 and step < 4) else g.clone()
        if step == 6:
            for group in opt.param_groups:
                group["lr"] = group["lr"] * 0.4
        opt.step()
        state = [opt.state.get(p, {}) for p in ps]
        snaps.append([[p.detach().clone()] + [v.clone() for k, v in sorted(st.items()) if k != "step"] + [torch.tensor(float(st.get("step", 0)))]
                      for p, st in zip(ps, state)])
        for p, g in zip(ps, grads(step)):
            assert p.grad is None or same(p.grad, g), "the gradient tensor itself is not modified"
    return opt, snaps


def first_difference(snaps, ref):
    for step, (a, b) in enumerate(zip(snaps, ref)):
        for i, (ta, tb) in enumerate(zip(a, b)):
            if len(ta) != len(tb) or not all(same(x.cpu(), y.cpu()) for x, y in zip(ta, tb)):
                return step, i
    return None


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_one_launch_step_is_torch_foreach_step_bit_for_bit(kind):
    """after each of 12 steps every parameter and every state tensor (and the step counts) equal torch's foreach optimiser's, NaN at the
    same places: tensors of 1 .. 2049 elements and a (256, 294) matrix, a parameter whose pointer is not 16-byte aligned, gradients over
    eight orders of magnitude with exact zeros, a NaN and an Inf, a rate changed at step 6, a parameter that joins at step 4, two groups.
    Prints which contraction masks reproduce torch; the pinned one must be among them."""
    import nerf_atlas_amd.train as T
    name, torch_name, hyper, lr, walks = KINDS[kind]
    cls = getattr(T, name)
    ref_opt, ref = trajectory(getattr(torch.optim, torch_name), dict(hyper, foreach=True), lr)
    assert any(bool(t.isnan().any()) for t in ref[-1][6]), "the NaN gradient must have reached the trajectory"
    for attr, masks in walks:
        pinned, matching = getattr(cls, attr), []
        for mask in masks:
            setattr(cls, attr, mask)
            try:
                _, snaps = trajectory(cls, hyper, lr)
            finally:
                setattr(cls, attr, pinned)
            if first_difference(snaps, ref) is None:
                matching.append(mask)
        print(f"\n[{kind}] {attr}: contraction masks that reproduce torch's foreach step bit for bit: {matching}; pinned: {pinned}")
        assert pinned in matching, (kind, attr, matching)
    opt, snaps = trajectory(cls, hyper, lr)
    assert first_difference(snaps, ref) is None, first_difference(snaps, ref)
    # state_dicts interchange in both directions
    other = getattr(torch.optim, torch_name)(groups(make_params(), lr), lr=lr, **hyper)
    other.load_state_dict(opt.state_dict())
    mine = cls(groups(make_params(), lr), lr=lr, **hyper)
    mine.load_state_dict(ref_opt.state_dict())
    assert sorted(opt.state_dict()["state"]) == sorted(ref_opt.state_dict()["state"])
    assert all(sorted(a) == sorted(b) for a, b in zip(opt.state_dict()["state"].values(), ref_opt.state_dict()["state"].values()))


def test_a_chunk_with_an_empty_tensor_updates_every_tensor_once():
    """50 tensors, an empty one among the first 48: the tensor at index 48 belongs to the second launch only.  Through na_optim_step
    (adam and sgd) and through na_adam_step, every tensor against torch after one step."""
    from nerf_atlas_amd import ops
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-7
    sizes = [7] * 50
    sizes[5] = 0

    def make():
        torch.manual_seed(3)
        ps = [torch.nn.Parameter(torch.randn(n, device="cuda")) for n in sizes]
        for p in ps:
            p.grad = torch.randn(p.shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(int(p.numel()) + 5))
        return ps

    ref = make()
    torch.optim.Adam(ref, lr=lr, betas=(b1, b2), eps=eps, foreach=True).step()
    scal = [1 - b1, b2, 1 - b2, (1 - b2 ** 1.0) ** 0.5, eps, (lr / (1 - b1 ** 1.0)) * -1]
    for entry in ("optim", "adam"):
        ps = make()
        with torch.no_grad():
            m, v = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
            if entry == "optim":
                ops.optim_step("adam", ps, [p.grad for p in ps], m, v, scal + [0.0], 7)
            else:
                ops.adam_step(ps, [p.grad for p in ps], m, v, *scal, 7)
        bad = [i for i, (a, b) in enumerate(zip(ps, ref)) if not torch.equal(a, b)]
        assert bad == [], (entry, bad)
    ref, ps = make(), make()
    torch.optim.SGD(ref, lr=lr, foreach=True).step()
    with torch.no_grad():
        ops.optim_step("sgd", ps, [p.grad for p in ps], [], [], [-lr], 8)
    assert [i for i, (a, b) in enumerate(zip(ps, ref)) if not torch.equal(a, b)] == []


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_fitting_group_is_one_launch_and_another_takes_torchs_step(kind, monkeypatch):
    """ops.optim_step is called once per step, group and step count, and torch's _foreach_* ops are not entered; a group with
    momentum (sgd, rmsprop) or amsgrad (adam, adamw) takes torch's step and equals torch."""
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import ops
    name, torch_name, hyper, lr, _ = KINDS[kind]
    calls, foreach = [], []
    real = ops.optim_step
    monkeypatch.setattr(ops, "optim_step", lambda *a, **k: (calls.append(len(a[1])), real(*a, **k))[1])
    for f in [n for n in dir(torch) if n.startswith("_foreach_")]:
        monkeypatch.setattr(torch, f, (lambda fn, n: lambda *a, **k: (foreach.append(n), fn(*a, **k))[1])(getattr(torch, f), f))
    _, snaps = trajectory(getattr(T, name), hyper, lr)
    assert foreach == [], sorted(set(foreach))
    # two groups; in the first one parameter 1 joins at step 4: its own step count, so its own launch for the rules that count steps
    late = 1 if kind in ("adamw", "adam_decay") else 0
    assert len(calls) == 4 * 2 + (STEPS - 4) * (2 + late), calls
    calls.clear()
    unfit = dict(momentum=0.9) if kind in ("sgd", "rmsprop") else dict(amsgrad=True)
    _, snaps = trajectory(getattr(T, name), dict(hyper, **unfit), lr)
    assert calls == [] and len(foreach) > 0
    _, ref = trajectory(getattr(torch.optim, torch_name), dict(hyper, foreach=True, **unfit), lr)
    assert first_difference(snaps, ref) is None


# ------------------------------------------------------------------------------------------------------------ training against the reference
@pytest.mark.parametrize("kind,learns", [("rmsprop", 0.5), ("adamw", 0.5), ("sgd", 0.6)])
def test_training_tracks_the_reference(tmp_path, kind, learns):
    """tests/golden/train_parity_voxel_<kind>.json: the reference's runner.main with --opt-kind <kind> on the analytic scene, replayed
    like tests/test_gpu_voxel.py::test_training_tracks_the_reference with that test's bars (a model without a GEMM): first 10 losses
    within 2e-4, the smoothed curve within 0.1 of its maximum, every test view within 0.01 dB.  The reference's own 8- and 2-thread
    runs differ by 3e-8 in the worst loss and 1e-6 dB for every kind.  The recipe itself must learn: last-20 mean below `learns` x
    first-20 mean (recorded: rmsprop 0.27, adamw 0.16, sgd 0.51)."""
    from tools.make_scene import make_scene
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import config
    fx = json.load(open(os.path.join(GOLDEN, f"train_parity_voxel_{kind}.json")))
    data = make_scene(str(tmp_path / "scene"), **fx["scene"]) + "/"
    args = T.args_from_argv(["-d", data] + [x for x in fx["argv"] if x not in ("-d", "--outdir")])
    assert args.epochs == len(fx["losses"]) == 200 and args.model == "voxel" and args.opt_kind == kind

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
    got, ref = np.array(res["losses"]), np.array(fx["losses"])
    d = np.abs(np.array(res["test_psnr"]) - np.array(fx["test_psnr"]))
    sm = lambda v: np.convolve(v, np.ones(20) / 20, mode="valid")
    dev = np.abs(sm(got) - sm(ref)).max() / sm(ref).max()
    print(f"[voxel {kind} parity] |loss - ref| first 10 {np.abs(got[:10] - ref[:10]).max():.2e}, all 200 {np.abs(got - ref).max():.2e}; smoothed "
          f"curve {dev:.2e}; test PSNR {np.round(res['test_psnr'], 4).tolist()} vs {np.round(fx['test_psnr'], 4).tolist()} ({d.max():.5f} dB)")
    assert np.abs(got[:10] - ref[:10]).max() <= 2e-4 and dev <= 0.1 and d.max() <= 0.01
    assert ref[-20:].mean() < learns * ref[:20].mean(), "the recipe must actually learn"


# ------------------------------------------------------------------------------------------------------------ command line, upsampling
def test_runner_cli_trains_with_rmsprop(tmp_path):
    """python -m nerf_atlas_amd.runner --model voxel --refl-kind pos --opt-kind rmsprop"""
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    out = tmp_path / "out"
    res = runner.main(["-d", data, "--size", "32", "--crop-size", "16", "--test-crop-size", "32", "--batch-size", "2", "--steps", "24",
                       "--epochs", "12", "--quiet", "--model", "voxel", "--refl-kind", "pos", "--opt-kind", "rmsprop", "-lr", "1e-2",
                       "--outdir", str(out)])
    txt = (out / "results.txt").read_text()
    assert "[Summary" in txt and txt.count("PSNR") == 2 and len(res["losses"]) == 12 and all(np.isfinite(res["losses"]))


def test_voxel_upsample_with_rmsprop_keeps_training(tmp_path):
    """--voxel-upsample 6:8 from a 4^3 model under --opt-kind rmsprop: the new grids take the old ones' places in the optimiser, their
    state restarts with their shapes, and the run goes on"""
    import voxel_ref as V
    from tools.make_scene import make_scene
    from nerf_atlas_amd import loaders, train as T
    data = make_scene(str(tmp_path / "s"), size=32, n_train=4, n_test=2) + "/"
    args = T.args_from_argv(["-d", data, "--size", "32", "--crop-size", "16", "--batch-size", "2", "--steps", "24", "--epochs", "12",
                             "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2", "--opt-kind", "rmsprop", "--voxel-upsample", "6:8"])
    T.seed(args.seed)
    labels, cam, _ = loaders.load(args, training=True)
    model = T.load_model(args)
    model.load_state_dict({k: v for k, v in zip(("densities", "rgb"), V.grid_values(4, 5520))})
    opt = T.load_optim(args, model.parameters())
    assert type(opt) is T.NaRMSprop
    before = {}
    losses = T.train(model, cam.to("cuda"), labels, opt, args,
                     on_iter=lambda i, l: before.setdefault(i, [p.detach().clone() for p in model.parameters()]))
    assert len(losses) == 12 and all(np.isfinite(losses)) and model.resolution == 8
    params = [p for g in opt.param_groups for p in g["params"]]
    assert {id(p) for p in params} == {id(model.densities), id(model.rgb)} == {id(p) for p in opt.state}
    assert all(float(st["step"]) == 6 and st["square_avg"].shape == p.shape and sorted(st) == ["square_avg", "step"] for p, st in opt.state.items())
    assert all(not torch.equal(a, b) for a, b in zip(before[6], before[11])), "the upsampled grids keep moving"
