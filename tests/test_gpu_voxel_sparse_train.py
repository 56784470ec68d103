"""NeRFVoxel.sparsify through the model and train.fit: the eval routes are the sparse launch and agree with the masked
operator route within the voxel tests' bar for that pair (tests/test_gpu_voxel.py `close`: the project's 1e-4); the gradient of a voxel
no live sample reads is exactly 0; --voxel-sparsify trains reproducibly under config.set_deterministic, changes nothing with an
all-live table, and at ITER == epochs only the test render."""
import contextlib
import os
import sys

import pytest
import torch

import voxel_ref as V
import voxel_sparse_ref as X

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tools.make_scene import make_scene  # noqa: E402

pytestmark = pytest.mark.gpu

GR = V.GRID_RADIUS
MID = X.MID
TOL = 1e-4   # tests/test_gpu_voxel.py, test_gpu_voxel_plv.py: `close` of the one-launch and the operator route
HEADS = (("rgb", -1), ("plv", 1), ("sh", 1))
HEAD_IDS = ("rgb", "plv1", "sh1")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def mode(det):
    from nerf_atlas_amd import config
    if det:
        config.set_deterministic(True)
    try:
        yield
    finally:
        if det:
            config.set_deterministic(False)


def model(head, order, S, steps, bg, act="upshifted"):
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=steps, bg=bg, sigmoid_kind=act)
    if head == "plv":
        m.set_refl(refl.PosLinearView(act=act, latent_size=0, out_features=3, voxel_order=order))
    elif head == "sh":
        m.set_refl(refl.SphericalHarmonic(act=act, latent_size=0, out_features=3, order=order, voxel_order=order))
    else:
        m.set_refl(refl.Positional(act=act, latent_size=0, out_features=3))
    m.set_sigmoid(act)
    den, rgb = V.grid_values(S)[0], X.grids(head, order, S)[1]   # (one density grid for every head: the same table)
    with torch.no_grad():
        m.densities.copy_(den)
        m.rgb.copy_(rgb)
    return m.cuda()


def close(got, ref, what):
    for g, r, n in zip(got, ref, ("out", "alpha", "weights")):
        err = float((g.detach().double() - r.detach().double()).abs().max())
        print(f"[{what}] {n} max |err| {err:.2e}")
        assert g.shape == r.shape and err <= TOL, (what, n, err)


# ------------------------------------------------------------------------------------------------------------ the model's routes
@pytest.mark.parametrize("bg", ("black", "white"))
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_eval_routes_are_the_sparse_launch_and_agree_with_the_operator_route(ops, head, order, bg, monkeypatch):
    S, T, N = 6, 17, 8
    m = model(head, order, S, T, bg).eval()
    frac = m.sparsify(MID)
    want_live = X.table_of(m.densities.detach().cpu(), MID)
    assert torch.equal(m.live.cpu(), want_live) and frac == float(want_live.sum()) / S ** 3 and 0 < frac < 1
    assert "live" in m.state_dict()
    calls = []
    for n in ("voxel_sparse_render", "voxel_render", "voxel_plv_render", "voxel_sh_render", "voxel_render_rayts", "voxel_plv_render_rayts",
              "voxel_sh_render_rayts", "voxel_proposal", "voxel_live_samples"):
        monkeypatch.setattr(ops, n, (lambda n, fn: lambda *a, **k: (calls.append(n), fn(*a, **k))[1])(n, getattr(ops, n)))
    rays = V.generic_rays((2, 3, 5), 9100).cuda()
    r_o, r_d = rays[..., :3], rays[..., 3:]
    with torch.no_grad():
        # forward: one sparse launch over the shared row
        out = m(rays)
        assert calls == ["voxel_sparse_render"], calls
        fused = (out, m.alpha, m.weights)
        ts = m.ts
        want = ops.voxel_sparse_render(head, rays, ts, m.densities.data, m.rgb.data, m.live, GR, max(order, -1), "upshifted", bg)
        assert all(torch.equal(a, b) for a, b in zip(fused, want))
        flags = ops.voxel_live_samples(m.live, GR, rays=rays, ts=ts).bool()
        assert 0 < int(flags.sum()) < flags.numel() and bool((m.alpha[~flags] == 0).all()) and bool((m.weights[~flags] == 0).all())
        calls.clear()
        via_ops = (m._operators(rays, ts, r_d), m.alpha, m.weights)
        assert calls == ["voxel_live_samples"], calls
        close(via_ops, fused, f"{head} forward, operator route")
        assert bool((via_ops[1][~flags] == 0).all()) and bool((via_ops[2][~flags] == 0).all())
        # from_pts with explicit points takes the operators
        calls.clear()
        out_p = m.from_pts(ops.compute_pts(rays, ts), ts, r_o, r_d, rays=rays)
        assert calls == ["voxel_live_samples"], calls
        close((out_p, m.alpha, m.weights), fused, f"{head} from_pts")
        # coarse -> fine: a dense proposal, then one sparse launch over per-ray rows
        m.steps_fine = N
        calls.clear()
        out_f = m(rays)
        assert calls == ["voxel_proposal", "voxel_sparse_render"], calls
        fused_f = (out_f, m.alpha, m.weights)
        ts_ray = m.ts_ray
        _, w = ops.voxel_proposal(rays, m.ts, m.densities.data, GR)
        assert torch.equal(ts_ray, ops.resample_ts(m.ts, w, N))
        want = ops.voxel_sparse_render(head, rays, ts_ray, m.densities.data, m.rgb.data, m.live, GR, max(order, -1), "upshifted", bg)
        assert all(torch.equal(a, b) for a, b in zip(fused_f, want))
        via_ops = (m._operators(rays, ts_ray, r_d, pts=ops.compute_pts_rayts(rays, ts_ray)), m.alpha, m.weights)
        close(via_ops, fused_f, f"{head} coarse -> fine, operator route")
        # without a table: the same launches as ever
        m.clear_live()
        calls.clear()
        m(rays)
        m.steps_fine = 0
        m(rays)
        assert "voxel_sparse_render" not in calls and "voxel_live_samples" not in calls and len(calls) == 3, calls


@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_a_voxel_no_live_sample_reads_has_gradient_exactly_zero(ops, head, order, det):
    S, T = 6, 17
    rays = V.generic_rays((1, 5, 7), 9200).cuda()
    with mode(det):
        m = model(head, order, S, T, "white").train()
        m.sparsify(MID)
        torch.manual_seed(5)
        out = m(rays)
        (out ** 2).sum().backward()
        ts = m.ts.detach().cpu()
        flat = rays.reshape(-1, 6).cpu()
        pts = V.pts_of(flat, ts).reshape(-1, 3)
        flags = X.flags_of(pts, m.live.cpu())
        ids, _ = V.cells(pts, S, GR)
        read = torch.zeros(S ** 3, dtype=torch.bool)
        read[V.rows_of(ids, S)[flags].reshape(-1)] = True
        assert 0 < int(read.sum()) < S ** 3 and 0 < int(flags.sum()) < flags.numel()
        g_den, g_rgb = m.densities.grad.reshape(S ** 3).cpu(), m.rgb.grad.reshape(S ** 3, -1).cpu()
        assert bool((g_den[~read] == 0).all()) and bool((g_rgb[~read] == 0).all())
        assert bool((g_den[read] != 0).any()) and bool((g_rgb[read] != 0).any())
        if det:
            # a table of ones is the identity in both directions: the dense model's gradients bit for bit
            grads = []
            for live in (torch.ones(S, S, S, dtype=torch.uint8, device="cuda"), None):
                m2 = model(head, order, S, T, "white").train()
                m2.live = live
                torch.manual_seed(5)
                o2 = m2(rays)
                (o2 ** 2).sum().backward()
                grads.append((o2.detach(), m2.densities.grad, m2.rgb.grad))
            assert all(torch.equal(a, b) for a, b in zip(*grads))


# ------------------------------------------------------------------------------------------------------------ train.fit
def scene(tmp_path):
    return make_scene(str(tmp_path / "s"), size=16, n_train=2, n_test=1) + "/"


def args(T, data, **kw):
    base = dict(data=data, model="voxel", refl_kind="pos", steps=16, size=16, crop_size=8, batch_size=1, epochs=6, learning_rate=1e-2)
    base.update(kw)
    return T.make_args(**base)


def noisy(model):
    """densities uniform in +-1: a threshold in the middle leaves a table that is neither empty nor full"""
    with torch.no_grad():
        d = model.nerf.densities
        d.copy_((2 * torch.rand(d.shape, generator=torch.Generator().manual_seed(11)) - 1).to(d.device))


def test_an_all_live_table_changes_no_loss_and_a_mixed_one_is_reproducible(tmp_path):
    import nerf_atlas_amd.train as T
    data = scene(tmp_path)
    with mode(True):
        plain = T.fit(args(T, data), init=noisy)
        ones = T.fit(args(T, data, voxel_sparsify=["0:0"]), init=noisy)
        mixed = [T.fit(args(T, data, voxel_sparsify=[f"0:{MID}", "3:0.5"]), init=noisy) for _ in range(2)]
    assert plain["sparsify"] == [] and plain["model"].nerf.live is None
    assert ones["sparsify"] == [[0, 0.0, 1.0]] and bool(ones["model"].nerf.live.all())
    assert len(plain["losses"]) == 6 and ones["losses"] == plain["losses"]
    assert torch.equal(ones["model"].nerf.densities, plain["model"].nerf.densities)
    a, b = mixed
    assert a["losses"] == b["losses"] and all(l == l and abs(l) != float("inf") for l in a["losses"])
    assert torch.equal(a["model"].nerf.densities, b["model"].nerf.densities) and torch.equal(a["model"].nerf.live, b["model"].nerf.live)
    assert torch.equal(a["frames"][0], b["frames"][0])
    assert [e[:2] for e in a["sparsify"]] == [[0, MID], [3, 0.5]] and a["sparsify"] == b["sparsify"]
    assert all(0 < e[2] < 1 for e in a["sparsify"]), a["sparsify"]
    assert a["losses"][0] != plain["losses"][0]   # the table was in force from the first step
    print(f"\n[voxel sparsify fit] live fractions {[round(e[2], 3) for e in a['sparsify']]}, loss {a['losses'][0]:.4f} -> {a['losses'][-1]:.4f}")


def test_sparsify_after_the_last_step_changes_the_test_render_only(tmp_path, monkeypatch):
    import nerf_atlas_amd.train as T
    from nerf_atlas_amd import ops
    data = scene(tmp_path)
    count = {"voxel_sparse_render": 0, "voxel_render": 0}
    for n in count:
        monkeypatch.setattr(ops, n, (lambda n, fn: lambda *a, **k: (count.__setitem__(n, count[n] + 1), fn(*a, **k))[1])(n, getattr(ops, n)))
    with mode(True):
        plain = T.fit(args(T, data), init=noisy)
        assert count["voxel_sparse_render"] == 0 and count["voxel_render"] >= 1
        count["voxel_render"] = 0
        late = T.fit(args(T, data, voxel_sparsify=[f"6:{MID}"]), init=noisy)
    assert late["losses"] == plain["losses"] and torch.equal(late["model"].nerf.densities, plain["model"].nerf.densities)
    assert count["voxel_sparse_render"] >= 1 and count["voxel_render"] == 0
    assert len(late["sparsify"]) == 1 and late["sparsify"][0][:2] == [6, MID] and 0 < late["sparsify"][0][2] < 1
    assert late["model"].nerf.live is not None
