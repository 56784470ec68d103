"""--voxel-steps-fine on the GPU (csrc/voxel_fine.hip): the density-only proposal pass and the three renderers over per-ray
steps.  Bit for bit against the shared-step renderers where the steps are shared; against tests/voxel_fine_ref.py (membership fixed in
fp32, everything behind it in fp64, the rows taken from na_resample_ts as given) within the bounds that module chains from
voxel_ref.sample_bound / composite_ref.forward_bounds / the heads' scatter_bound (worst |err| / bound printed) where they are each ray's
own; the model's forward against the composition of the operators bit for bit."""
import contextlib

import pytest
import torch

import voxel_fine_ref as F
import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

pytestmark = pytest.mark.gpu

NA_EINVAL, NA_ENULL, NA_EUNSUPPORTED = -1, -2, -3   # include/nerf_atlas_amd.h
GR = V.GRID_RADIUS
HEADS = (("rgb", -1), ("plv", 0), ("plv", 4), ("sh", 0), ("sh", 4))
HEAD_IDS = [f"{h}{'' if k < 0 else k}" for h, k in HEADS]
ORACLE_ACTS = ("normal", "thin", "fat", "tanh", "upshifted", "relu", "sin", "leaky_relu", "upshifted_softplus", "upshifted_relu", "cyclic")
# (T, N): M = T + N lands on 3, 12, 64 and 65 -- one chunk of the lanes, several, a whole number of them and one step more
TN = ((2, 1), (8, 4), (33, 31), (33, 32))
SIZES = (1, 63, 65, 257)


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


def grids(head, order, S):
    return V.grid_values(S) if head == "rgb" else P.grid_values(S, order) if head == "plv" else H.grid_values(S, order)


def mixed_rays(R, seed=7300):
    """rays through the grid from outside (generic_rays: near 2 / far 6 start in the extrapolated region); every 4th starts INSIDE the
    grid (origins in +-1, the heads' own direction set: un-normalised, the zero direction and an axis among them), every 5th points
    away from it and never meets it"""
    rays = V.generic_rays((R,), seed + R).clone()
    if R >= 4:
        inside = P.rays_of(H.directions(R, seed + 1), seed + 2)
        rays[::4] = inside[::4]
        rays[1::5, 3:] = -rays[1::5, 3:]
    return rays.contiguous()


def shared_render(ops, head, order, rays, ts, den, rgb, act, bg):
    if head == "rgb":
        return ops.voxel_render(rays, ts, den, rgb, GR, act, bg)
    if head == "plv":
        return ops.voxel_plv_render(rays, ts, den, rgb, GR, act, bg)
    return ops.voxel_sh_render(rays, ts, den, rgb, order, GR, act, bg)


def rayts_render(ops, head, order, rays, ts_ray, den, rgb, act, bg):
    if head == "rgb":
        return ops.voxel_render_rayts(rays, ts_ray, den, rgb, GR, act, bg)
    if head == "plv":
        return ops.voxel_plv_render_rayts(rays, ts_ray, den, rgb, GR, act, bg)
    return ops.voxel_sh_render_rayts(rays, ts_ray, den, rgb, order, GR, act, bg)


def cases():
    """(S, T, N, R, act, bg): every S, (T, N), R and activation at least once"""
    acts = tuple(ops_sigmoid())
    out = []
    for i in range(max(len(acts), len(TN) * len(SIZES))):
        T, N = TN[i % len(TN)]
        out.append(((4, 6)[i % 2], T, N, SIZES[(i // len(TN)) % len(SIZES)], acts[i % len(acts)], ("black", "white")[(i // 2) % 2]))
    return out


def ops_sigmoid():
    from nerf_atlas_amd import ops as _ops
    return _ops.SIGMOID


# ------------------------------------------------------------------------------------------------------------ 1. proposal
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_proposal_is_the_renderers_alpha_and_weights_bit_for_bit(ops, head, order):
    for S, T, N, R, act, bg in cases():
        den, rgb = (g.cuda() for g in grids(head, order, S))
        rays = mixed_rays(R).cuda()
        for ts in (torch.linspace(2.0, 6.0, T).cuda(), torch.linspace(2.0, 6.0, T + N).cuda()):
            _, alpha, weights = shared_render(ops, head, order, rays, ts, den, rgb, act, bg)
            a, w = ops.voxel_proposal(rays, ts, den, GR)
            assert a.shape == alpha.shape and torch.equal(a, alpha), (S, ts.shape[0], R, float((a - alpha).abs().max()))
            assert w.shape == weights.shape and torch.equal(w, weights), (S, ts.shape[0], R, float((w - weights).abs().max()))


def test_proposal_batch_shape_and_lane_counts(ops):
    den, _ = grids("rgb", -1, 6)
    rays = V.generic_rays((2, 5, 7), 7310).cuda()
    ts = torch.linspace(2.0, 6.0, 33).cuda()
    a, w = ops.voxel_proposal(rays, ts, den.cuda(), GR)
    assert a.shape == w.shape == (33, 2, 5, 7)
    for lanes in ops.VOXEL_FINE_LANES:
        _, a2, w2 = ops.voxel_fine_lanes("density", lanes, rays, ts, den.cuda(), None, GR)
        assert torch.equal(a, a2) and torch.equal(w, w2), lanes


# ------------------------------------------------------------------------------------------------------------ 2. shared rows
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_rows_that_equal_a_shared_row_give_the_shared_step_renderer_bit_for_bit(ops, head, order):
    for S, T, N, R, act, bg in cases():
        M = T + N
        den, rgb = (g.cuda() for g in grids(head, order, S))
        rays = mixed_rays(R).cuda()
        ts = torch.linspace(2.0, 6.0, M)
        if M > 4:
            ts[3] = ts[2]   # a duplicate step (the 1e-5 clamp) in the shared row as well
        ts = ts.cuda()
        want = shared_render(ops, head, order, rays, ts, den, rgb, act, bg)
        got = rayts_render(ops, head, order, rays, ts.expand(R, M).contiguous(), den, rgb, act, bg)
        for g, r, n in zip(got, want, ("out", "alpha", "weights")):
            assert g.shape == r.shape and torch.equal(g, r), (S, M, R, act, bg, n, float((g - r).abs().max()))


def test_every_lane_count_gives_the_same_bits_and_the_optional_outputs_are_optional(ops):
    S, R, M = 6, 65, 65
    rays = mixed_rays(R).cuda()
    ts_ray = torch.sort(2.0 + 4.0 * torch.rand(R, M, generator=torch.Generator().manual_seed(5)), dim=1).values.cuda()
    for head, order in HEADS:
        den, rgb = (g.cuda() for g in grids(head, order, S))
        want = rayts_render(ops, head, order, rays, ts_ray, den, rgb, "thin", "white")
        for lanes in ops.VOXEL_FINE_LANES:
            got = ops.voxel_fine_lanes(head, lanes, rays, ts_ray, den, rgb, GR, order, "thin", "white")
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (head, order, lanes)
    out, alpha, weights = ops.voxel_render_rayts(rays, ts_ray, den.cuda(), grids("rgb", -1, S)[1].cuda(), GR, "thin", "white", want_weights=False)
    assert alpha is None and weights is None
    assert torch.equal(out, ops.voxel_render_rayts(rays, ts_ray, den.cuda(), grids("rgb", -1, S)[1].cuda(), GR, "thin", "white")[0])


# ------------------------------------------------------------------------------------------------------------ 3. real rows
def check_fine(ops, head, order, rays, ts_ray, den, rgb, act, bg, what):
    f = F.fine_ref(rays, ts_ray, den, rgb, head, order, act, bg)
    b = F.fine_bounds(f)
    got = rayts_render(ops, head, order, rays.cuda(), ts_ray.cuda(), den.cuda(), rgb.cuda(), act, bg)
    worst = {}
    for g, n in zip(got, ("out", "alpha", "weights")):
        assert g.shape == f["comp"][n].shape
        worst[n] = V.worst_ratio(g, f["comp"][n], b[n])
    print(f"[voxel fine {head}{order if order >= 0 else ''} {what} {act}/{bg}] worst |err| / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), (what, worst)


@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_resampled_rows_against_the_fp64_restatement(ops, head, order):
    """rows from na_resample_ts (linspace draws: the first and last land on coarse steps -- duplicates -- and given draws), rays that
    start outside, inside and never meet the grid"""
    i = HEADS.index((head, order))
    for j, (T, N) in enumerate(TN):
        S, R = (4, 6)[(i + j) % 2], SIZES[(i + j) % len(SIZES)]
        act, bg = ORACLE_ACTS[(2 * i + j) % len(ORACLE_ACTS)], ("black", "white")[(i + j) % 2]
        den, rgb = grids(head, order, S)
        rays = mixed_rays(R)
        ts = torch.linspace(2.0, 6.0, T)
        ref, pb = F.proposal_ref(rays, ts, den)
        a, w = ops.voxel_proposal(rays.cuda(), ts.cuda(), den.cuda(), GR)
        ra, rw = V.worst_ratio(a, ref["alpha"], pb["alpha"]), V.worst_ratio(w, ref["weights"], pb["weights"])
        print(f"[voxel proposal S={S} T={T} R={R}] worst |err| / bound: alpha {ra:.3f}, weights {rw:.3f}")
        assert ra <= 1.0 and rw <= 1.0, (ra, rw)
        u = None if j % 2 == 0 else torch.rand((N, R), generator=torch.Generator().manual_seed(7 + j)).cuda()
        ts_ray = ops.resample_ts(ts.cuda(), w, N, u).cpu()
        assert ts_ray.shape == (R, T + N) and bool((ts_ray[:, 1:] >= ts_ray[:, :-1]).all())
        check_fine(ops, head, order, rays, ts_ray, den, rgb, act, bg, f"S={S} T={T} N={N} R={R}")


@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 4), ("sh", 4)), ids=("rgb", "plv4", "sh4"))
def test_rows_on_the_lattice_and_with_duplicate_steps(ops, head, order):
    """every sample ON the lattice set (cell faces and centres, the corners, the origin: one ulp decides the membership, which the
    restatement fixes in fp32 like the kernel): origins voxel_ref.lattice_points, directions half a voxel per unit step along +-axes
    and diagonals, rows of small integers (exact products) with repeated steps"""
    S = 6
    o = V.lattice_points(S, n=56)
    R = o.shape[0]
    half = GR / S
    sign = torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [1.0, 1.0, 1.0], [-1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    rays = torch.cat([o, (sign[torch.arange(R) % 5] * half).float()], dim=-1).contiguous()
    M = 12
    rows = torch.arange(M, dtype=torch.float32).repeat(R, 1)
    rows[:, 5] = rows[:, 4]
    rows[1::2, 9:] = rows[1::2, 8:9]   # every second ray ends on four equal steps
    den, rgb = grids(head, order, S)
    check_fine(ops, head, order, rays, rows, den, rgb, "upshifted", "white", f"lattice R={R}")


# ------------------------------------------------------------------------------------------------------------ 4. NaN containment
def readers(rays, ts_ray, S, row):
    """[R] bool: the rays one of whose samples has grid row `row` among its 8 corners (whatever the weight: 0 x NaN is NaN)"""
    M = ts_ray.shape[1]
    ids, _ = V.cells(F.pts_rayts(rays, ts_ray).reshape(-1, 3), S, GR)
    return (V.rows_of(ids, S) == row).any(dim=1).reshape(M, -1).any(dim=0)


@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 1), ("sh", 1)), ids=("rgb", "plv1", "sh1"))
def test_a_nan_voxel_reaches_exactly_the_rays_that_read_it(ops, head, order):
    S, T, N, R = 6, 8, 4, 65
    den, rgb = grids(head, order, S)
    rays = V.generic_rays((R,), 7400)
    ts = torch.linspace(2.0, 6.0, T)
    _, w = ops.voxel_proposal(rays.cuda(), ts.cuda(), den.cuda(), GR)
    ts_ray = ops.resample_ts(ts.cuda(), w, N).cpu()
    ids, _ = V.cells(F.pts_rayts(rays, ts_ray).reshape(-1, 3), S, GR)
    rows = V.rows_of(ids, S).reshape(T + N, R, 8)
    per = torch.zeros(S ** 3, R, dtype=torch.bool)
    for r in range(R):
        per[rows[:, r].reshape(-1), r] = True
    row = int((per.sum(1).float() - R / 3).abs().argmin())   # a voxel a third of the rays read
    want = readers(rays, ts_ray, S, row)
    assert torch.equal(want, per[row])
    assert 0 < int(want.sum()) < R
    clean = rayts_render(ops, head, order, rays.cuda(), ts_ray.cuda(), den.cuda(), rgb.cuda(), "upshifted", "white")[0]
    assert bool(torch.isfinite(clean).all())
    for which in ("density", "colour"):
        d2, c2 = den.clone(), rgb.clone()
        if which == "density":
            d2.reshape(-1)[row] = float("nan")
        else:
            c2.reshape(S ** 3, -1)[row, c2.shape[-1] - 1] = float("nan")
        out = rayts_render(ops, head, order, rays.cuda(), ts_ray.cuda(), d2.cuda(), c2.cuda(), "upshifted", "white")[0].cpu()
        got = torch.isnan(out).any(-1)
        assert torch.equal(got, want), (which, int(got.sum()), int(want.sum()))
        assert torch.equal(out[~want], clean.cpu()[~want])
    # the proposal reads the density grid only
    d2 = den.clone()
    d2.reshape(-1)[row] = float("nan")
    a, w2 = ops.voxel_proposal(rays.cuda(), ts.cuda(), d2.cuda(), GR)
    assert torch.equal(torch.isnan(w2).any(0).cpu(), readers(rays, ts.expand(R, T).contiguous(), S, row))


# ------------------------------------------------------------------------------------------------------------ 5. the model
def model(head, order, S, steps, bg, act="upshifted"):
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=steps, bg=bg, sigmoid_kind=act)
    if head == "plv":
        m.set_refl(refl.PosLinearView(act=act, latent_size=0, out_features=3, voxel_order=order))
    elif head == "sh":
        m.set_refl(refl.SphericalHarmonic(act=act, latent_size=0, out_features=3, order=order, voxel_order=order))
    elif order == -1:
        m.set_refl(refl.Positional(act=act, latent_size=0, out_features=3))   # (order -2: the bare model, no head installed)
    m.set_sigmoid(act)
    den, rgb = grids(head, order, S)
    with torch.no_grad():
        m.densities.copy_(den)
        m.rgb.copy_(rgb)
    return m.cuda()


@pytest.mark.parametrize("bg", ("black", "white", "random"))
@pytest.mark.parametrize("head,order", HEADS + (("rgb", -2),), ids=HEAD_IDS + ["bare"])
def test_eval_forward_is_the_composition_of_the_operators_bit_for_bit(ops, head, order, bg):
    from types import SimpleNamespace
    from nerf_atlas_amd import render, utils
    S, T, N = 6, 8, 4
    m = model(head, order, S, T, bg).eval()
    m.steps_fine = N
    rays = V.generic_rays((2, 5, 7), 7500).cuda()
    torch.manual_seed(3)
    with torch.no_grad():
        out = m(rays)
    assert out.shape == (2, 5, 7, 3) and not out.requires_grad
    assert m.ts.shape == (T,) and m.ts_ray.shape == (2, 5, 7, T + N) and m.alpha.shape == m.weights.shape == (T + N, 2, 5, 7)
    ts = m.ts
    assert float((ts.cpu() - torch.linspace(2.0, 6.0, T)).abs().max()) <= 1e-6
    _, w = ops.voxel_proposal(rays, ts, m.densities.data, GR)
    ts_ray = ops.resample_ts(ts, w, N)
    assert torch.equal(m.ts_ray, ts_ray)
    want, alpha, weights = rayts_render(ops, head, max(order, -1), rays, ts_ray, m.densities.data, m.rgb.data, "upshifted", "black" if bg == "random" else bg)
    if bg == "random":
        torch.manual_seed(3)
        ops.sky_random(weights, utils.rand((2, 5, 7, 1), rays.device), want)
    assert torch.equal(out, want) and torch.equal(m.alpha, alpha) and torch.equal(m.weights, weights)
    depth = render.depth_map(SimpleNamespace(nerf=m))
    assert torch.equal(depth, ops.integrate(weights, ts_ray.movedim(-1, 0).unsqueeze(-1).contiguous()))
    # the caller's draws, and back to shared steps
    u = torch.rand((N, 2, 5, 7), generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        m.forward_coarse_fine(rays, N, u=u)
    assert torch.equal(m.ts_ray, ops.resample_ts(ts, w, N, u)) and not torch.equal(m.ts_ray, ts_ray)
    m.steps_fine = 0
    with torch.no_grad():
        plain = m(rays)
    assert m.ts_ray is None and m.weights.shape == (T, 2, 5, 7)
    if bg != "random":
        assert torch.equal(plain, shared_render(ops, head, max(order, -1), rays, ts, m.densities.data, m.rgb.data, "upshifted", bg)[0])
    m.steps_fine = N
    with torch.no_grad():
        m(rays)
        m.from_pts(ops.compute_pts(rays, ts), ts, rays[..., :3], rays[..., 3:], rays=rays)
    assert m.ts_ray is None


def test_training_mode_draws_once_and_takes_the_operator_route(ops, monkeypatch):
    calls = []
    for n in ("voxel_proposal", "resample_ts", "compute_pts_rayts", "voxel_render_rayts", "voxel_sample", "composite_rayts"):
        monkeypatch.setattr(ops, n, (lambda n, fn: lambda *a, **k: (calls.append(n), fn(*a, **k))[1])(n, getattr(ops, n)))
    m = model("rgb", -1, 6, 8, "black").train()
    m.steps_fine = 4
    rays = V.generic_rays((1, 3, 5), 7510).cuda()
    outs = []
    for seed in (11, 11, 12):
        torch.manual_seed(seed)
        out = m(rays)
        assert out.requires_grad and not m.ts_ray.requires_grad and m.ts_ray.shape == (1, 3, 5, 12)
        outs.append((out.detach().clone(), m.ts_ray.clone(), m.ts.clone()))
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert not torch.equal(outs[0][1], outs[2][1]) and not torch.equal(outs[0][2], torch.linspace(2.0, 6.0, 8).cuda())
    assert calls[:4] == ["voxel_proposal", "resample_ts", "compute_pts_rayts", "voxel_sample"] and "voxel_render_rayts" not in calls
    calls.clear()
    m.eval()
    with torch.no_grad():
        m(rays)
    assert calls == ["voxel_proposal", "resample_ts", "voxel_render_rayts"]


# ------------------------------------------------------------------------------------------------------------ 6. gradients
@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 1), ("sh", 1)), ids=("rgb", "plv1", "sh1"))
def test_gradients_of_both_grids_against_the_fp64_restatement(ops, head, order, det):
    """training mode, the caller's draws: d sum(out^2) / d densities, d rgb through the lookup's scatter, the activation's backward and
    na_composite_rayts_backward, against fp64 autograd of the restatement AT THE GPU's rows.  The proposal is outside the graph."""
    S, T, N = 4, 8, 4
    rays = mixed_rays(63).reshape(1, 7, 9, 6)
    u = torch.rand((N, 1, 7, 9), generator=torch.Generator().manual_seed(9))
    runs = []
    with mode(det):
        for _ in range(2):
            m = model(head, order, S, T, "white").train()
            torch.manual_seed(21)
            out = m.forward_coarse_fine(rays.cuda(), N, u=u.cuda())
            assert out.requires_grad
            out.square().sum().backward()
            runs.append((m.densities.grad.clone(), m.rgb.grad.clone(), m.ts_ray.clone()))
    if det:
        assert all(torch.equal(a, b) for a, b in zip(*runs))
    g_den, g_rgb, ts_ray = runs[0]
    ref, bound = F.fine_grads(rays.reshape(-1, 6), ts_ray.cpu().reshape(-1, T + N), *grids(head, order, S), head, order, "upshifted", "white", det)
    r_den = V.worst_ratio(g_den.reshape(-1), ref[:, 0], bound[:, 0])
    r_rgb = V.worst_ratio(g_rgb.reshape(S ** 3, -1), ref[:, 1:], bound[:, 1:])
    print(f"[voxel fine grads {head}{order if order >= 0 else ''} {'fixed-point' if det else 'atomics'}] worst |err| / bound: densities {r_den:.3f}, rgb {r_rgb:.3f}")
    assert r_den <= 1.0 and r_rgb <= 1.0, (r_den, r_rgb)


# ------------------------------------------------------------------------------------------------------------ 7. argument checks
def test_validation_codes_and_messages(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    p, st = ops._ptr, ops._stream()
    S, R, M = 4, 8, 5
    rays = V.generic_rays((R,), 7600).cuda()
    ts = torch.linspace(2, 6, M).cuda()
    ts_ray = ts.expand(R, M).contiguous()
    den = V.grid_values(S)[0].cuda()
    grid = torch.zeros(S ** 3 * 75 + 1, device="cuda")
    out, alpha, weights = (torch.full(s, 5.0, device="cuda") for s in ((R, 3), (M, R), (M, R)))

    def prop(rays_=p(rays), R_=R, ts_=p(ts), T_=M, den_=p(den), S_=S, gr=GR, a=p(alpha), w=p(weights)):
        return lib.na_voxel_proposal(rays_, R_, ts_, T_, den_, S_, gr, a, w, st)

    def rgbr(C=3, S_=S, M_=M, R_=R, act=4, bg=0, rays_=p(rays), row=p(ts_ray), den_=p(den), rgb_=p(grid), out_=p(out), gr=GR):
        return lib.na_voxel_render_rayts(rays_, R_, row, M_, den_, rgb_, S_, C, gr, act, bg, None, None, out_, st)

    def plvr(order=2, S_=S, M_=M, act=4, bg=0, rgb_=p(grid), out_=p(out)):
        return lib.na_voxel_plv_render_rayts(p(rays), R, p(ts_ray), M_, p(den), rgb_, S_, order, GR, act, bg, None, None, out_, st)

    def shr(C=12, order=1, S_=S, M_=M, act=4, bg=0, rgb_=p(grid), out_=p(out)):
        return lib.na_voxel_sh_render_rayts(p(rays), R, p(ts_ray), M_, p(den), rgb_, S_, C, order, GR, act, bg, None, None, out_, st)

    # shapes, resolution, grid radius, order
    assert prop(T_=0) == NA_EINVAL and b"na_voxel_proposal: bad shape" in lib.na_last_error()
    assert prop(R_=-1) == NA_EINVAL and prop(S_=5) == NA_EINVAL and prop(S_=0) == NA_EINVAL and prop(gr=0.0) == NA_EINVAL
    assert rgbr(M_=0) == NA_EINVAL and b"na_voxel_render_rayts: bad shape" in lib.na_last_error()
    assert rgbr(S_=3) == NA_EINVAL and b"resolution" in lib.na_last_error()
    assert rgbr(gr=-1.0) == NA_EINVAL and plvr(M_=0) == NA_EINVAL and shr(M_=0) == NA_EINVAL
    assert plvr(order=5) == NA_EINVAL and b"na_voxel_plv_render_rayts: order" in lib.na_last_error()
    assert plvr(order=-1) == NA_EINVAL and shr(C=27, order=5) == NA_EINVAL
    for C, order in ((12, 2), (3, 1), (75, 3)):   # C names another head's row
        assert shr(C=C, order=order) == NA_EINVAL and b"3 (order + 1)^2" in lib.na_last_error()
    # unsupported: channel count of the RGB head, activation, background
    assert rgbr(C=4) == NA_EUNSUPPORTED and b"C = 4" in lib.na_last_error()
    for fn in (rgbr, plvr, shr):
        assert fn(act=12) == NA_EUNSUPPORTED and b"activation kind 12" in lib.na_last_error()
        assert fn(act=-1) == NA_EUNSUPPORTED
        assert fn(bg=2) == NA_EUNSUPPORTED and b"bg kind 2" in lib.na_last_error()
    # null pointers
    assert prop(rays_=None) == NA_ENULL and prop(ts_=None) == NA_ENULL and prop(den_=None) == NA_ENULL
    assert prop(w=None) == NA_ENULL and b"na_voxel_proposal: weights is null" in lib.na_last_error()
    assert rgbr(rays_=None) == NA_ENULL and rgbr(row=None) == NA_ENULL and rgbr(den_=None) == NA_ENULL and rgbr(rgb_=None) == NA_ENULL
    assert rgbr(out_=None) == NA_ENULL and b"na_voxel_render_rayts: out is null" in lib.na_last_error()
    assert plvr(out_=None) == NA_ENULL and shr(out_=None) == NA_ENULL and plvr(rgb_=None) == NA_ENULL and shr(rgb_=None) == NA_ENULL
    # rows read 16 bytes at a time need an aligned grid
    off = grid[1:]
    assert plvr(order=2, rgb_=p(off)) == NA_EINVAL and b"16-byte" in lib.na_last_error()
    assert shr(C=12, order=1, rgb_=p(off)) == NA_EINVAL and b"16-byte" in lib.na_last_error()
    assert lib.na_voxel_fine_lanes(0, -1, 5, 0, p(rays), R, p(ts_ray), M, p(den), p(grid), S, GR, 4, 0, None, None, p(out), st) == NA_EINVAL
    assert b"lanes" in lib.na_last_error()
    assert lib.na_voxel_fine_lanes(4, -1, 16, 0, p(rays), R, p(ts_ray), M, p(den), p(grid), S, GR, 4, 0, None, None, p(out), st) == NA_EINVAL
    torch.cuda.synchronize()
    for t in (out, alpha, weights):
        assert bool((t == 5.0).all())
    # an empty batch is fine, alpha is optional, and the unaligned orders take any grid
    assert prop(R_=0) == 0 and rgbr(R_=0) == 0
    assert prop(a=None) == 0 and plvr(order=1, rgb_=p(off)) == 0 and shr(C=27, order=2, rgb_=p(off)) == 0 and rgbr(rgb_=p(off)) == 0
    torch.cuda.synchronize()
    assert bool((alpha == 5.0).all()) and not bool((weights == 5.0).any())
    # the Python wrappers
    with pytest.raises(ValueError, match=r"\[S,S,S,1\]"):
        ops.voxel_proposal(rays, ts, torch.zeros(S, S, S, 3).cuda(), GR)
    with pytest.raises(ValueError, match="channels"):
        ops.voxel_sh_render_rayts(rays, ts_ray, den, torch.zeros(S, S, S, 12).cuda(), 2, GR)
    with pytest.raises(ValueError, match="channels"):
        ops.voxel_plv_render_rayts(rays, ts_ray, den, torch.zeros(S, S, S, 5).cuda(), GR)
    with pytest.raises(NotImplementedError):
        ops.voxel_render_rayts(rays, ts_ray, den, torch.zeros(S, S, S, 3).cuda(), GR, bg="random")
    with pytest.raises(AssertionError):
        ops.voxel_render_rayts(rays, ts_ray[:4].contiguous(), den, torch.zeros(S, S, S, 3).cuda(), GR)
