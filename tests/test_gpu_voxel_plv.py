"""--model voxel --refl-kind pos-linear-view --voxel-refl-order K on the GPU (csrc/voxel.hip): the lookup with the head, its scatter
in both accumulation modes and both table variants, its position gradient and the one-launch eval route against tests/voxel_plv_ref.py
(membership fixed in fp32, everything behind it in fp64), and the model on both routes against the recorded reference (g27).  Bounds:
voxel_plv_ref's derived ones for the operators (worst |err| / bound printed), the project's 1e-4 for everything composited."""
import contextlib

import pytest
import torch

from conftest import golden_params, load_golden
import voxel_plv_ref as P
import voxel_ref as V
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

NA_EINVAL, NA_ENULL, NA_EWORKSPACE = -1, -2, -5   # include/nerf_atlas_amd.h
SAMPLE_N = {1: (1, 1), 63: (7, 9), 65: (5, 13), 257: (1, 257), 1000: (8, 125)}   # N: (T, R); no R divides 64 but 1
ORDERS = (0, 1, 4)   # rows of 16, 28 (4-byte loads) and 112 bytes


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


def check_sample(ops, pts, rays, den, rgb, order, what, ts=None, grid_radius=V.GRID_RADIUS):
    """pts [T,R,3] (explicit when ts is None, else what the kernel forms from rays x ts)"""
    raw, mag, s, mag_s = P.sample_ref(pts.reshape(-1, 3), rays[:, 3:], den, rgb, grid_radius)
    kw = {"pts": pts.cuda()} if ts is None else {"ts": ts.cuda()}
    got_raw, got_s = ops.voxel_plv_sample(den.cuda(), rgb.cuda(), grid_radius, rays.cuda(), **kw)
    assert got_raw.shape == pts.shape[:-1] + (4,) and got_s.shape == pts.shape[:-1]
    r1 = V.worst_ratio(got_raw, raw, V.sample_bound(mag))
    r2 = V.worst_ratio(got_s, s, P.sh_bound(mag_s, order))
    print(f"[voxel_plv_sample K={order} {what}] worst |err| / bound: raw {r1:.3f}, sh {r2:.3f}")
    assert r1 <= 1.0 and r2 <= 1.0, (what, r1, r2)
    return got_raw, got_s


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_sample_both_position_forms(ops, S, order):
    """uniform points in +-2.5 (inside and extrapolated) at every ragged size, explicit and formed in the kernel; directions
    un-normalised, one of them zero, one on an axis"""
    den, rgb = P.grid_values(S, order)
    for N, (T, R) in SAMPLE_N.items():
        rays = P.rays_of(P.directions(R))
        check_sample(ops, V.uniform_points(N).reshape(T, R, 3), rays, den, rgb, order, f"S={S} N={N} pts")
        ts = torch.linspace(0.0, 2.5, T) if T > 1 else torch.tensor([1.25])
        a = check_sample(ops, V.pts_of(rays, ts), rays, den, rgb, order, f"S={S} N={N} rays x ts", ts=ts)
        b = ops.voxel_plv_sample(den.cuda(), rgb.cuda(), V.GRID_RADIUS, rays.cuda(), pts=V.pts_of(rays, ts).cuda())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])   # the two position forms: the same bits


@pytest.mark.parametrize("order", ORDERS)
def test_sample_lattice_and_zero_sets(ops, order):
    for S in (2, 4, 16):
        den, rgb = P.grid_values(S, order)
        for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points())):
            n = pts.shape[0]
            R = next(r for r in (5, 3, 1) if n % r == 0)
            check_sample(ops, pts.reshape(n // R, R, 3), P.rays_of(P.directions(R)), den, rgb, order, f"S={S} {name}")


def test_leading_outputs_are_the_rgb_heads_bits(ops):
    """density and colour parameters are vox_gather's arithmetic: na_voxel_sample on the three leading channels gives the same bits"""
    den, rgb = P.grid_values(16, 4)
    rays = P.rays_of(P.directions(125))
    pts = V.uniform_points(1000).reshape(8, 125, 3).cuda()
    raw, _ = ops.voxel_plv_sample(den.cuda(), rgb.cuda(), V.GRID_RADIUS, rays.cuda(), pts=pts)
    ref = ops.voxel_sample(den.cuda(), rgb[..., :3].contiguous().cuda(), V.GRID_RADIUS, pts=pts)
    assert torch.equal(raw.view(torch.int32), ref.view(torch.int32))


def _guarded(t, pad=64, fill=-777.0):
    """t inside a buffer with `pad` sentinel floats on either side (16-byte aligned data); returns (view, check)"""
    buf = torch.full((t.numel() + 2 * pad,), fill, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, lambda: bool((buf[:pad] == fill).all()) and bool((buf[pad + t.numel():] == fill).all())


def test_non_finite_coordinates_are_nan_in_their_sample_only_and_guards_hold(ops):
    """a NaN and an Inf coordinate in every operator: NaN in that sample's outputs (and its <= 8 grid rows) only; guard regions around
    every buffer the kernels read or write are unchanged"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    S, order, T, R = 16, 4, 9, 29
    N = T * R
    den, rgb = P.grid_values(S, order)
    rays = P.rays_of(P.directions(R))
    pts = V.uniform_points(N, 4301).clone()
    bad = {5: (1, float("nan")), 70: (0, float("inf")), 200: (2, float("-inf")), N - 1: (0, float("nan"))}
    for n, (a, v) in bad.items():
        pts[n, a] = v
    g_raw = torch.from_numpy(proc_uniform((N, 4), 4851, 1.0))
    g_sh = torch.from_numpy(proc_uniform((N,), 4852, 1.0))
    bufs = {k: _guarded(v.cuda()) for k, v in dict(pts=pts, rays=rays, den=den, rgb=rgb, g_raw=g_raw, g_sh=g_sh, raw=torch.zeros(N, 4),
                                                    sh=torch.zeros(N), g_pts=torch.zeros(N, 3), g_den=torch.zeros(S ** 3),
                                                    g_rgb=torch.zeros(S ** 3, 28)).items()}
    b = {k: v[0] for k, v in bufs.items()}
    p = ops._ptr
    rc = lib.na_voxel_plv_sample(p(b["pts"]), p(b["rays"]), R, None, T, p(b["den"]), p(b["rgb"]), S, order, V.GRID_RADIUS, p(b["raw"]), p(b["sh"]),
                                 ops._stream())
    assert rc == 0
    rc = lib.na_voxel_plv_sample_backward_pts(p(b["pts"]), p(b["rays"]), R, N, p(b["den"]), p(b["rgb"]), p(b["g_raw"]), p(b["g_sh"]), S, order,
                                              V.GRID_RADIUS, p(b["g_pts"]), ops._stream())
    assert rc == 0
    rc = lib.na_voxel_plv_sample_backward(p(b["pts"]), p(b["rays"]), R, None, T, p(b["g_raw"]), p(b["g_sh"]), S, order, V.GRID_RADIUS,
                                          p(b["g_den"]), p(b["g_rgb"]), ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert all(check() for _, check in bufs.values()), [k for k, (_, check) in bufs.items() if not check()]
    for k in ("raw", "g_pts"):
        rows = torch.isnan(b[k]).any(dim=-1).cpu()
        assert sorted(torch.nonzero(rows).flatten().tolist()) == sorted(bad) and bool(torch.isnan(b[k].cpu()[rows]).all()), k
    assert sorted(torch.nonzero(torch.isnan(b["sh"])).flatten().tolist()) == sorted(bad)
    # the outputs and the scattered gradient against the restatement (which makes the same samples and the same grid entries NaN)
    raw, mag, s, mag_s = P.sample_ref(pts, rays[:, 3:], den, rgb)
    assert V.worst_ratio(b["raw"], raw, V.sample_bound(mag)) <= 1.0 and V.worst_ratio(b["sh"], s, P.sh_bound(mag_s, order)) <= 1.0
    ref, mag, cnt = P.scatter_ref(pts, rays[:, 3:], g_raw, g_sh, S, order)
    got = torch.cat([b["g_den"].reshape(-1, 1), b["g_rgb"]], dim=-1)
    assert 0 < int(torch.isnan(ref[:, 0]).sum()) <= 8 * len(bad)
    assert V.worst_ratio(got, ref, P.scatter_bound(ref, mag, cnt, False)) <= 1.0


# ------------------------------------------------------------------------------------------------------------ scatter
def scatter(ops, name, order=4, perm=None, variant=None):
    p, dirs, g, gs, S, gr = P.scatter_inputs(name)
    R = dirs.shape[0]
    if perm is not None:   # a permutation of the samples that keeps every sample's ray: whole rows of R are permuted
        idx = (perm[:, None] * R + torch.arange(R)[None]).reshape(-1)
        p, g, gs = p[idx], g[idx], gs[idx]
    gd, gc = ops.voxel_plv_sample_backward(g.cuda(), gs.cuda(), S, order, gr, P.rays_of(dirs).cuda(), pts=p.reshape(-1, R, 3).cuda(),
                                           variant=variant)
    assert gd.shape == (S, S, S, 1) and gc.shape == (S, S, S, P.channels(order))
    return torch.cat([gd, gc], dim=-1).reshape(S ** 3, -1).cpu()


_SCATTER_REF = {}


def scatter_reference(name, order=4):
    if (name, order) not in _SCATTER_REF:
        p, dirs, g, gs, S, gr = P.scatter_inputs(name)
        _SCATTER_REF[name, order] = P.scatter_ref(p, dirs, g, gs, S, order, gr)
    return _SCATTER_REF[name, order]


@pytest.mark.parametrize("variant", (1, 2), ids=("rows-in-lds", "lead-in-lds"))
@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("name", V.SCATTER_CASES)
def test_scatter_every_entry_inside_its_bound(ops, name, det, variant):
    """voxel_ref's scatter shapes at C = 28: duplicates (A, B, L), more distinct cells in a workgroup's run than its table holds (D1000:
    up to 2048 cells in one round against 512 / 256 rows), two rounds (F); both modes, both table variants"""
    ref, mag, cnt = scatter_reference(name)
    with mode(det):
        got = scatter(ops, name, variant=variant)
    ratio = V.worst_ratio(got, ref, P.scatter_bound(ref, mag, cnt, det))
    print(f"[voxel_plv scatter {name} {'det' if det else 'atomic'} variant {variant}] worst |err| / bound {ratio:.3f}, most addends in one "
          f"entry {int(cnt.max())}")
    assert ratio <= 1.0, (name, det, variant, ratio)
    if name == "G":   # exact arithmetic in the four leading sums (the basis values are not dyadic): bitwise the fp64 sum
        assert torch.equal(got[:, :4].double(), ref[:, :4])


@pytest.mark.parametrize("order", (0, 1))
def test_scatter_other_orders(ops, order):
    for name in ("D257", "L"):
        ref, mag, cnt = scatter_reference(name, order)
        for det in (False, True):
            with mode(det):
                got = scatter(ops, name, order)
            ratio = V.worst_ratio(got, ref, P.scatter_bound(ref, mag, cnt, det))
            print(f"[voxel_plv scatter K={order} {name} {'det' if det else 'atomic'}] worst |err| / bound {ratio:.3f}")
            assert ratio <= 1.0


def test_deterministic_scatter_is_independent_of_run_and_sample_order(ops):
    for name in ("D1000", "L", "F"):
        p, dirs = P.scatter_inputs(name)[:2]
        rows = p.shape[0] // dirs.shape[0]
        perm = torch.from_numpy(proc_uniform((rows,), 4860, 1.0)).argsort()
        with mode(True):
            a, b, c = scatter(ops, name), scatter(ops, name), scatter(ops, name, perm=perm)
            d = scatter(ops, name, variant=2)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), name
        assert torch.equal(a.view(torch.int32), d.view(torch.int32)), name   # (nor of the table: only integers are added)


def test_a_too_small_deterministic_workspace_is_refused_before_anything_is_written(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    p, dirs, g, gs, S, gr = P.scatter_inputs("D257")
    assert dirs.shape[0] == 1
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    g_den, g_rgb = torch.full((S ** 3,), 3.0, device="cuda"), torch.full((S ** 3, 28), 3.0, device="cuda")
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        pc, rays, gc, gsc = p.cuda(), P.rays_of(dirs).cuda(), g.cuda(), gs.cuda()
        rc = lib.na_voxel_plv_sample_backward(ops._ptr(pc), ops._ptr(rays), 1, None, 257, ops._ptr(gc),
                                              ops._ptr(gsc), S, 4, gr, ops._ptr(g_den), ops._ptr(g_rgb), ops._stream())
        assert rc == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 29 * S ** 3} bytes".encode() in lib.na_last_error()
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0 and bool((g_den == 3.0).all()) and bool((g_rgb == 3.0).all())
        # through ops the process workspace is grown to fit (60.8 MB at S = 64, C = 28)
        config.set_deterministic(True)
        ops.voxel_plv_sample_backward(gc, gsc, 64, 4, gr, rays, pts=pc.reshape(257, 1, 3))
        assert config._det_ws.numel() >= 8 * 29 * 64 ** 3
    finally:
        config.set_deterministic(False)


# ------------------------------------------------------------------------------------------------------------ position gradient
@pytest.mark.parametrize("order", ORDERS)
def test_position_gradient(ops, order):
    """against the restatement's closed form, which is also checked against fp64 autograd of the restated lookup at interior points"""
    for S in (4, 16):
        den, rgb = P.grid_values(S, order)
        for N, (T, R) in SAMPLE_N.items():
            rays = P.rays_of(P.directions(R))
            pts = V.uniform_points(N, 4303)
            g_raw = torch.from_numpy(proc_uniform((N, 4), 4870 + N, 1.0))
            g_sh = torch.from_numpy(proc_uniform((N,), 4880 + N, 1.0))
            ref, bound = P.pts_grad_ref(pts, rays[:, 3:], den, rgb, g_raw, g_sh)
            got = ops.voxel_plv_sample_backward_pts(g_raw.cuda(), g_sh.cuda(), pts.reshape(T, R, 3).cuda(), rays.cuda(), den.cuda(), rgb.cuda(),
                                                    V.GRID_RADIUS)
            assert got.shape == (T, R, 3)
            ratio = V.worst_ratio(got, ref, bound)
            print(f"[voxel_plv pts grad K={order} S={S} N={N}] worst |err| / bound {ratio:.3f}")
            assert ratio <= 1.0, (S, N, ratio)
    # the closed form is the derivative of the restated lookup: central differences in fp64 on the cell's polynomial (the weights are
    # multilinear in xyz, so a finite difference of the restatement over the same cell is exact up to rounding)
    S, N, R = 16, 63, 9
    den, rgb = P.grid_values(S, order)
    rays = P.rays_of(P.directions(R))
    pts = V.uniform_points(N, 4304, amp=1.0)
    g_raw = torch.from_numpy(proc_uniform((N, 4), 4890, 1.0))
    g_sh = torch.from_numpy(proc_uniform((N,), 4891, 1.0))
    ids, xyz = V.cells(pts, S)
    grid = torch.cat([den, rgb], dim=-1).double().reshape(S ** 3, -1)[V.rows_of(ids, S)]
    Y = P.basis(rays[:, 3:], order)[0][torch.arange(N) % R]
    x = xyz.double().requires_grad_(True)
    pick = lambda v, pos: v if pos else 1 - v
    w = torch.stack([pick(x[:, 0], V.bit_i(u, 0)) * pick(x[:, 1], V.bit_i(u, 1)) * pick(x[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    val = (g_raw.double()[:, None, :] * grid[..., :4]).sum(-1) + g_sh.double()[:, None] * (Y[:, None, :] * grid[..., 4:]).sum(-1)
    (w * val).sum().backward()
    ref, _ = P.pts_grad_ref(pts, rays[:, 3:], den, rgb, g_raw, g_sh)
    assert float((x.grad / (V.GRID_RADIUS * 2 / S) - ref).abs().max()) <= 1e-9 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------------ fused render + operator route
RENDER_T = (1, 2, 63, 64, 65, 130)
RENDER_R = {1: (1,), 35: (5, 7), 257: (257,)}
ACTS = ("upshifted", "thin", "leaky_relu")
BGS = ("black", "white", "random")


def close(got, ref, what, tol=1e-4):
    for g, r, n in zip(got, ref, ("out", "alpha", "weights")):
        err = float((g.detach().cpu().double() - r).abs().max())
        print(f"[{what}] {n} max |err| {err:.2e}")
        assert g.shape == r.shape and err <= tol, (what, n, err)


@pytest.mark.parametrize("T", RENDER_T)
def test_render_one_launch_and_operator_route(ops, T):
    """1, 35 and 257 rays x the three backgrounds x the three activations (cycled so that each T sees all of them), order 4 and one
    other order per T; explicit points give the same bits as points formed in the kernel"""
    S = 16
    ts = torch.linspace(2.0, 6.0, T) if T > 1 else torch.tensor([4.0])
    for i, (R, shape) in enumerate(RENDER_R.items()):
        order = 4 if i != 1 else (T % 4)
        den, rgb = P.grid_values(S, order)
        dc, rc = den.cuda(), rgb.cuda()
        act, bg = ACTS[(i + T) % 3], BGS[(i + T // 2) % 3]
        rays = V.generic_rays(shape, 4730 + R)
        rand = torch.from_numpy(proc_uniform(shape + (1,), 4740 + R, 0.5)) + 0.5 if bg == "random" else None
        ref = P.render_ref(rays, ts, den, rgb, act, bg, rand)
        kbg = "black" if bg == "random" else bg
        got = ops.voxel_plv_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, kbg)
        viapts = ops.voxel_plv_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, kbg, pts=V.pts_of(rays, ts).cuda())
        for a, b in zip(got, viapts):
            assert torch.equal(a, b)
        if bg == "random":
            ops.sky_random(got[2], rand.cuda(), got[0])
        close(got, ref, f"voxel_plv_render K={order} T={T} R={R} {act} {bg}")
        raw, sh = ops.voxel_plv_sample(dc, rc, V.GRID_RADIUS, rays.cuda(), ts=ts.cuda())
        col = ops.pos_linear_combine(sh.unsqueeze(-1), ops.sigmoid(raw[..., 1:].contiguous(), act), 3)
        via_ops = ops.composite(raw[..., 0].contiguous(), col, ts.cuda(), rays.cuda(), bg=bg, rand=None if rand is None else rand.cuda())
        close(via_ops, ref, f"operator route K={order} T={T} R={R} {act} {bg}")
    out_only = ops.voxel_plv_render(rays.cuda(), ts.cuda(), dc, rc, V.GRID_RADIUS, act, "white", want_weights=False)
    assert out_only[1] is None and out_only[2] is None and out_only[0].shape == shape + (3,)


def build_model(g, device="cuda"):
    from nerf_atlas_amd import nerf, refl
    m = nerf.NeRFVoxel(resolution=int(g["S"]), t_near=float(g["near"]), t_far=float(g["far"]), steps=int(g["steps"]), bg=str(g["bg"]))
    m.set_refl(refl.PosLinearView(act=str(g["act"]), latent_size=0, out_features=3, voxel_order=4))
    m.load_state_dict(golden_params(g), strict=True)
    return m.to(device).eval()


class Spy:
    NAMES = ("voxel_plv_render", "voxel_plv_sample", "voxel_plv_sample_backward", "voxel_render", "voxel_sample", "composite")

    def __init__(self, monkeypatch, ops):
        self.calls = {n: 0 for n in self.NAMES}
        for n in self.NAMES:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, n, fn):
        def f(*a, **k):
            self.calls[n] += 1
            return fn(*a, **k)
        return f

    def take(self):
        c, self.calls = {k: v for k, v in self.calls.items() if v}, {n: 0 for n in self.NAMES}
        return c


@pytest.mark.parametrize("name", ("s64_black", "s16_ragged", "s4", "s2"))
def test_model_matches_the_reference_on_both_routes(ops, monkeypatch, name):
    """g27: out / alpha / weights within the project's 1e-4 on the one-launch and the operator route; the gradients of both grids within
    1e-4 of the largest entry of the reference's fp64 gradient (the bars tests/test_gpu_voxel.py applies to g23)"""
    g = load_golden(f"g27_voxel_plv_{name}")
    m = build_model(g)
    rays = g["rays"].cuda()
    ref = (g["out64"], g["alpha64"], g["weights64"])
    spy = Spy(monkeypatch, ops)
    with torch.no_grad():
        out = m(rays)
    assert spy.take() == {"voxel_plv_render": 1}
    assert torch.equal(m.ts.cpu(), g["ts"])
    close((out, m.alpha, m.weights), ref, f"{name} eval route")
    with torch.no_grad():
        pts = V.pts_of(g["rays"], g["ts"]).cuda()
        out_p = m.from_pts(pts, m.ts, rays[..., :3], rays[..., 3:], rays=rays)
    assert torch.equal(out_p, out) and spy.take() == {"voxel_plv_render": 1}
    out_t = m(rays)
    assert spy.take() == {"voxel_plv_sample": 1, "composite": 1} and out_t.requires_grad
    close((out_t, m.alpha, m.weights), ref, f"{name} operator route")
    out_t.square().sum().backward()
    assert spy.take().get("voxel_plv_sample_backward") == 1
    if "g_densities64" in g:
        for got, key in ((m.densities.grad, "g_densities64"), (m.rgb.grad, "g_rgb64")):
            want = g[key]
            err = float((got.cpu().double() - want).abs().max() / want.abs().max())
            print(f"[{name}] {key}: max |err| / largest entry {err:.2e} (the reference's own fp32: {g['g_dev'].tolist()})")
            assert got.shape == want.shape and err <= 1e-4, (name, key, err)


def test_tv_and_upsample_carry_28_channels(ops):
    """--voxel-tv-rgb and --voxel-upsample over the head's grid: the grid operators take C = 28 (they carry up to 32 channels)"""
    from nerf_atlas_amd import nerf
    g = load_golden("g27_voxel_plv_s4")
    m = build_model(g)
    tv = nerf.total_variation(m.rgb, samples=257)
    tv.backward()
    assert tv.dim() == 0 and float(tv) > 0 and m.rgb.grad.shape == (4, 4, 4, 28) and bool(torch.isfinite(m.rgb.grad).all())
    m.upsample(8)
    assert tuple(m.rgb.shape) == (8, 8, 8, 28) and m.resolution == 8
    with torch.no_grad():
        out = m(g["rays"].cuda())
    assert bool(torch.isfinite(out).all())


def test_a_training_step_lowers_the_loss(ops):
    from nerf_atlas_amd import train
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "pos-linear-view", "--voxel-refl-order", "4", "--near", "2", "--far", "6",
                                 "--steps", "16"])
    torch.manual_seed(0)
    m = train.load_model(args).train()
    opt = train.NaAdam(m.parameters(), lr=5e-2)
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (m(rays) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("[voxel plv train] loss", losses[0], "->", losses[-1])
    assert losses[-1] < 0.5 * losses[0] and all(l == l for l in losses)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    den, rgb = P.grid_values(4, 4)
    dc, rc = den.cuda(), rgb.cuda()
    rays = P.rays_of(P.directions(8)).cuda()
    pts = V.uniform_points(8).cuda()
    raw, sh, g_pts = torch.zeros(8, 4).cuda(), torch.zeros(8).cuda(), torch.zeros(8, 3).cuda()
    p, st = ops._ptr, ops._stream()
    with pytest.raises(ValueError):
        ops.voxel_plv_sample(dc, rc, 1.3, rays.cpu(), pts=pts)                      # host tensors
    with pytest.raises(ValueError, match="channels"):
        ops.voxel_plv_sample(dc, torch.zeros(4, 4, 4, 5).cuda(), 1.3, rays, pts=pts)  # C = 5: no order
    sample = lambda **k: lib.na_voxel_plv_sample(*[k.get(n, d) for n, d in (("pts", p(pts)), ("rays", p(rays)), ("R", 8), ("ts", None), ("T", 1),
                                                                              ("den", p(dc)), ("rgb", p(rc)), ("S", 4), ("order", 4), ("gr", 1.3),
                                                                              ("raw", p(raw)), ("sh", p(sh)))], st)
    assert sample() == 0
    assert sample(order=5) == NA_EINVAL and b"order 5" in lib.na_last_error()
    assert sample(order=-1) == NA_EINVAL
    assert sample(S=3) == NA_EINVAL and b"resolution 3" in lib.na_last_error()
    assert sample(gr=0.0) == NA_EINVAL and b"grid_radius" in lib.na_last_error()
    assert sample(T=0) == NA_EINVAL
    assert sample(R=0) == 0                                                          # nothing to do: no launch, no pointer is read
    for name in ("rays", "den", "rgb", "raw", "sh"):
        assert sample(**{name: None}) == NA_ENULL and {"den": b"densities"}.get(name, name.encode()) in lib.na_last_error(), name
    assert sample(pts=None) == NA_ENULL and b"pts and ts" in lib.na_last_error()
    odd = torch.zeros(33).cuda()[1:]
    assert sample(raw=ops._ptr(odd)) == NA_EINVAL and b"16-byte" in lib.na_last_error()
    off = torch.zeros(4 * 4 * 4 * 28 + 1).cuda()[1:]
    assert sample(rgb=ops._ptr(off)) == NA_EINVAL and b"16-byte" in lib.na_last_error()
    off7 = torch.zeros(4 * 4 * 4 * 7 + 1).cuda()[1:]
    assert sample(rgb=ops._ptr(off7), order=1) == 0                                 # 28-byte rows: 4-byte loads, any alignment
    g_den, g_rgb = torch.zeros(64).cuda(), torch.zeros(64, 28).cuda()
    bwd = lambda **k: lib.na_voxel_plv_sample_backward_variant(p(pts), p(rays), 8, None, 1, k.get("g_raw", p(raw)), k.get("g_sh", p(sh)), 4,
                                                               k.get("order", 4), 1.3, p(g_den), k.get("g_rgb", p(g_rgb)),
                                                               k.get("variant", 1), st)
    assert bwd() == 0 and bwd(variant=2) == 0
    assert bwd(variant=3) == NA_EINVAL and bwd(order=7) == NA_EINVAL
    assert bwd(g_sh=None) == NA_ENULL and b"g_sh" in lib.na_last_error()
    assert bwd(g_rgb=None) == NA_ENULL and b"g_rgb" in lib.na_last_error()
    gp = lambda **k: lib.na_voxel_plv_sample_backward_pts(k.get("pts", p(pts)), p(rays), k.get("R", 8), k.get("N", 8), p(dc), p(rc), p(raw), p(sh), 4,
                                                          k.get("order", 4), 1.3, k.get("g_pts", p(g_pts)), st)
    assert gp() == 0 and gp(N=0) == 0
    assert gp(N=7) == NA_EINVAL                                                      # not a multiple of R
    assert gp(order=9) == NA_EINVAL
    assert gp(pts=None) == NA_ENULL and b"pts" in lib.na_last_error()
    assert gp(g_pts=None) == NA_ENULL and b"g_pts" in lib.na_last_error()
    ts = torch.linspace(2, 6, 5).cuda()
    out = torch.zeros(8, 3).cuda()
    rend = lambda **k: lib.na_voxel_plv_render(k.get("rays", p(rays)), None, k.get("R", 8), k.get("ts", p(ts)), 5, p(dc), p(rc), k.get("S", 4),
                                               k.get("order", 4), 1.3, k.get("act", 4), k.get("bg", 0), None, None, k.get("out", p(out)), st)
    assert rend() == 0 and rend(R=0) == 0
    assert rend(order=5) == NA_EINVAL and rend(S=6000) == NA_EINVAL
    assert rend(act=99) == -3 and rend(bg=2) == -3
    assert rend(ts=None) == NA_ENULL and b"ts" in lib.na_last_error()
    assert rend(out=None) == NA_ENULL and b"out" in lib.na_last_error()
    torch.cuda.synchronize()
