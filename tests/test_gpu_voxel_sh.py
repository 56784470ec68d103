"""--model voxel --refl-kind sph-har --voxel-sh-order K on the GPU (csrc/voxel.hip): the lookup with the head, its scatter in both
accumulation modes and both table geometries, its position gradient and the one-launch eval route.  Operators against
tests/voxel_sh_ref.py (membership fixed in fp32, everything behind it in fp64) within its derived bounds (worst |err| / bound printed; an
entry with bound 0 must be exact); the ties to the pinned kernels and the eval route against the operator composition bit for bit."""
import contextlib
import functools

import pytest
import torch

import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

NA_EINVAL, NA_ENULL, NA_EWORKSPACE = -1, -2, -5   # include/nerf_atlas_amd.h
SAMPLE_N = {1: (1, 1), 63: (7, 9), 65: (5, 13), 257: (1, 257), 1000: (8, 125)}   # N: (T, R)
SCATTER_CASES = ("A", "B", "D257", "D1000", "L", "G")   # A: every sample in one cell; D1000 at S = 16: more rows than a table holds
GR = V.GRID_RADIUS


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


def check_sample(ops, pts, rays, den, rgb, order, what, ts=None):
    """pts [T,R,3] (explicit when ts is None, else what the kernel forms from rays x ts)"""
    raw, mag = H.sample_ref(pts.reshape(-1, 3), rays[:, 3:], den, rgb, order)
    kw = {"pts": pts.cuda()} if ts is None else {"ts": ts.cuda()}
    got = ops.voxel_sh_sample(den.cuda(), rgb.cuda(), order, GR, rays.cuda(), **kw)
    assert got.shape == pts.shape[:-1] + (4,)
    ratio = V.worst_ratio(got, raw, H.sample_bound(mag, order))
    print(f"[voxel_sh_sample K={order} {what}] worst |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)
    return got


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("order", H.ORDERS)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_sample_both_position_forms(ops, S, order):
    """uniform points in +-2.5 (inside and extrapolated: sign-alternating weights) at every ragged size, explicit and formed in the kernel;
    directions un-normalised, one zero, one on an axis, two on the cancellation cones of x^2 - y^2 and 35 z^4 - 30 z^2 + 3"""
    den, rgb = H.grid_values(S, order)
    for N, (T, R) in SAMPLE_N.items():
        rays = H.rays_of(H.directions(R))
        check_sample(ops, V.uniform_points(N).reshape(T, R, 3), rays, den, rgb, order, f"S={S} N={N} pts")
        ts = torch.linspace(0.0, 2.5, T) if T > 1 else torch.tensor([1.25])
        a = check_sample(ops, V.pts_of(rays, ts), rays, den, rgb, order, f"S={S} N={N} rays x ts", ts=ts)
        b = ops.voxel_sh_sample(den.cuda(), rgb.cuda(), order, GR, rays.cuda(), pts=V.pts_of(rays, ts).cuda())
        assert torch.equal(a, b)   # the two position forms: the same bits


@pytest.mark.parametrize("order", H.ORDERS)
def test_sample_on_cell_faces_and_around_zero(ops, order):
    for S in (2, 4, 16):
        den, rgb = H.grid_values(S, order)
        for name, pts in (("lattice", V.lattice_points(S)), ("zero", V.zero_points())):
            n = pts.shape[0]
            R = next(r for r in (5, 3, 1) if n % r == 0)
            check_sample(ops, pts.reshape(n // R, R, 3), H.rays_of(H.directions(R)), den, rgb, order, f"S={S} {name}")


@pytest.mark.parametrize("order", H.ORDERS)
def test_bit_for_bit_tie_to_the_pinned_kernels(ops, order):
    """channel block c of an SH grid = the coefficient block of a pos-linear-view grid: raw[:, 1 + c] is na_voxel_plv_sample's sh, bit for
    bit; with all coefficients zero the density column is na_voxel_sample's bits"""
    S, T, R = 16, 8, 125
    NK = H.nk(order)
    den, rgb = H.grid_values(S, order)
    rays = H.rays_of(H.directions(R)).cuda()
    pts = V.uniform_points(T * R).reshape(T, R, 3).cuda()
    raw = ops.voxel_sh_sample(den.cuda(), rgb.cuda(), order, GR, rays, pts=pts)
    for c in range(3):
        plv = torch.cat([torch.zeros(S, S, S, 3), rgb[..., c * NK:(c + 1) * NK]], dim=-1).contiguous()
        _, sh = ops.voxel_plv_sample(den.cuda(), plv.cuda(), GR, rays, pts=pts)
        assert torch.equal(raw[..., 1 + c].contiguous().view(torch.int32), sh.view(torch.int32)), (order, c)
    zero = ops.voxel_sh_sample(den.cuda(), torch.zeros_like(rgb).cuda(), order, GR, rays, pts=pts)
    ref = ops.voxel_sample(den.cuda(), torch.zeros(S, S, S, 3).cuda(), GR, pts=pts)
    assert torch.equal(zero[..., 0].contiguous().view(torch.int32), ref[..., 0].contiguous().view(torch.int32))
    assert not bool(zero[..., 1:].any())


def _guarded(t, pad=64, fill=-777.0):
    """t inside a buffer with `pad` sentinel floats on either side (16-byte aligned data); returns (view, check)"""
    buf = torch.full((t.numel() + 2 * pad,), fill, device="cuda")
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return view, lambda: bool((buf[:pad] == fill).all()) and bool((buf[pad + t.numel():] == fill).all())


@pytest.mark.parametrize("order", (3, 4))
def test_non_finite_coordinates_are_nan_in_their_sample_only_and_guards_hold(ops, order):
    """a NaN and an Inf coordinate in every operator: NaN in that sample's outputs (and its <= 8 grid rows) only; guard regions around
    every buffer the kernels read or write are unchanged"""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    S, T, R = 16, 9, 29
    N, C = T * R, H.channels(order)
    den, rgb = H.grid_values(S, order)
    rays = H.rays_of(H.directions(R))
    pts = V.uniform_points(N, 4301).clone()
    bad = {5: (1, float("nan")), 70: (0, float("inf")), 200: (2, float("-inf")), N - 1: (0, float("nan"))}
    for n, (a, v) in bad.items():
        pts[n, a] = v
    g_raw = H.grads(N)
    bufs = {k: _guarded(v.cuda()) for k, v in dict(pts=pts, rays=rays, den=den, rgb=rgb, g_raw=g_raw, raw=torch.zeros(N, 4),
                                                    g_pts=torch.zeros(N, 3), g_den=torch.zeros(S ** 3), g_rgb=torch.zeros(S ** 3, C)).items()}
    b = {k: v[0] for k, v in bufs.items()}
    p = ops._ptr
    assert lib.na_voxel_sh_sample(p(b["pts"]), p(b["rays"]), R, None, T, p(b["den"]), p(b["rgb"]), S, C, order, GR, p(b["raw"]), ops._stream()) == 0
    assert lib.na_voxel_sh_sample_backward_pts(p(b["pts"]), p(b["rays"]), R, N, p(b["den"]), p(b["rgb"]), p(b["g_raw"]), S, C, order, GR,
                                               p(b["g_pts"]), ops._stream()) == 0
    assert lib.na_voxel_sh_sample_backward(p(b["pts"]), p(b["rays"]), R, None, T, p(b["g_raw"]), S, C, order, GR, p(b["g_den"]), p(b["g_rgb"]),
                                           ops._stream()) == 0
    torch.cuda.synchronize()
    assert all(check() for _, check in bufs.values()), [k for k, (_, check) in bufs.items() if not check()]
    for k in ("raw", "g_pts"):
        rows = torch.isnan(b[k]).any(dim=-1).cpu()
        assert sorted(torch.nonzero(rows).flatten().tolist()) == sorted(bad) and bool(torch.isnan(b[k].cpu()[rows]).all()), k
    raw, mag = H.sample_ref(pts, rays[:, 3:], den, rgb, order)
    assert V.worst_ratio(b["raw"], raw, H.sample_bound(mag, order)) <= 1.0
    ref, mag, cnt = H.scatter_ref(pts, rays[:, 3:], g_raw, S, order)
    got = torch.cat([b["g_den"].reshape(-1, 1), b["g_rgb"]], dim=-1)
    assert 0 < int(torch.isnan(ref[:, 0]).sum()) <= 8 * len(bad)
    assert V.worst_ratio(got, ref, H.scatter_bound(ref, mag, cnt, False)) <= 1.0


# ------------------------------------------------------------------------------------------------------------ scatter
def scatter(ops, name, order, perm=None, variant=None):
    p, dirs, g, S, gr = H.scatter_inputs(name)
    R = dirs.shape[0]
    if perm is not None:   # a permutation of the samples that keeps every sample's ray: whole rows of R are permuted
        idx = (perm[:, None] * R + torch.arange(R)[None]).reshape(-1)
        p, g = p[idx], g[idx]
    gd, gc = ops.voxel_sh_sample_backward(g.cuda(), S, order, gr, H.rays_of(dirs).cuda(), pts=p.reshape(-1, R, 3).cuda(), variant=variant)
    assert gd.shape == (S, S, S, 1) and gc.shape == (S, S, S, H.channels(order))
    return torch.cat([gd, gc], dim=-1).reshape(S ** 3, -1).cpu()


@functools.lru_cache(maxsize=None)
def scatter_reference(name, order):
    p, dirs, g, S, gr = H.scatter_inputs(name)
    return H.scatter_ref(p, dirs, g, S, order, gr)


@pytest.mark.parametrize("variant", (1, 2), ids=("rows-in-lds", "channel-passes"))
@pytest.mark.parametrize("det", (False, True), ids=("atomics", "fixed-point"))
@pytest.mark.parametrize("name", SCATTER_CASES)
def test_scatter_every_entry_inside_its_bound(ops, name, det, variant):
    """voxel_ref's scatter shapes at C = 75 (76 sums per row): duplicates (A: all samples in one cell, the largest cnt; B; the lattice set L), more
    distinct cells in a workgroup's run than its table holds (D1000: up to 2048 cells in one round against 64 .. 512 rows); both modes,
    both table geometries"""
    ref, mag, cnt = scatter_reference(name, 4)
    with mode(det):
        got = scatter(ops, name, 4, variant=variant)
    ratio = V.worst_ratio(got, ref, H.scatter_bound(ref, mag, cnt, det))
    print(f"[voxel_sh scatter {name} {'det' if det else 'atomic'} variant {variant}] worst |err| / bound {ratio:.3f}, most addends in one "
          f"entry {int(cnt.max())}")
    assert ratio <= 1.0, (name, det, variant, ratio)
    if name == "G":   # exact arithmetic in the density sum (the basis values are not dyadic): bitwise the fp64 sum
        assert torch.equal(got[:, 0].double(), ref[:, 0])


@pytest.mark.parametrize("order", (0, 1, 2, 3))
def test_scatter_other_orders(ops, order):
    for name in ("D257", "L"):
        ref, mag, cnt = scatter_reference(name, order)
        for det in (False, True):
            for variant in (1, 2):
                with mode(det):
                    got = scatter(ops, name, order, variant=variant)
                ratio = V.worst_ratio(got, ref, H.scatter_bound(ref, mag, cnt, det))
                print(f"[voxel_sh scatter K={order} {name} {'det' if det else 'atomic'} variant {variant}] worst |err| / bound {ratio:.3f}")
                assert ratio <= 1.0, (order, name, det, variant, ratio)


@pytest.mark.parametrize("order", H.ORDERS)
@pytest.mark.parametrize("S", (2, 4))
def test_scatter_on_the_smallest_grids(ops, S, order):
    """S = 2 and 4: every row of the grid is hit many times (257 samples inside and outside over 8 / 64 rows), every order, both modes,
    both geometries"""
    N, R = 257, 1
    pts, g = V.uniform_points(N, 4305), H.grads(N, 5670)
    dirs = torch.tensor([[0.3, -1.1, 0.7]])
    ref, mag, cnt = H.scatter_ref(pts, dirs, g, S, order)
    for det in (False, True):
        for variant in (1, 2):
            with mode(det):
                gd, gc = ops.voxel_sh_sample_backward(g.cuda(), S, order, GR, H.rays_of(dirs).cuda(), pts=pts.reshape(N, R, 3).cuda(),
                                                      variant=variant)
            got = torch.cat([gd, gc], dim=-1).reshape(S ** 3, -1)
            ratio = V.worst_ratio(got, ref, H.scatter_bound(ref, mag, cnt, det))
            print(f"[voxel_sh scatter S={S} K={order} {'det' if det else 'atomic'} variant {variant}] worst |err| / bound {ratio:.3f}")
            assert ratio <= 1.0, (S, order, det, variant, ratio)


@pytest.mark.parametrize("order", (1, 4))
def test_deterministic_scatter_is_independent_of_run_sample_order_and_geometry(ops, order):
    for name in ("D1000", "L"):
        p, dirs = H.scatter_inputs(name)[:2]
        rows = p.shape[0] // dirs.shape[0]
        perm = torch.from_numpy(proc_uniform((rows,), 4860, 1.0)).argsort()
        with mode(True):
            a, b, c = scatter(ops, name, order), scatter(ops, name, order), scatter(ops, name, order, perm=perm)
            d, e = scatter(ops, name, order, variant=1), scatter(ops, name, order, variant=2)
        for other in (b, c, d, e):
            assert torch.equal(a.view(torch.int32), other.view(torch.int32)), name


def test_a_too_small_deterministic_workspace_is_refused_before_anything_is_written(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    p, dirs, g, S, gr = H.scatter_inputs("D257")
    assert dirs.shape[0] == 1
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    g_den, g_rgb = torch.full((S ** 3,), 3.0, device="cuda"), torch.full((S ** 3, 75), 3.0, device="cuda")
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        pc, rays, gc = p.cuda(), H.rays_of(dirs).cuda(), g.cuda()
        for variant in (1, 2):
            rc = lib.na_voxel_sh_sample_backward_variant(ops._ptr(pc), ops._ptr(rays), 1, None, 257, ops._ptr(gc), S, 75, 4, gr, ops._ptr(g_den),
                                                         ops._ptr(g_rgb), variant, ops._stream())
            assert rc == NA_EWORKSPACE and f"deterministic workspace 4096 < {8 * 76 * S ** 3} bytes".encode() in lib.na_last_error()
        torch.cuda.synchronize()
        assert int(ws.count_nonzero()) == 0 and bool((g_den == 3.0).all()) and bool((g_rgb == 3.0).all())
        config.set_deterministic(True)   # through ops the process workspace is grown to fit
        ops.voxel_sh_sample_backward(gc, 16, 4, gr, rays, pts=pc.reshape(257, 1, 3))
        assert config._det_ws.numel() >= 8 * 76 * 16 ** 3
    finally:
        config.set_deterministic(False)


# ------------------------------------------------------------------------------------------------------------ position gradient
@pytest.mark.parametrize("order", H.ORDERS)
def test_position_gradient(ops, order):
    for S in (2, 4, 16):
        den, rgb = H.grid_values(S, order)
        for N, (T, R) in SAMPLE_N.items():
            rays = H.rays_of(H.directions(R))
            pts = V.uniform_points(N, 4303)
            g_raw = H.grads(N, 5650)
            ref, bound = H.pts_grad_ref(pts, rays[:, 3:], den, rgb, g_raw, order)
            got = ops.voxel_sh_sample_backward_pts(g_raw.cuda(), pts.reshape(T, R, 3).cuda(), rays.cuda(), den.cuda(), rgb.cuda(), order, GR)
            assert got.shape == (T, R, 3)
            ratio = V.worst_ratio(got, ref, bound)
            print(f"[voxel_sh pts grad K={order} S={S} N={N}] worst |err| / bound {ratio:.3f}")
            assert ratio <= 1.0, (S, N, ratio)


# ------------------------------------------------------------------------------------------------------------ eval route
def composition(ops, rays, ts, den, rgb, order, act, bg, pts=None):
    kw = {"ts": ts} if pts is None else {"pts": pts}
    raw = ops.voxel_sh_sample(den, rgb, order, GR, rays, **kw)
    return ops.composite(raw[..., 0].contiguous(), ops.sigmoid(raw[..., 1:].contiguous(), act), ts, rays, bg=bg)


@pytest.mark.parametrize("T", (1, 17, 80))
@pytest.mark.parametrize("order", H.ORDERS)
def test_eval_route_equals_the_operator_composition_bit_for_bit(ops, T, order):
    """lookup -> activation -> compositing in one launch: the same bits as the three launches, for 1, 35 and 257 rays, both backgrounds,
    points formed in the kernel and explicit ones; and the fp64 model within the project's 1e-4"""
    S = 16
    den, rgb = H.grid_values(S, order)
    dc, rc = den.cuda(), rgb.cuda()
    ts = torch.linspace(2.0, 6.0, T) if T > 1 else torch.tensor([4.0])
    for i, R in enumerate((1, 35, 257)):
        act, bg = ("upshifted", "thin", "leaky_relu")[(i + T) % 3], ("black", "white")[(i + order) % 2]
        rays = V.generic_rays((R,), 4730 + R)
        for pts in (None, V.uniform_points(T * R, 5660).reshape(T, R, 3).cuda()):
            got = ops.voxel_sh_render(rays.cuda(), ts.cuda(), dc, rc, order, GR, act, bg, pts=pts)
            ref = composition(ops, rays.cuda(), ts.cuda(), dc, rc, order, act, bg, pts)
            for g, r, n in zip(got, ref, ("out", "alpha", "weights")):
                assert g.shape == r.shape and torch.equal(g, r), (T, R, order, n, pts is None, float((g - r).abs().max()))
        want = H.render_ref(rays, ts, den, rgb, order, act, bg)
        got = ops.voxel_sh_render(rays.cuda(), ts.cuda(), dc, rc, order, GR, act, bg)
        for g, r, n in zip(got, want, ("out", "alpha", "weights")):
            err = float((g.cpu().double() - r).abs().max())
            assert err <= 1e-4, (T, R, order, n, err)


def test_model_routes_and_a_training_step(ops, monkeypatch):
    """NeRFVoxel picks the head's operators on both routes; 20 Adam steps lower the loss"""
    from nerf_atlas_amd import train
    calls = []
    for n in ("voxel_sh_render", "voxel_sh_sample", "voxel_sh_sample_backward", "voxel_render", "voxel_sample", "voxel_plv_sample"):
        monkeypatch.setattr(ops, n, (lambda n, fn: lambda *a, **k: (calls.append(n), fn(*a, **k))[1])(n, getattr(ops, n)))
    args = train.args_from_argv(["--model", "voxel", "--refl-kind", "sph-har", "--voxel-sh-order", "2", "--near", "2", "--far", "6", "--steps", "16"])
    torch.manual_seed(0)
    m = train.load_model(args).eval()
    rays = V.generic_rays((2, 8, 8), 4750).cuda()
    with torch.no_grad():
        out = m(rays)
    assert calls == ["voxel_sh_render"] and out.shape == (2, 8, 8, 3)
    m.train()
    opt = train.NaAdam(m.parameters(), lr=5e-2)
    target = torch.full((2, 8, 8, 3), 0.25, device="cuda")
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = (m(rays) - target).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert set(calls[1:]) == {"voxel_sh_sample", "voxel_sh_sample_backward"}
    print("[voxel sh train] loss", losses[0], "->", losses[-1])
    assert losses[-1] < 0.5 * losses[0] and all(l == l for l in losses)


# ------------------------------------------------------------------------------------------------------------ argument checks
def test_wrong_channel_count_and_misaligned_grid_leave_the_outputs_untouched(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    p, st = ops._ptr, ops._stream()
    S, R = 4, 8
    rays = H.rays_of(H.directions(R)).cuda()
    pts = V.uniform_points(R).cuda()
    ts = torch.linspace(2, 6, 5).cuda()
    den = H.grid_values(S, 1)[0].cuda()
    raw, g_pts, out = (torch.full(s, 5.0, device="cuda") for s in ((R, 4), (R, 3), (R, 3)))
    g_den, g_rgb = torch.full((S ** 3,), 5.0, device="cuda"), torch.full((S ** 3, 75), 5.0, device="cuda")
    g_raw = H.grads(R).cuda()

    def calls(rgb, C, order):
        return (lib.na_voxel_sh_sample(p(pts), p(rays), R, None, 1, p(den), rgb, S, C, order, GR, p(raw), st),
                lib.na_voxel_sh_sample_backward_pts(p(pts), p(rays), R, R, p(den), rgb, p(g_raw), S, C, order, GR, p(g_pts), st),
                lib.na_voxel_sh_render(p(rays), None, R, p(ts), 5, p(den), rgb, S, C, order, GR, 4, 0, None, None, p(out), st))

    grid = torch.zeros(S ** 3 * 75 + 1, device="cuda")
    # C names another head's row: 12 = the pos-linear-view head's at order 2, 3 = the RGB head's
    for C, order in ((12, 2), (3, 1), (75, 3), (27, 5), (27, -1)):
        assert calls(p(grid), C, order) == (NA_EINVAL,) * 3, (C, order)
        assert lib.na_voxel_sh_sample_backward(p(pts), p(rays), R, None, 1, p(g_raw), S, C, order, GR, p(g_den), p(g_rgb), st) == NA_EINVAL
    assert b"3 (order + 1)^2" in lib.na_last_error() or b"order" in lib.na_last_error()
    # rows read 16 bytes at a time (orders 1 and 3) need an aligned grid; the other orders take any
    off = grid[1:]
    for order in (1, 3):
        assert calls(p(off), H.channels(order), order) == (NA_EINVAL,) * 3 and b"16-byte" in lib.na_last_error()
    torch.cuda.synchronize()
    for t in (raw, g_pts, out, g_den, g_rgb):
        assert bool((t == 5.0).all())
    for order in (0, 2, 4):
        assert calls(p(off), H.channels(order), order) == (0,) * 3
    assert lib.na_voxel_sh_sample_backward_variant(p(pts), p(rays), R, None, 1, p(g_raw), S, 75, 4, GR, p(g_den), p(g_rgb), 3, st) == NA_EINVAL
    assert lib.na_voxel_sh_sample(p(pts), None, R, None, 1, p(den), p(grid), S, 75, 4, GR, p(raw), st) == NA_ENULL
    with pytest.raises(ValueError, match="channels"):
        ops.voxel_sh_sample(den, torch.zeros(S, S, S, 12).cuda(), 2, GR, rays, pts=pts)
    with pytest.raises(ValueError, match="order"):
        ops.voxel_sh_sample(den, torch.zeros(S, S, S, 12).cuda(), 7, GR, rays, pts=pts)
    # a contiguous view at an odd offset is copied by ops, not refused
    view = off[:S ** 3 * 12].view(S, S, S, 12)
    a = ops.voxel_sh_sample(den, view, 1, GR, rays, pts=pts)
    assert torch.equal(a, ops.voxel_sh_sample(den, view.clone(), 1, GR, rays, pts=pts))
    torch.cuda.synchronize()
