"""NeRFVoxel.sparsify on the GPU (csrc/voxel_sparse.hip): the liveness table and the sample flags against their exact
restatement (tests/voxel_sparse_ref.py), the sparse renderer bit for bit against the dense renderers where the two must agree (a table of
ones; a grid whose dead voxels already render to alpha 0), against the fp64 restatement within its bounds on the edge set of the
compaction (worst |err| / bound printed), NaN containment, every lane count, and the argument checks."""
import pytest
import torch

import voxel_fine_ref as F
import voxel_ref as V
import voxel_sparse_ref as X

pytestmark = pytest.mark.gpu

NA_EINVAL, NA_ENULL, NA_EUNSUPPORTED = -1, -2, -3   # include/nerf_atlas_amd.h
GR = V.GRID_RADIUS
HEADS = (("rgb", -1), ("plv", 0), ("plv", 4), ("sh", 0), ("sh", 4))
HEAD_IDS = [f"{h}{'' if k < 0 else k}" for h, k in HEADS]
MS = (1, 2, 3, 15, 16, 17, 33, 65)
RS = (1, 3, 4, 5, 257)
ACTS = ("upshifted", "thin")
MID = X.MID


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def shapes():
    """(S, M, R, act, bg): every M, every R, both S, activations and backgrounds"""
    return [((4, 6)[i % 2], MS[i % len(MS)], RS[i % len(RS)], ACTS[(i // 2) % 2], ("black", "white")[(i // 3) % 2]) for i in range(10)]


def rayts_render(ops, head, order, rays, ts_ray, den, rgb, act, bg):
    if head == "rgb":
        return ops.voxel_render_rayts(rays, ts_ray, den, rgb, GR, act, bg)
    if head == "plv":
        return ops.voxel_plv_render_rayts(rays, ts_ray, den, rgb, GR, act, bg)
    return ops.voxel_sh_render_rayts(rays, ts_ray, den, rgb, order, GR, act, bg)


def shared_render(ops, head, order, rays, ts, den, rgb, act, bg):
    if head == "rgb":
        return ops.voxel_render(rays, ts, den, rgb, GR, act, bg)
    if head == "plv":
        return ops.voxel_plv_render(rays, ts, den, rgb, GR, act, bg)
    return ops.voxel_sh_render(rays, ts, den, rgb, order, GR, act, bg)


def sparse(ops, head, order, rays, ts, den, rgb, live, act, bg, **kw):
    return ops.voxel_sparse_render(head, rays, ts, den, rgb, live, GR, order, act, bg, **kw)


# ------------------------------------------------------------------------------------------------------------ 1. table
@pytest.mark.parametrize("S", (4, 6, 16))
def test_live_table_and_count_are_the_restatement(ops, S):
    den, _ = V.grid_values(S)
    odd = den.clone()
    odd[1, 2, 3, 0], odd[S - 1, S - 1, S - 1, 0], odd[0, 0, 0, 0], odd[2, 0, 1, 0] = float("nan"), float("inf"), -float("inf"), float("nan")
    for grid, thresh in ((den, 0), (den, MID), (den, 0.3), (den, 10.0), (odd, 0), (odd, MID), (odd, 10.0)):
        live, count = ops.voxel_live_table(grid.cuda(), thresh)
        want = X.table_of(grid, thresh)
        assert live.dtype == torch.uint8 and live.shape == (S, S, S) and torch.equal(live.cpu(), want), (S, thresh)
        assert count.dtype == torch.int64 and int(count) == int(want.sum()), (S, thresh, int(count), int(want.sum()))
    assert bool(X.table_of(den, 0).all()) and not bool(X.table_of(den, 10.0).any()) and 0 < int(X.table_of(den, MID).sum()) < S ** 3
    assert int(X.table_of(odd, 10.0).sum()) > 0                                    # the NaN and +Inf voxels stay
    live, count = ops.voxel_live_table(den.cuda().reshape(S, S, S), MID, want_count=False)
    assert count is None and torch.equal(live.cpu(), X.table_of(den, MID))


# ------------------------------------------------------------------------------------------------------------ 2. flags
def test_live_samples_equal_the_reference_flags(ops):
    for S in (4, 6):
        live = X.table_of(V.grid_values(S)[0], MID)
        pts = torch.cat([V.lattice_points(S), V.uniform_points(1000, 8700 + S, 2.5), V.zero_points(),
                         torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [0.3, 0.1, -float("inf")]])]).contiguous()
        got = ops.voxel_live_samples(live.cuda(), GR, pts=pts.cuda())
        want = X.flags_of(pts, live)
        assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got.cpu().bool(), want), S
        assert bool(want[-3:].all()) and 0 < int(want.sum()) < want.numel()
        for _, M, R, _, _ in shapes():
            rays, rows = X.mixed_rays(R), X.mixed_rows(R, M)
            got = ops.voxel_live_samples(live.cuda(), GR, rays=rays.cuda(), ts=rows.cuda())
            want = X.flags_of(F.pts_rayts(rays, rows).reshape(-1, 3), live).reshape(M, R)
            assert got.shape == (M, R) and torch.equal(got.cpu().bool(), want), (S, M, R, "per-ray rows")
            ts = rows[R // 2].contiguous()
            got = ops.voxel_live_samples(live.cuda(), GR, rays=rays.cuda(), ts=ts.cuda())
            want = X.flags_of(V.pts_of(rays, ts).reshape(-1, 3), live).reshape(M, R)
            assert got.shape == (M, R) and torch.equal(got.cpu().bool(), want), (S, M, R, "shared row")
    rays = V.generic_rays((2, 3, 5), 8710).cuda()
    assert ops.voxel_live_samples(live.cuda(), GR, rays=rays, ts=torch.linspace(2, 6, 7).cuda()).shape == (7, 2, 3, 5)


def test_mask_rows(ops):
    g = torch.Generator().manual_seed(3)
    for N, C in ((1, 4), (257, 4), (1000, 1), (63, 5)):
        x = torch.randn(N, C, generator=g).cuda()
        flags = (torch.rand(N, generator=g) < 0.5).to(torch.uint8).cuda()
        for fill in (ops.VOXEL_DEAD_DENSITY, 0.0):
            want = x.clone()
            want[flags == 0] = 0.0
            want[flags == 0, 0] = fill
            assert torch.equal(ops.voxel_mask_rows(x, flags, fill), want), (N, C, fill)
        assert torch.equal(ops.voxel_mask_rows(x, torch.ones_like(flags), -1e30), x)
        y = x.clone()
        assert ops.voxel_mask_rows(y, flags, 0.0, out=y) is y and torch.equal(y, want)   # in place
    x = torch.randn(5, 7, generator=g).cuda()   # a column: one value per row
    flags = (torch.rand(5, 7, generator=g) < 0.5).to(torch.uint8).cuda()
    assert torch.equal(ops.voxel_mask_rows(x, flags, 0.0), x * flags)
    # the dead density renders to nothing
    assert float(torch.nn.functional.softplus(torch.tensor(ops.VOXEL_DEAD_DENSITY) - 1)) == 0.0


# ------------------------------------------------------------------------------------------------------------ 3. / 4. trivial tables
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_a_table_of_ones_gives_the_dense_renderers_bit_for_bit(ops, head, order):
    for S, M, R, act, bg in shapes():
        den, rgb = (g.cuda() for g in X.grids(head, order, S))
        ones = torch.ones(S, S, S, dtype=torch.uint8, device="cuda")
        rays, rows = X.mixed_rays(R).cuda(), X.mixed_rows(R, M).cuda()
        want = rayts_render(ops, head, order, rays, rows, den, rgb, act, bg)
        got = sparse(ops, head, order, rays, rows, den, rgb, ones, act, bg)
        for g, w, n in zip(got, want, ("out", "alpha", "weights")):
            assert g.shape == w.shape and torch.equal(g, w), (S, M, R, act, bg, n, "per-ray rows")
        ts = rows[R // 2].contiguous()
        want = shared_render(ops, head, order, rays, ts, den, rgb, act, bg)
        got = sparse(ops, head, order, rays, ts, den, rgb, ones, act, bg)
        for g, w, n in zip(got, want, ("out", "alpha", "weights")):
            assert g.shape == w.shape and torch.equal(g, w), (S, M, R, act, bg, n, "shared row")


@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_a_table_of_zeros_renders_the_background_alone(ops, head, order):
    for S, M, R, act, bg in shapes():
        den, rgb = (g.cuda() for g in X.grids(head, order, S))
        zeros = torch.zeros(S, S, S, dtype=torch.uint8, device="cuda")
        rays, rows = V.generic_rays((R,), 8720 + R).cuda(), X.mixed_rows(R, M).cuda()
        for ts in (rows, rows[0].contiguous()):
            out, alpha, weights = sparse(ops, head, order, rays, ts, den, rgb, zeros, act, bg)
            assert bool((alpha == 0).all()) and bool((weights == 0).all()), (S, M, R)
            assert bool((out == (1.0 if bg == "white" else 0.0)).all()), (S, M, R, bg)
    out, alpha, weights = sparse(ops, head, order, rays, rows, den, rgb, zeros, act, bg, want_weights=False)
    assert alpha is None and weights is None and bool((out == (1.0 if bg == "white" else 0.0)).all())


# ------------------------------------------------------------------------------------------------------------ 5. mixed tables
def check_sparse(ops, head, order, rays, rows, den, rgb, live, act, bg, what):
    f = X.sparse_ref(rays, rows, den, rgb, live, head, order, act, bg)
    b = X.sparse_bounds(f)
    dev = [t.cuda() for t in (rays, rows, den, rgb, live)]
    got = sparse(ops, head, order, *dev, act, bg)
    worst = {}
    for g, n in zip(got, ("out", "alpha", "weights")):
        assert g.shape == f["comp"][n].shape
        worst[n] = V.worst_ratio(g, f["comp"][n], b[n])
    print(f"[voxel sparse {head}{order if order >= 0 else ''} {what} {act}/{bg}] live {float(f['flags'].float().mean()):.2f}, "
          "worst |err| / bound: " + ", ".join(f"{n} {r:.3f}" for n, r in worst.items()))
    assert all(r <= 1.0 for r in worst.values()), (what, worst)
    flags = f["flags"].cuda()
    assert bool((got[1][~flags] == 0).all()) and bool((got[2][~flags] == 0).all()), what       # dead: exactly 0
    dense = rayts_render(ops, head, order, *dev[:4], act, bg)
    assert torch.equal(got[1][flags], dense[1][flags]), what                                   # a sample's alpha depends on no other
    return f["flags"]


@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_the_edge_set_against_the_fp64_restatement(ops, head, order):
    den, rgb = X.grids(head, order, X.EDGE_S)
    for what, (rays, rows, live, want) in (("edge set", X.edge_set()), ("drain set", X.edge_set(X.DRAIN_LINES, X.DRAIN_M))):
        for act in ACTS:
            for bg in ("black", "white"):
                flags = check_sparse(ops, head, order, rays, rows, den, rgb, live, act, bg, what)
                assert torch.equal(flags, want)


@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_mixed_tables_against_the_fp64_restatement(ops, head, order):
    """rays that start outside, inside (every 4th: the zero direction among them), miss the grid (every 5th), rows with a duplicate step"""
    i = HEADS.index((head, order))
    seen = 0
    for j, (S, M, R) in enumerate(((4, 17, 5), (6, 33, 257), (6, 65, 4), (4, 3, 3), (6, 16, 5), (4, 15, 257), (6, 31, 257))):
        den, rgb = V.grid_values(S)[0], X.grids(head, order, S)[1]
        live = X.table_of(den, MID)
        flags = check_sparse(ops, head, order, X.mixed_rays(R), X.mixed_rows(R, M), den, rgb, live, ACTS[(i + j) % 2],
                             ("black", "white")[(i + j // 2) % 2], f"S={S} M={M} R={R}")
        seen += int(flags.sum()) * int((~flags).sum()) > 0
    assert seen >= 4   # live and dead samples side by side


# ------------------------------------------------------------------------------------------------------------ 6. exact oracle
@pytest.mark.parametrize("head,order", HEADS, ids=HEAD_IDS)
def test_a_grid_whose_dead_voxels_render_to_nothing_is_rendered_bit_for_bit(ops, head, order):
    """every voxel that is not kept holds a density so low that the DENSE renderer's own alpha is exactly 0 where the table says dead:
    then the two renderers agree in every bit of out, alpha and weights.  All samples at least one voxel inside the grid (outside the
    lookup extrapolates with negative weights)."""
    for S, M, R, bg in ((6, 33, 65, "white"), (16, 65, 257, "black"), (6, 17, 4, "black")):
        den, rgb = V.grid_values(S)[0], X.grids(head, order, S)[1]   # (one density grid for every head: the same table)
        keep = X.keep_of(den, MID)
        den = torch.where(keep[..., None], den, torch.full_like(den, -1e30))
        g = torch.Generator().manual_seed(8800 + S + M)
        o = 0.6 * torch.rand(R, 3, generator=g) - 0.3
        d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * (0.2 + 0.8 * torch.rand(R, 1, generator=g))
        rays = torch.cat([o, d], dim=-1).float().contiguous()
        rows = torch.sort(0.5 * torch.rand(R, M, generator=g), dim=1).values.contiguous()
        assert float(F.pts_rayts(rays, rows).abs().max()) <= GR - GR * 2 / S
        live, _ = ops.voxel_live_table(den.cuda(), MID)
        assert torch.equal(live.cpu(), X.table_from_keep(keep))
        flags = X.flags_of(F.pts_rayts(rays, rows).reshape(-1, 3), live.cpu()).reshape(M, R).cuda()
        dev = [t.cuda() for t in (rays, rows, den, rgb)]
        want = rayts_render(ops, head, order, *dev, "upshifted", bg)
        assert int((~flags).sum()) > 0 and int(flags.sum()) > 0 and bool((want[1][~flags] == 0).all()), (S, int((~flags).sum()))
        got = sparse(ops, head, order, *dev, live, "upshifted", bg)
        for a, b, n in zip(got, want, ("out", "alpha", "weights")):
            assert torch.equal(a, b), (S, M, R, n, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------------ 7. lanes
@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 4), ("sh", 4)), ids=("rgb", "plv4", "sh4"))
def test_every_lane_count_gives_the_bits_of_16(ops, head, order):
    e_rays, e_rows, e_live, _ = X.edge_set()
    d_rays, d_rows, d_live, _ = X.edge_set(X.DRAIN_LINES, X.DRAIN_M)
    den6, rgb6 = V.grid_values(6)[0], X.grids(head, order, 6)[1]
    sets = [(e_rays, e_rows, den6, rgb6, e_live), (d_rays, d_rows, den6, rgb6, d_live), (X.mixed_rays(257), X.mixed_rows(257, 33), den6, rgb6, X.table_of(den6, MID)),
            (X.mixed_rays(5), X.mixed_rows(5, 17)[2].contiguous(), den6, rgb6, X.table_of(den6, MID))]
    for k, tensors in enumerate(sets):
        dev = [t.cuda() for t in tensors]
        want = sparse(ops, head, order, *dev, "thin", "white", lanes=16)
        for lanes in ops.VOXEL_FINE_LANES:
            got = sparse(ops, head, order, *dev, "thin", "white", lanes=lanes)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (k, lanes)


# ------------------------------------------------------------------------------------------------------------ 8. NaN containment
@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 1), ("sh", 1)), ids=("rgb", "plv1", "sh1"))
def test_a_nan_colour_reaches_exactly_the_rays_with_a_live_sample_that_reads_it(ops, head, order):
    S, M, R = 6, 17, 65
    den, rgb = V.grid_values(S)[0], X.grids(head, order, S)[1]
    rays, rows = V.generic_rays((R,), 8900), X.mixed_rows(R, M)
    rows[::4] = rows[::4] * 2.0 + 2.0   # (generic rays all start outside: undo mixed_rows' rows for rays that start inside)
    rows = torch.sort(rows, dim=1).values.contiguous()
    live = X.table_of(den, MID)
    pts = F.pts_rayts(rays, rows).reshape(-1, 3)
    ids, _ = V.cells(pts, S, GR)
    reads = V.rows_of(ids, S).reshape(M, R, 8)
    flags = X.flags_of(pts, live).reshape(M, R)
    per_live = torch.zeros(S ** 3, R, dtype=torch.bool)
    per_any = torch.zeros(S ** 3, R, dtype=torch.bool)
    for r in range(R):
        per_any[reads[:, r].reshape(-1), r] = True
        per_live[reads[:, r][flags[:, r]].reshape(-1), r] = True
    # a voxel that live samples of some rays read, and dead samples of OTHER rays as well
    score = per_live.sum(1) * (per_any & ~per_live).sum(1)
    row = int(score.argmax())
    want = per_live[row]
    assert 0 < int(want.sum()) < R and int((per_any[row] & ~want).sum()) > 0
    dev = [t.cuda() for t in (rays, rows, den)]
    clean = sparse(ops, head, order, *dev, rgb.cuda(), live.cuda(), "upshifted", "white")[0].cpu()
    assert bool(torch.isfinite(clean).all())
    c2 = rgb.clone()
    c2.reshape(S ** 3, -1)[row, c2.shape[-1] - 1] = float("nan")
    out = sparse(ops, head, order, *dev, c2.cuda(), live.cuda(), "upshifted", "white")[0].cpu()
    assert torch.equal(torch.isnan(out).any(-1), want), (int(torch.isnan(out).any(-1).sum()), int(want.sum()))
    assert torch.equal(out[~want], clean[~want])
    # the same voxel behind a table in which every cell whose samples can read it is dead: the NaN reaches nothing
    x, y, z = row // (S * S), (row // S) % S, row % S
    dead = live.clone()
    dead[max(x - 2, 0):x + 1, max(y - 2, 0):y + 1, max(z - 2, 0):z + 1] = 0
    f2 = X.flags_of(pts, dead).reshape(M, R)
    assert not bool((f2[..., None] & (reads == row)).any())
    clean2 = sparse(ops, head, order, *dev, rgb.cuda(), dead.cuda(), "upshifted", "white")
    out2 = sparse(ops, head, order, *dev, c2.cuda(), dead.cuda(), "upshifted", "white")
    assert all(torch.equal(a, b) for a, b in zip(out2, clean2)) and bool(torch.isfinite(out2[0]).all())
    # a NaN position stays NaN, whatever the table
    bad = rays.clone()
    bad[3, 1] = float("nan")
    out3 = sparse(ops, head, order, bad.cuda(), dev[1], dev[2], rgb.cuda(), torch.zeros_like(live).cuda(), "upshifted", "white")[0].cpu()
    assert bool(torch.isnan(out3[3]).all()) and bool((out3[torch.arange(R) != 3] == 1).all())


# ------------------------------------------------------------------------------------------------------------ 9. argument checks
def test_validation_codes_and_messages(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    p, st = ops._ptr, ops._stream()
    S, R, M = 4, 8, 5
    rays = V.generic_rays((R,), 8950).cuda()
    ts_ray = torch.linspace(2, 6, M).cuda().expand(R, M).contiguous()
    den = V.grid_values(S)[0].cuda()
    grid = torch.zeros(S ** 3 * 75 + 1, device="cuda")
    live = torch.ones(S, S, S, dtype=torch.uint8, device="cuda")
    out, alpha, weights = (torch.full(s, 5.0, device="cuda") for s in ((R, 3), (M, R), (M, R)))

    def call(head=0, order=-1, lanes=16, shared=0, rays_=p(rays), R_=R, row=p(ts_ray), M_=M, den_=p(den), rgb_=p(grid), S_=S, gr=GR,
             live_=p(live), act=4, bg=0, out_=p(out)):
        return lib.na_voxel_sparse_render(head, order, lanes, shared, rays_, R_, row, M_, den_, rgb_, S_, gr, live_, act, bg, p(alpha),
                                          p(weights), out_, st)

    assert call(live_=None) == NA_ENULL and b"na_voxel_sparse_render: live is null" in lib.na_last_error()
    for lanes in (0, 5, 128):
        assert call(lanes=lanes) == NA_EINVAL and b"lanes" in lib.na_last_error()
    for head in (-1, 3, 4):   # (3 is the proposal's tag: it has no colours to skip)
        assert call(head=head) == NA_EINVAL and b"head" in lib.na_last_error()
    assert call(M_=0) == NA_EINVAL and call(R_=-1) == NA_EINVAL and call(S_=5) == NA_EINVAL and call(gr=0.0) == NA_EINVAL
    assert call(head=1, order=5) == NA_EINVAL and call(head=2, order=-1) == NA_EINVAL
    assert call(act=12) == NA_EUNSUPPORTED and call(bg=2) == NA_EUNSUPPORTED
    assert call(rays_=None) == NA_ENULL and call(row=None) == NA_ENULL and call(den_=None) == NA_ENULL and call(rgb_=None) == NA_ENULL
    assert call(out_=None) == NA_ENULL
    assert call(head=1, order=2, rgb_=p(grid[1:])) == NA_EINVAL and b"16-byte" in lib.na_last_error()
    assert lib.na_voxel_live_table(None, S, 0.0, p(live), None, st) == NA_ENULL and lib.na_voxel_live_table(p(den), S, 0.0, None, None, st) == NA_ENULL
    assert lib.na_voxel_live_table(p(den), 5, 0.0, p(live), None, st) == NA_EINVAL
    flags = torch.full((M, R), 5, dtype=torch.uint8, device="cuda")
    assert lib.na_voxel_live_samples(None, p(rays), p(ts_ray), M, M, R, S, GR, None, p(flags), st) == NA_ENULL
    assert lib.na_voxel_live_samples(None, None, None, 0, M, R, S, GR, p(live), p(flags), st) == NA_ENULL
    assert lib.na_voxel_live_samples(None, p(rays), p(ts_ray), M - 1, M, R, S, GR, p(live), p(flags), st) == NA_EINVAL
    assert lib.na_voxel_mask_rows(None, p(flags), 4, 4, 0.0, p(out), st) == NA_ENULL and lib.na_voxel_mask_rows(p(out), p(flags), 4, 0, 0.0, p(out), st) == NA_EINVAL
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((alpha == 5.0).all()) and bool((weights == 5.0).all()) and bool((flags == 5).all())
    assert call(R_=0) == 0 and call() == 0
    with pytest.raises(ValueError, match="liveness table"):
        ops.voxel_sparse_render("rgb", rays, ts_ray, den, grid[:S ** 3 * 3].reshape(S, S, S, 3), live.float(), GR)
    with pytest.raises(ValueError, match="liveness table"):
        ops.voxel_sparse_render("rgb", rays, ts_ray, den, grid[:S ** 3 * 3].reshape(S, S, S, 3), live.cpu(), GR)
    with pytest.raises(ValueError, match="head"):
        ops.voxel_sparse_render("density", rays, ts_ray, den, grid[:S ** 3 * 3].reshape(S, S, S, 3), live, GR)
