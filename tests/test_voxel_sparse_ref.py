"""NeRFVoxel.sparsify on the CPU: the restatement of tests/voxel_sparse_ref.py against its own definition -- the threshold, the table's
window, conservativeness of the lower-id test over the corners a sample reads, dead samples, the table of ones -- and the coverage of
the edge set the GPU tests run (so that no GPU test passes without meeting the edges of the compaction)."""
import math

import pytest
import torch

import voxel_fine_ref as F
import voxel_ref as V
import voxel_sparse_ref as X

GR = V.GRID_RADIUS


def test_d_thresh_is_the_density_whose_softplus_is_the_threshold():
    assert X.d_thresh(0) == float("-inf")
    for t in (1e-6, 1e-2, 0.3, 1.0, 5.0, 50.0):
        d = X.d_thresh(t)
        assert d == float(torch.tensor(d, dtype=torch.float32)), t                    # an fp32 number
        assert abs(math.log1p(math.exp(d - 1)) - t) <= 2.0 ** -22 * max(t, abs(d)) + 1e-12, (t, d)
    assert X.d_thresh(1e3) == 1001.0
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError):
            X.d_thresh(bad)


def test_table_is_the_window_or_and_keeps_nan():
    S = 6
    den, _ = V.grid_values(S)
    den = den.clone()
    den[1, 2, 3, 0] = float("nan")
    den[4, 4, 4, 0] = float("inf")
    den[0, 0, 0, 0] = -float("inf")
    assert bool(X.table_of(den, 0).all())                              # thresh 0 keeps everything, -inf included
    keep = X.keep_of(den, 10.0)                                        # above every finite density
    assert bool(keep[1, 2, 3]) and bool(keep[4, 4, 4]) and int(keep.sum()) == 2
    live = X.table_from_keep(keep)
    want = torch.zeros(S, S, S, dtype=torch.uint8)
    for x in range(S):
        for y in range(S):
            for z in range(S):
                want[x, y, z] = int(any(keep[min(x + i, S - 1), min(y + j, S - 1), min(z + k, S - 1)]
                                        for i in range(3) for j in range(3) for k in range(3)))
    assert torch.equal(live, want)
    assert int(live.sum()) == 2 * 3 * 3 + 3 * 3 * 3                    # the windows at and below (1,2,3), clipped at x = 0, and (4,4,4)
    mid = X.table_of(den, 0.5)
    assert 0 < int(mid.sum()) and bool((mid >= X.keep_of(den, 0.5).to(torch.uint8)).all())


@pytest.mark.parametrize("S", (2, 4, 6, 16))
def test_every_sample_that_reads_a_kept_voxel_is_live(S):
    """conservativeness, on the lattice (one ulp decides the membership of either floor), inside, outside and on the faces of the
    grid; and its premise: the upper id of an axis is the lower id + 0, 1 or 2"""
    g = torch.Generator().manual_seed(90 + S)
    faces = V.uniform_points(512, 8400 + S, 1.5).clone()
    faces[torch.arange(512), torch.arange(512) % 3] = torch.tensor([GR, -GR])[torch.arange(512) % 2]
    pts = torch.cat([V.lattice_points(S), V.uniform_points(2048, 8500 + S, 1.3), V.uniform_points(2048, 8600 + S, 2.5), faces,
                     V.zero_points()]).contiguous()
    spread = X.axis_spread(pts, S)
    assert int(spread.min()) >= 0 and int(spread.max()) <= 2, (int(spread.min()), int(spread.max()))
    for frac in (0.02, 0.2, 0.7):
        keep = torch.rand(S, S, S, generator=g) < frac
        live = X.table_from_keep(keep)
        reads, flags = X.reads_kept(pts, keep), X.flags_of(pts, live)
        assert bool((flags | ~reads).all()), (S, frac, int((reads & ~flags).sum()))
        assert not bool(flags.all()) or frac > 0.5 or S == 2
    bad = torch.tensor([[float("nan"), 0.0, 0.0], [0.0, float("inf"), 0.0], [0.1, 0.2, -float("inf")]])
    assert bool(X.flags_of(bad, torch.zeros(S, S, S, dtype=torch.uint8)).all())   # a non-finite position stays live


@pytest.mark.parametrize("head,order", (("rgb", -1), ("plv", 1), ("sh", 1)), ids=("rgb", "plv1", "sh1"))
def test_a_table_of_ones_is_fine_ref_and_a_dead_sample_has_no_alpha_and_no_weight(head, order):
    S, R, M = 6, 9, 17
    den, rgb = X.grids(head, order, S)
    rays, rows = X.mixed_rays(R), X.mixed_rows(R, M)
    f = F.fine_ref(rays, rows, den, rgb, head, order, "thin", "white")
    s = X.sparse_ref(rays, rows, den, rgb, torch.ones(S, S, S, dtype=torch.uint8), head, order, "thin", "white")
    assert bool(s["flags"].all())
    for k in ("out", "alpha", "weights"):
        assert torch.equal(s["comp"][k], f["comp"][k]), k
    b, fb = X.sparse_bounds(s), F.fine_bounds(f)
    assert all(torch.equal(b[k], fb[k]) for k in ("out", "alpha", "weights"))
    live = X.table_of(den, X.MID)
    s = X.sparse_ref(rays, rows, den, rgb, live, head, order, "thin", "white")
    dead = ~s["flags"]
    assert 0 < int(dead.sum()) < dead.numel()
    assert bool((s["comp"]["alpha"][dead] == 0).all()) and bool((s["comp"]["weights"][dead] == 0).all())
    b = X.sparse_bounds(s)
    assert all(bool(torch.isfinite(b[k]).all()) for k in ("out", "alpha", "weights"))
    # nothing alive: the background alone
    s = X.sparse_ref(rays, rows, den, rgb, torch.zeros(S, S, S, dtype=torch.uint8), head, order, "thin", "white")
    assert not bool(s["flags"].any()) and bool((s["comp"]["out"] == 1).all())


def test_the_edge_set_meets_every_edge_of_the_compaction():
    rays, rows, live, want = X.edge_set()
    M, R = want.shape
    L = X.LANES
    assert rows.shape == (R, M) and M == X.EDGE_M and M > 4 * L and bool((rows[:, 1:] > rows[:, :-1]).all())
    flags = X.flags_of(F.pts_rayts(rays, rows).reshape(-1, 3), live).reshape(M, R)
    assert torch.equal(flags, want)
    count, cross = X.run_stats(flags)
    for n in (0, 1, L - 1, L, L + 1, M):
        assert int((count == n).sum()) >= 1, n
    first_only = (count == 1) & flags[0]
    last_only = (count == 1) & flags[M - 1]
    assert bool(first_only.any()) and bool(last_only.any())
    assert int(cross.sum()) >= 2
    # whole chunks: the first, the last full one, one in the middle
    names = [n for n, _, _ in X.EDGE_LINES]
    assert bool(flags[:L, names.index("first L")].all()) and int(count[names.index("first L")]) == L
    assert bool(flags[M - L:, names.index("last L")].all()) and int(count[names.index("last L")]) == L
    assert bool(flags[L:2 * L, names.index("second chunk only")].all()) and int(count[names.index("second chunk only")]) == L


def test_the_drain_set_leaves_more_than_a_chunk_in_the_queue():
    """M = 31: L - 1 steps can wait when the last chunk of L - 1 steps arrives, so the queue is drained in two rounds"""
    rays, rows, live, want = X.edge_set(X.DRAIN_LINES, X.DRAIN_M)
    M, R = want.shape
    L = X.LANES
    assert M == 31 and rows.shape == (R, M)
    flags = X.flags_of(F.pts_rayts(rays, rows).reshape(-1, 3), live).reshape(M, R)
    assert torch.equal(flags, want)
    waiting = flags[:L].sum(0) % L + flags[L:].sum(0)      # steps in the queue at the drain
    for n in (0, L, L + 1, 2 * L - 2):
        assert int((waiting == n).sum()) >= 1, (n, waiting.tolist())


def test_mixed_tables_of_the_gpu_tests_are_mixed():
    for S in (4, 6):
        den, _ = V.grid_values(S)
        live = X.table_of(den, X.MID)
        assert 0 < int(live.sum()) < S ** 3, (S, int(live.sum()))
        rays, rows = X.mixed_rays(257), X.mixed_rows(257, 33)
        flags = X.flags_of(F.pts_rayts(rays, rows).reshape(-1, 3), live)
        assert 0.05 < float(flags.float().mean()) < 0.95, (S, float(flags.float().mean()))
