"""The marching state machines on the GPU (csrc/march.hip) fed CHOSEN states: each update kernel and its `_indexed` form against one
step of the reference (src/march.py:39-45, :96-103, :159-179) as restated in tests/deform_sdf_ref.py, with torch.equal -- every
operation is a comparison or one fp32 add / halving of given values --, and na_compact_rays at the segment boundaries.
The chosen rows (an SDF value equal to eps, a distance equal to far or one ulp beyond it, ties, +-0, NaN, a bracket exactly eps wide)
are decided by hand in tests/test_deform_sdf_ref.py::test_exact_thresholds_of_the_marching_restatement."""
import pytest
import torch

import deform_sdf_ref as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def column(v, stride, seed):
    """v [R] -> a contiguous [R, stride] CUDA tensor whose column 0 is v (the other columns hold other values)"""
    if stride == 1:
        return v.cuda().clone()
    out = D.uniform((v.numel(), stride), seed, 3.0)
    out[:, 0] = v
    return out.cuda()


def compact(ops, live):
    """-> (idx int32 [R + 256] on the device, n)"""
    R = live.numel()
    idx = torch.full((R + 256,), -7, device="cuda", dtype=torch.int32)
    cnt = torch.zeros(1, device="cuda", dtype=torch.int32)
    n = ops.compact_rays(live.cuda(), idx, cnt)
    return idx, n


def same(got, want, what):
    got = got.cpu()
    if got.dtype == torch.uint8:
        got = got.bool()
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    ok = torch.equal(torch.nan_to_num(got, nan=12345.0), torch.nan_to_num(want, nan=12345.0)) if got.is_floating_point() else torch.equal(got, want)
    assert ok, (what, (got != want).nonzero().flatten()[:8].tolist())
    if got.is_floating_point():
        assert torch.equal(torch.isnan(got), torch.isnan(want)), what


@pytest.mark.parametrize("stride", (1, 4))
@pytest.mark.parametrize("R", D.MARCH_ROWS)
def test_sphere_march_update_on_chosen_states(ops, R, stride):
    sdf, dist, hits, rem = D.sphere_states(R)
    want = D.sphere_step(sdf, D.EPS, D.FAR, dist, hits, rem)
    dev = lambda: (dist.cuda().clone(), hits.to(torch.uint8).cuda(), rem.to(torch.uint8).cuda())
    d, h, r = dev()
    ops.sphere_march_update(column(sdf, stride, 7300 + R), D.EPS, D.FAR, d, h, r)
    for g, w, name in zip((d, h, r), want, ("dist", "hits", "rem")):
        same(g, w, f"sphere {name} R={R} stride={stride}")
    # the indexed form over the compacted live rays: row i of the SDF buffer belongs to ray idx[i]
    idx, n = compact(ops, rem.to(torch.uint8))
    assert n == int(rem.sum()) and torch.equal(idx[:n].cpu().long(), rem.nonzero().flatten())
    d2, h2, r2 = dev()
    ops.sphere_march_update_indexed(column(sdf[rem], stride, 7310 + R), idx, n, D.EPS, D.FAR, d2, h2, r2)
    for g, w, name in zip((d2, h2, r2), (d, h, r), ("dist", "hits", "rem")):
        assert torch.equal(torch.nan_to_num(g, nan=1.5) if g.is_floating_point() else g, torch.nan_to_num(w, nan=1.5) if w.is_floating_point() else w), (name, R, stride)
    # ... and over a random live mask: rays outside it keep their state, rays inside it with rem == 0 as well
    live = D.live_mask(R)
    idx, n = compact(ops, live)
    lv = live.bool()
    assert n == int(lv.sum())
    d3, h3, r3 = dev()
    ops.sphere_march_update_indexed(column(sdf[lv], stride, 7320 + R), idx, n, D.EPS, D.FAR, d3, h3, r3)
    w3 = D.sphere_step(sdf, D.EPS, D.FAR, dist, hits, rem & lv)
    same(d3, w3[0], "sphere indexed dist")
    same(h3, w3[1], "sphere indexed hits")
    same(r3, torch.where(lv, w3[2], rem), "sphere indexed rem")


@pytest.mark.parametrize("stride", (1, 4))
@pytest.mark.parametrize("R", D.MARCH_ROWS)
def test_sign_change_update_on_chosen_states(ops, R, stride):
    """ties, +-0, a first_neg that is already written, NaN on either side (torch.minimum keeps it)"""
    sd, cm, idxs, last, first = D.sign_states(R)
    for step in (0, 8):
        want = D.sign_change_step(sd, step, cm, idxs, last, first)
        c, i, l, f = cm.cuda().clone(), idxs.cuda().clone(), last.cuda().clone(), first.cuda().clone()
        ops.sign_change_update(column(sd, stride, 7400 + R), step, c, i, l, f)
        for g, w, name in zip((c, i, l, f), want, ("curr_min", "idxs", "last_pos", "first_neg")):
            same(g, w, f"sign change {name} R={R} stride={stride} step={step}")
    # two steps in a row: first_neg is written once
    c, i, l, f = cm.cuda().clone(), idxs.cuda().clone(), last.cuda().clone(), first.cuda().clone()
    neg = -sd.abs() - 0.5
    ops.sign_change_update(column(neg, stride, 7410 + R), 3, c, i, l, f)
    ops.sign_change_update(column(neg - 1.0, stride, 7420 + R), 4, c, i, l, f)
    w = D.sign_change_step(neg - 1.0, 4, *D.sign_change_step(neg, 3, cm, idxs, last, first))
    for g, ww, name in zip((c, i, l, f), w, ("curr_min", "idxs", "last_pos", "first_neg")):
        same(g, ww, f"sign change twice {name} R={R}")
    fin = ~torch.isnan(neg)
    assert bool(((f.cpu() == 4) | (first != -1))[fin].all()) and not bool(((f.cpu() == 5) & (first != 5)).any())


@pytest.mark.parametrize("stride", (1, 4))
@pytest.mark.parametrize("R", D.MARCH_ROWS)
def test_bisection_update_on_chosen_states(ops, R, stride):
    """the init call (sdf_mid null), high == low, high - low == eps, sdf_mid == +-0, done rows; dense against indexed"""
    lo, hi, sl, sh, sm = D.bisect_states(R)
    eps = D.BISECT_EPS
    z0, todo0 = D.bisection_init(lo, hi, sl, sh, eps)
    state = lambda: [v.cuda().clone() for v in (lo, hi, sl, sh)] + [torch.full((R,), -3.0, device="cuda"), torch.full((R,), 9, device="cuda", dtype=torch.uint8)]
    a = state()
    ops.bisection_update(None, eps, *a)
    for g, w, name in zip(a, (lo, hi, sl, sh, z0, todo0), ("low", "high", "sdf_low", "sdf_high", "z", "todo")):
        same(g, w, f"bisection init {name} R={R}")
    want = D.bisection_step(sm, eps, lo, hi, sl, sh, z0, todo0)
    ops.bisection_update(column(sm, stride, 7500 + R), eps, *a)
    for g, w, name in zip(a, want, ("low", "high", "sdf_low", "sdf_high", "z", "todo")):
        same(g, w, f"bisection step {name} R={R} stride={stride}")
    done = ~todo0
    assert torch.equal(a[0].cpu()[done], lo[done]) and torch.equal(a[1].cpu()[done], hi[done])       # done rows keep their bracket
    # indexed, over the rays that are still to do (what nerf_atlas_amd.march runs) == dense, bit for bit
    b = state()
    ops.bisection_update(None, eps, *b)
    idx, n = compact(ops, b[5])
    assert n == int(todo0.sum())
    if n:
        ops.bisection_update_indexed(column(sm[todo0], stride, 7510 + R), idx, n, eps, *b)
    for g, w, name in zip(b, a, ("low", "high", "sdf_low", "sdf_high", "z", "todo")):
        assert torch.equal(g, w), (name, R, stride)
    # ... and over a random live mask: the rows outside it keep everything
    live = D.live_mask(R)
    lv = live.bool()
    c = state()
    ops.bisection_update(None, eps, *c)
    idx, n = compact(ops, live)
    if n:
        ops.bisection_update_indexed(column(sm[lv], stride, 7520 + R), idx, n, eps, *c)
    init = (lo, hi, sl, sh, z0, todo0)
    for g, w, w0, name in zip(c, want, init, ("low", "high", "sdf_low", "sdf_high", "z", "todo")):
        same(g, torch.where(lv, w, w0), f"bisection indexed {name} R={R}")


@pytest.mark.parametrize("R", (1, 255, 256, 257, 4099, 65535, 65536, 65537))
def test_compact_rays_boundaries(ops, R):
    """256 blocks own ceil(R / 256) rays each: segments of one ray, a ragged last segment, R just around 256 x 256"""
    cases = {"all": torch.ones(R, dtype=torch.uint8), "last": torch.zeros(R, dtype=torch.uint8), "none": torch.zeros(R, dtype=torch.uint8),
             "random": D.live_mask(R), "bytes": (D.live_mask(R, 6950) * 255)}
    cases["last"][R - 1] = 1
    for name, live in cases.items():
        idx, n = compact(ops, live)
        want = live.nonzero().flatten()
        assert n == want.numel(), (name, R, n)
        assert torch.equal(idx[:n].cpu().long(), want), (name, R)
        assert bool((idx[n:R] == -7).all()), (name, R)                     # nothing written behind the live rays
