"""The small operators of the D-NeRF and VolSDF paths on the GPU (csrc/basic_ops.hip, csrc/backward.hip, csrc/march.hip: the spline warp
and its gradient, the FFJORD divergence, the Laplace density, act_deriv / mul_bcast / mul_reduce / eikonal, normalize3, the
PosLinearView combine, the point light) against tests/deform_sdf_ref.py and its derived bounds, at the pitches, row counts and
values where their paths change; the autograd nodes over them against fp64 torch autograd of the plain expressions.

Every comparison covers every element (deform_sdf_ref.worst_ratio) and prints `[ratio] <operator> <worst |err| / bound>`.
NOT COVERED: the second sweep of the grid-stride loops -- it needs more than 32768 workgroups' worth of rows, about a gigabyte of
`est` for the staged warp."""
import itertools

import pytest
import torch

import deform_sdf_ref as D

pytestmark = pytest.mark.gpu

NA_EINVAL = -1   # include/nerf_atlas_amd.h
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def libm():
    """torch's own exp / sin / cos on this GPU against fp64 over D.libm_probe(): the kernels get twice that, never less than 2 u"""
    x = D.libm_probe().cuda()
    m = D.libm_errors(torch.exp(x), torch.sin(x), torch.cos(x))
    D.set_libm(m)
    print(f"[libm] torch.exp {m['exp']:.3e} relative, torch.sin {m['sin']:.3e}, torch.cos {m['cos']:.3e} absolute -> "
          f"E_exp {D.LIBM['exp']:.3e} E_sin {D.LIBM['sin']:.3e} E_cos {D.LIBM['cos']:.3e}")
    yield m
    D.set_libm(dict(exp=0.0, sin=0.0, cos=0.0))


WORST = {}


def inside(what, got, ref, bound, key=None):
    r = D.worst_ratio(got, ref, bound)
    key = key or what.split()[0]
    WORST[key] = max(WORST.get(key, 0.0), r) if r == r else NAN
    assert r <= 1.0, (what, r)
    return r


def report(*keys):
    for k in keys:
        if k in WORST:
            print(f"[ratio] {k} {WORST[k]:.3f}")


def cu(*ts):
    return [None if t is None else t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------------------ warp, forward
def run_warp(ops, est, pts, t, n, n_rl):
    out = ops.bezier_warp(*cu(est, pts, t), n, n_rl)
    N = pts.shape[0]
    assert out[0].shape == (N, 3) and out[1].shape == (N, 3) and out[2].shape == (N, 1) and (n_rl == 0 or out[3].shape == (N, n_rl))
    return [o.cpu() for o in out]


def check_warp(ops, est, pts, t, n, n_rl, ref, what):
    out = run_warp(ops, est, pts, t, n, n_rl)
    inside(f"warp.warped {what}", out[0], ref["warped"], ref["warped_b"])
    inside(f"warp.dp {what}", out[1], ref["dp"], ref["dp_b"])
    inside(f"warp.rig {what}", out[2], ref["rig"], ref["rig_b"])
    if n_rl:
        inside(f"warp.latent {what}", out[3], ref["enc"], ref["enc_b"])
    return out


@pytest.mark.parametrize("n", range(2, 9))
def test_warp_forward_every_pitch_and_row_count_inside_the_bounds(ops, n):
    """n_rl x pitch (the minimum, 31 | 32 | 33: direct / staged, 62 | 63 | 64 | 65: 256- / 64-thread workgroups, 255: the widest) x N
    (one row, around the 64- and 256-thread workgroups, several workgroups).  One reference per (n_rl, N): the pitch only adds columns."""
    for n_rl in (0, 1, 2, 16):
        for N in D.WARP_ROWS:
            est, pts, t = D.warp_inputs(n, n_rl, N)
            ref = D.warp_ref(est, pts, t, n, n_rl)
            for pitch in D.warp_pitches(n, n_rl):
                check_warp(ops, D.pad_cols(est, pitch), pts, t, n, n_rl, ref, f"n={n} n_rl={n_rl} N={N} pitch={pitch}")
    report("warp.warped", "warp.dp", "warp.rig", "warp.latent")


def test_warp_refuses_pitch_256_and_nine_control_points(ops):
    from nerf_atlas_amd._lib import NaError
    pts, t = torch.zeros(4, 3).cuda(), torch.zeros(4).cuda()
    for n_rl in (0, 2):
        with pytest.raises(NaError) as e:
            ops.bezier_warp(torch.zeros(4, 256).cuda(), pts, t, 4, n_rl)
        assert e.value.code == NA_EINVAL
        with pytest.raises(NaError) as e:
            ops.bezier_warp(torch.zeros(4, 200).cuda(), pts, t, 9, n_rl)
        assert e.value.code == NA_EINVAL
        ops.bezier_warp(torch.zeros(4, 255).cuda(), pts, t, 8, n_rl)
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", range(2, 9))
def test_warp_endpoints_are_the_end_control_points_bit_for_bit(ops, n):
    """t == 0 and t == 1 (the cubic form at n = 4, de Casteljau elsewhere): dp and the unscaled latent (latent scale saturated at 1)
    ARE the first / last control point; t outside [0, 1] extrapolates inside the bound"""
    n_rl, N = 2, 257
    for pitch in (D.est_min_width(n, n_rl), 64):
        for kind, k in (("zero", 0), ("one", n - 1)):
            est, pts, t = D.warp_inputs(n, n_rl, N, kind)
            est[:, 3 * n + 1] = 200.0
            est = D.pad_cols(est, pitch)
            out = check_warp(ops, est, pts, t, n, n_rl, D.warp_ref(est, pts, t, n, n_rl), f"t={kind} n={n} pitch={pitch}")
            assert torch.equal(out[1], est[:, 1 + 3 * k:4 + 3 * k]), (n, kind, pitch)
            assert torch.equal(out[3], est[:, 3 * n + 2 + k * n_rl:3 * n + 2 + (k + 1) * n_rl]), (n, kind, pitch)
        est, pts, t = D.warp_inputs(n, n_rl, N, "outside")
        est = D.pad_cols(est, pitch)
        check_warp(ops, est, pts, t, n, n_rl, D.warp_ref(est, pts, t, n, n_rl), f"t outside n={n} pitch={pitch}")


def test_warp_saturated_rigidity_is_exactly_zero_or_one(ops):
    for n, n_rl, pitch in ((3, 0, 10), (4, 0, 33), (6, 3, 38), (8, 0, 64)):
        est, pts, t = D.warp_inputs(n, n_rl, 300)
        est[:, 0] = torch.where(torch.arange(300) % 2 == 0, torch.tensor(-200.0), torch.tensor(200.0))
        est = D.pad_cols(est, pitch)
        out = check_warp(ops, est, pts, t, n, n_rl, D.warp_ref(est, pts, t, n, n_rl), f"saturated n={n} pitch={pitch}")
        assert torch.equal(out[2][:, 0], (torch.arange(300) % 2).float())
        assert torch.equal(out[0][0::2], pts[0::2])                      # rigidity 0: the points pass bit for bit
        assert torch.equal(out[0][1::2], pts[1::2] + out[1][1::2])       # rigidity 1: one add


@pytest.mark.parametrize("pitch", (40, 64))
def test_warp_rows_do_not_leak_through_the_shared_tile(ops, pitch):
    """a row of NaN in est: that row's outputs are NaN, every other row keeps its bits (rows share the staged LDS tile)"""
    n, n_rl, N = 6, 3, 600
    est, pts, t = D.warp_inputs(n, n_rl, N)
    est = D.pad_cols(est, pitch)
    clean = run_warp(ops, est, pts, t, n, n_rl)
    for row in (0, 63, 64, 255, 256, 300, N - 1):
        bad = est.clone()
        bad[row] = NAN
        out = run_warp(ops, bad, pts, t, n, n_rl)
        keep = torch.arange(N) != row
        for o, c in zip(out, clean):
            assert bool(torch.isnan(o[row]).all()), (pitch, row)
            assert torch.equal(o[keep], c[keep]), (pitch, row)


# ------------------------------------------------------------------------------------------------------------ warp, backward
def grads(N, n_rl, seed, mask=(1, 1, 1, 1)):
    g = [D.uniform((N, 3), seed), D.uniform((N, 3), seed + 1), D.uniform((N, 1), seed + 2), D.uniform((N, max(n_rl, 1)), seed + 3) if n_rl else None]
    return [x if m else None for x, m in zip(g, mask)]


def check_warp_backward(ops, est, t, n, n_rl, g, what):
    ge = ops.bezier_warp_backward(est.cuda(), t.cuda(), n, *cu(*g[:3]), n_rl=n_rl, g_enc=None if g[3] is None else g[3].cuda()).cpu()
    ref, b = D.warp_backward_ref(est, t, n, n_rl, *g)
    assert ge.shape == est.shape
    inside(f"warp_bwd {what}", ge, ref, b)
    used = D.est_min_width(n, n_rl) if (n_rl and g[3] is not None) else 1 + 3 * n
    assert int(ge[:, used:].count_nonzero()) == 0, what                  # trailing (and gradient-less latent) columns: exact zeros
    return ge


@pytest.mark.parametrize("n", range(2, 9))
def test_warp_backward_every_control_count_and_pitch(ops, n):
    for n_rl in (0, 2):
        for N in (1, 255, 257):
            est, _, t = D.warp_inputs(n, n_rl, N)
            for pitch in D.warp_pitches(n, n_rl, extra=(256, 300)):
                check_warp_backward(ops, D.pad_cols(est, pitch), t, n, n_rl, grads(N, n_rl, 6150 + n + N), f"n={n} n_rl={n_rl} N={N} pitch={pitch}")
    report("warp_bwd")


@pytest.mark.parametrize("n", range(2, 9))
def test_warp_backward_endpoints_and_saturation(ops, n):
    """t == 0 / 1: the Bernstein recurrence puts the whole gradient on the first / last control point, exact zeros elsewhere;
    saturated rigidity: ge[:, 0] == 0"""
    n_rl, N = 2, 130
    for kind, k in (("zero", 0), ("one", n - 1)):
        est, _, t = D.warp_inputs(n, n_rl, N, kind)
        est = D.pad_cols(est, D.est_min_width(n, n_rl) + 5)
        ge = check_warp_backward(ops, est, t, n, n_rl, grads(N, n_rl, 6170 + n), f"t={kind} n={n}")
        others = [c for j in range(n) if j != k for c in range(1 + 3 * j, 4 + 3 * j)]
        others += [3 * n + 2 + j * n_rl + c for j in range(n) if j != k for c in range(n_rl)]
        assert int(ge[:, others].count_nonzero()) == 0, (n, kind)
        assert int(ge[:, 1 + 3 * k:4 + 3 * k].count_nonzero()) == 3 * N
    est, _, t = D.warp_inputs(n, n_rl, N)
    est[:, 0] = torch.where(torch.arange(N) % 2 == 0, torch.tensor(-200.0), torch.tensor(200.0))
    ge = check_warp_backward(ops, est, t, n, n_rl, grads(N, n_rl, 6180 + n), f"saturated n={n}")
    assert int(ge[:, 0].count_nonzero()) == 0
    est, _, t = D.warp_inputs(n, n_rl, N, "outside")
    check_warp_backward(ops, est, t, n, n_rl, grads(N, n_rl, 6190 + n), f"t outside n={n}")


def test_warp_backward_every_combination_of_absent_upstream_gradients(ops):
    for n, n_rl, pitch in ((3, 0, 12), (4, 2, 24), (6, 3, 38), (8, 1, 64)):
        est, _, t = D.warp_inputs(n, n_rl, 77)
        est = D.pad_cols(est, pitch)
        for mask in itertools.product((0, 1), repeat=4 if n_rl else 3):
            mask = tuple(mask) + ((0,) if not n_rl else ())
            check_warp_backward(ops, est, t, n, n_rl, grads(77, n_rl, 6160 + n, mask), f"absent n={n} mask={mask}")


# ------------------------------------------------------------------------------------------------------------ divergence
@pytest.mark.parametrize("n", range(2, 9))
def test_ffjord_div_inside_the_bound(ops, n):
    """pitch at the minimum and 38 (make dnerf); one row, around a workgroup, several workgroups; t inside, at the ends and outside"""
    for pitch in sorted({D.est_min_width(n), max(38, D.est_min_width(n))}):
        for N in (1, 255, 257, 2049):
            for kind in ("interior",) if N == 2049 else ("interior", "zero", "one", "outside"):
                est, tan, t, e = D.ffjord_inputs(n, N, pitch, kind)
                got = ops.ffjord_div(*cu(est, tan, t, e), n)
                assert got.shape == (N,)
                inside(f"ffjord n={n} pitch={pitch} N={N} t={kind}", got, *D.ffjord_ref(est, tan, t, e, n))
    # saturated rigidity: drig == 0; with the control-point tangents zero as well (ddp rig == 0) the divergence is exactly 0
    est, tan, t, e = D.ffjord_inputs(n, 257, 38 if n < 8 else 40)
    est[:, 0] = torch.where(torch.arange(257) % 2 == 0, torch.tensor(-200.0), torch.tensor(200.0))
    inside(f"ffjord saturated n={n}", ops.ffjord_div(*cu(est, tan, t, e), n), *D.ffjord_ref(est, tan, t, e, n))
    tan[:, 1:1 + 3 * n] = 0.0
    got = ops.ffjord_div(*cu(est, tan, t, e), n).cpu()
    assert int(got.count_nonzero()) == 0
    report("ffjord")


# ------------------------------------------------------------------------------------------------------------ Laplace density
def offset_view(x):
    """the same values as a contiguous view one float into its storage: not 16-byte aligned, the kernels' scalar path"""
    buf = torch.empty(x.numel() + 1, device="cuda")
    buf[1:] = x.cuda().reshape(-1)
    v = buf[1:].reshape(x.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("beta", D.LAPLACE_BETAS)
def test_laplace_density_forward_and_backward(ops, beta):
    bt = torch.tensor(beta)                       # fp32
    b32 = float(bt)
    for N in D.LAPLACE_ROWS:
        sdf = D.laplace_inputs(N, b32)
        ref, bound = D.laplace_ref(sdf, b32)
        g = D.uniform((N,), 6450 + N, 1.0)
        gs_ref, gs_b, _, _ = D.laplace_backward_ref(sdf, b32, g)
        fin = D.laplace_inputs(N, b32, special=False)
        _, _, gb_ref, gb_b = D.laplace_backward_ref(fin, b32, g)
        for name, view in (("aligned", lambda x: x.cuda()), ("offset", offset_view)):
            got = ops.laplace_density(view(sdf), bt.cuda())
            inside(f"laplace.fwd {name} beta={beta} N={N}", got, ref, bound)
            half = (torch.tensor(1.0) / bt) * 0.5
            assert got[:min(N, 2)].cpu().tolist() == [float(half)] * min(N, 2)             # sdf == +-0: 0.5 / beta from both branches
            g_sdf, g_beta = ops.laplace_density_backward(view(sdf), bt.cuda(), view(g), want_beta=True)
            inside(f"laplace.g_sdf {name} beta={beta} N={N}", g_sdf, gs_ref, gs_b)
            g_sdf2, none = ops.laplace_density_backward(view(sdf), bt.cuda(), view(g), want_beta=False)
            assert none is None and torch.equal(g_sdf2.cpu(), g_sdf.cpu())
            _, g_beta = ops.laplace_density_backward(view(fin), bt.cuda(), view(g), want_beta=True)
            assert g_beta.shape == (1,)
            inside(f"laplace.g_beta {name} beta={beta} N={N}", g_beta, gb_ref.reshape(1), gb_b)
    report("laplace.fwd", "laplace.g_sdf", "laplace.g_beta")


@pytest.mark.parametrize("beta", D.LAPLACE_BETAS)
def test_laplace_density_relative_error_outside_the_surface(ops, beta):
    """sdf > 0 from 0 to 110 beta: the density falls through the whole normal range into the denormals and to 0"""
    bt = torch.tensor(beta)
    sdf = (torch.arange(4099, dtype=torch.float32) * (110.0 / 4098)) * float(bt)
    ref, bound = D.laplace_ref(sdf, float(bt))
    inside(f"laplace.tail beta={beta}", ops.laplace_density(sdf.cuda(), bt.cuda()), ref, bound)
    report("laplace.tail")


# ------------------------------------------------------------------------------------------------------------ tangent operators
@pytest.mark.parametrize("n", D.ACT_ROWS)
def test_act_deriv_mul_bcast_mul_reduce(ops, n):
    x = D.act_inputs(n)
    for act in ("sin", "leaky_relu", "none"):
        for order in (1, 2):
            inside(f"act_deriv.{act}{order} n={n}", ops.act_deriv(x.cuda(), act, order), *D.act_deriv_ref(x, act, order))
    for J in (1, 3):
        a, b, g = D.uniform((n,), 6510 + n), D.uniform((J, n), 6520 + n + J), D.uniform((J, n), 6530 + n + J)
        inside(f"mul_bcast J={J} n={n}", ops.mul_bcast(a.cuda(), b.cuda()), *D.mul_bcast_ref(a, b))
        inside(f"mul_reduce J={J} n={n}", ops.mul_reduce(g.cuda(), b.cuda()), *D.mul_reduce_ref(g, b))
    nrm = D.uniform((3, n), 6540 + n, 1.5)
    loss, lb = D.eikonal_ref(nrm)
    inside(f"eikonal n={n}", ops.eikonal_loss(nrm.cuda()).reshape(1), loss.reshape(1), lb)
    inside(f"eikonal_bwd n={n}", ops.eikonal_loss_backward(nrm.cuda(), torch.tensor(0.7).cuda()), *D.eikonal_backward_ref(nrm, 0.7))
    report("act_deriv.sin1", "act_deriv.sin2", "act_deriv.leaky_relu1", "mul_bcast", "mul_reduce", "eikonal", "eikonal_bwd")


# ------------------------------------------------------------------------------------------------------------ normalize3, PosLinearView, light
@pytest.mark.parametrize("N", D.NORMALIZE_ROWS)
def test_normalize3(ops, N):
    v = D.normalize3_rows(N)
    got = ops.normalize3(v.cuda()).cpu()
    inside(f"normalize3 N={N}", got, *D.normalize3_ref(v))
    if N >= 8:
        assert int(got[[1, 5]].count_nonzero()) == 0                          # zero rows stay zero
        assert got[2].tolist() == [float(torch.tensor(1e-25) / torch.tensor(1e-12))] * 3
    report("normalize3")


def test_normalize3_nan_row_is_all_nan(ops):
    """F.normalize: the norm of a row with a NaN is NaN and every component is divided by it"""
    v = D.normalize3_nan_rows()
    got = ops.normalize3(v.cuda()).cpu()
    ref, b = D.normalize3_ref(v)
    assert bool(torch.isnan(ref[7]).all()) and bool(torch.isnan(got[7]).all()) and bool(torch.isnan(got[200]).all()), got[7].tolist()
    inside("normalize3 nan", got, ref, b)


@pytest.mark.parametrize("N", (1, 257, 3000))
def test_pos_linear_combine_and_backward(ops, N):
    for W, C, extra in ((3, 3, 0), (3, 3, 4), (7, 3, 0), (7, 5, 2)):
        lin = D.uniform((N, 1), 6560 + N + W, 4.0)
        if N > 2:
            lin[0], lin[1] = 200.0, -200.0
        big = D.uniform((N, W + extra), 6570 + N + W + extra, 1.5).cuda()
        pos = big[:, :W]                                                        # pos_ld = W + extra > C: a column slice, no copy
        g = D.uniform((N, C), 6580 + N + C)
        got = ops.pos_linear_combine(lin.cuda(), pos, C)
        assert got.shape == (N, C)
        inside(f"pos_linear W={W} C={C} ld={W + extra} N={N}", got, *D.pos_linear_ref(lin, pos.cpu(), C))
        gl_ref, gl_b, gp_ref, gp_b = D.pos_linear_backward_ref(lin, pos.cpu(), g, C)
        for want_lin, want_pos in ((True, True), (True, False), (False, True)):
            g_lin, g_pos = ops.pos_linear_combine_backward(lin.cuda(), pos, g.cuda(), C, want_lin, want_pos)
            if want_lin:
                inside(f"pos_linear.g_lin W={W} C={C} N={N}", g_lin, gl_ref, gl_b)
            else:
                assert g_lin is None
            if want_pos:
                assert g_pos.shape == (N, W) and int(g_pos[:, C:].count_nonzero()) == 0      # columns at or beyond C_out: exact zeros
                inside(f"pos_linear.g_pos W={W} C={C} N={N}", g_pos, gp_ref, gp_b)
            else:
                assert g_pos is None
    report("pos_linear", "pos_linear.g_lin", "pos_linear.g_pos")


@pytest.mark.parametrize("N", D.LIGHT_ROWS)
def test_point_light(ops, N):
    for per_c, per_i, decay in itertools.product((False, True), (False, True), (True, False)):
        x, c, _ = D.light_inputs(N, per_c)
        _, _, i = D.light_inputs(N, per_i)
        d, dist, spec = ops.point_light(*cu(x, c, i), distance_decay=decay)
        (dr, db), (lr, lb), (sr, sb) = D.point_light_ref(x, c, i, decay)
        what = f"N={N} centre stride {3 * per_c} intensity stride {3 * per_i} decay={decay}"
        inside(f"light.dir {what}", d, dr, db)
        inside(f"light.dist {what}", dist, lr, lb)
        inside(f"light.spectrum {what}", spec, sr, sb)
        if N > 3:                                                               # row 3 sits ON the light
            assert d[3].tolist() == [0.0, 0.0, 0.0] and float(dist[3]) == 0.0
            assert bool(torch.isinf(spec[3]).all()) if decay else torch.equal(spec[3].cpu(), i[3] if per_i else i)
    report("light.dir", "light.dist", "light.spectrum")


def test_point_light_nan_row_is_all_nan(ops):
    """F.normalize(eps=1e-6): a NaN coordinate makes the distance NaN and with it the whole direction and the decayed spectrum"""
    x, c, i = D.light_nan_inputs()
    d, dist, spec = ops.point_light(*cu(x, c, i))
    (dr, db), (lr, lb), (sr, sb) = D.point_light_ref(x, c, i, True)
    assert bool(torch.isnan(dr[9]).all()) and bool(torch.isnan(d[9]).all()), d[9].tolist()
    inside("light.dir nan", d, dr, db)
    inside("light.dist nan", dist, lr, lb)
    inside("light.spectrum nan", spec, sr, sb)


# ------------------------------------------------------------------------------------------------------------ autograd nodes
def close_grads(what, got, ref, scale=256.0):
    """the nodes' kernels are held to their bounds above; here the WIRING is under test (shapes, strides, which inputs get a gradient --
    a mistake there is an error of order 1): every entry within `scale` u of the tensor's largest magnitude (sums of a few hundred
    addends of mixed sign: g_beta, the eikonal mean).  A leaf the plain expression does not depend on may get no gradient or zeros."""
    if ref is None:
        assert got is None or int(got.count_nonzero()) == 0, what
        return
    assert got is not None, what
    got = got.detach().cpu().double()
    assert got.shape == ref.shape and torch.equal(torch.isnan(got), torch.isnan(ref)), (what, got.shape, ref.shape)   # (the mean of nothing is NaN)
    got, ref = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(ref, nan=0.0)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.numel() == 0:
        return
    tol = scale * D.U * max(float(ref.abs().max()), 1e-30)
    assert float((got.detach().cpu().double() - ref).abs().max()) <= tol, (what, float((got.detach().cpu().double() - ref).abs().max()), tol)


def leaf(x, req, dtype=torch.float32, dev="cuda"):
    return x.to(dev, dtype).clone().requires_grad_(req)


def node_case(what, fn_gpu, fn_ref, inputs, reqs, losses):
    """inputs: fp32 CPU tensors (or (tensor, view function) pairs: the node sees view(leaf)); every loss in `losses` maps the tuple
    of outputs to a scalar; gradients w.r.t. the leaves against fp64 autograd of fn_ref"""
    for lname, loss in losses:
        a = [leaf(x[0] if isinstance(x, tuple) else x, r) for x, r in zip(inputs, reqs)]
        d = [leaf(x[0] if isinstance(x, tuple) else x, r, torch.float64, "cpu") for x, r in zip(inputs, reqs)]
        view = lambda x, l: x[1](l) if isinstance(x, tuple) else l
        out = fn_gpu(*[view(x, l) for x, l in zip(inputs, a)])
        ref = fn_ref(*[view(x, l) for x, l in zip(inputs, d)])
        out, ref = (out if isinstance(out, tuple) else (out,)), (ref if isinstance(ref, tuple) else (ref,))
        for o, r in zip(out, ref):
            close_grads(f"{what} {lname} forward", o, r.detach())
        if not any(reqs):
            assert not any(o.requires_grad for o in out)
            continue
        loss(out).backward()
        if loss(ref).requires_grad:          # (a loss over rigidity alone does not depend on the points)
            loss(ref).backward()
        for k, (l, r) in enumerate(zip(a, d)):
            close_grads(f"{what} {lname} reqs={reqs} grad {k}", l.grad, r.grad)


def req_combos(k):
    return [c for c in itertools.product((False, True), repeat=k)]


def test_bezier_warp_fn(ops):
    from nerf_atlas_amd.autograd import BezierWarpFn
    for n, n_rl, N in ((5, 0, 257), (4, 2, 65), (6, 3, 0)):
        est, pts, t = D.warp_inputs(n, n_rl, max(N, 1))
        est, pts, t = est[:N], pts[:N], t[:N]
        estT = est.t().contiguous()                                              # the node sees its transpose: non-contiguous
        ref_fn = lambda e, p: tuple(o for o in D.warp_fp64(e, p, t.double().reshape(-1, 1), n, n_rl)[:4] if o is not None)
        gpu_fn = lambda e, p: BezierWarpFn.apply(e, p, t.cuda(), n, n_rl)
        losses = [("all", lambda o: sum((x * x).sum() for x in o)), ("warped only, sum", lambda o: o[0].sum()),
                  ("rigidity only", lambda o: (o[2] * o[2]).sum()), ("dp slice", lambda o: o[1][:, 1].sum())]
        if n_rl:
            losses.append(("latent only", lambda o: o[3].sum()))
        for reqs in req_combos(2):
            node_case(f"BezierWarpFn n={n} n_rl={n_rl} N={N}", gpu_fn, ref_fn, [(estT, lambda l: l.t()), pts], reqs, losses)


def test_laplace_density_fn(ops):
    from nerf_atlas_amd.autograd import LaplaceDensityFn
    ref_fn = lambda s, b: D.O.laplace_cdf(-s, b) / b
    losses = [("sum", lambda o: o[0].sum()), ("weighted", lambda o: (o[0] * o[0]).sum())]
    for N in (257, 0):
        net = D.uniform((max(N, 1), 4), 6610, 0.3)[:N]                            # the SDF column of an [N, 1 + C] network output
        for beta_shape in ((), (1,)):
            beta = torch.full(beta_shape, 0.05)
            for reqs in req_combos(2):
                node_case(f"LaplaceDensityFn N={N} beta{beta_shape}", LaplaceDensityFn.apply, ref_fn, [(net, lambda l: l[:, :1]), beta], reqs, losses)


def test_pos_linear_combine_fn(ops):
    from nerf_atlas_amd.autograd import PosLinearCombineFn
    for N, W, C in ((257, 7, 3), (64, 3, 3), (0, 7, 3)):
        lin, pos = D.uniform((max(N, 1), 2), 6620, 3.0)[:N], D.uniform((max(N, 1), W), 6621, 1.0)[:N]
        ref_fn = lambda l, p: (torch.sigmoid(l) / 2 + 0.5) * p[..., :C]
        gpu_fn = lambda l, p: PosLinearCombineFn.apply(l, p, C)
        losses = [("sum", lambda o: o[0].sum()), ("squares", lambda o: (o[0] * o[0]).sum()), ("one column", lambda o: o[0][:, 1].sum())]
        for reqs in req_combos(2):
            node_case(f"PosLinearCombineFn N={N} W={W} C={C}", gpu_fn, ref_fn, [(lin, lambda l: l[:, 1:]), pos], reqs, losses)


def test_act_deriv_fn(ops):
    """sin: the node's gradient is the double backward of torch.sin; LeakyReLU and none: zeros"""
    from nerf_atlas_amd.autograd import ActDerivFn
    for N in (257, 0):
        x = D.act_inputs(max(N, 1) * 4).reshape(-1, 4)[:N] * 0.05
        xT = x.t().contiguous()
        losses = [("sum", lambda o: o[0].sum()), ("weighted", lambda o: (o[0] * o[0]).sum())]
        for reqs in req_combos(1):
            node_case(f"ActDerivFn sin N={N}", lambda v: ActDerivFn.apply(v, "sin"), lambda v: torch.cos(v), [(xT, lambda l: l.t())], reqs, losses)
            slope = lambda v: torch.where(v > 0, torch.ones_like(v), torch.full_like(v, D.LEAKY_SLOPE)) + 0 * v
            node_case(f"ActDerivFn leaky N={N}", lambda v: ActDerivFn.apply(v, "leaky_relu"), slope, [(xT, lambda l: l.t())], reqs, losses)
    # the double backward itself: d/dx of (d sin / dx) by torch, against the node
    x = (D.act_inputs(300) * 0.05).double().requires_grad_()
    (first,) = torch.autograd.grad(torch.sin(x).sum(), x, create_graph=True)
    (second,) = torch.autograd.grad((first * first).sum(), x)
    xg = x.detach().float().cuda().requires_grad_()
    m = ActDerivFn.apply(xg, "sin")
    (m * m).sum().backward()
    close_grads("ActDerivFn double backward of sin", xg.grad, second)


def test_mul_bcast_fn(ops):
    from nerf_atlas_amd.autograd import MulBcastFn
    for N, K, J in ((65, 4, 3), (257, 1, 1), (0, 4, 3)):
        a, b = D.uniform((K, max(N, 1)), 6640 + K)[:, :N], D.uniform((J, max(N, 1), K), 6641 + K)[:, :N]
        losses = [("sum", lambda o: o[0].sum()), ("squares", lambda o: (o[0] * o[0]).sum()), ("one tangent row", lambda o: o[0][J - 1].sum())]
        for reqs in req_combos(2):
            node_case(f"MulBcastFn N={N} K={K} J={J}", MulBcastFn.apply, lambda x, y: x.unsqueeze(0) * y, [(a.contiguous(), lambda l: l.t()), b.contiguous()],
                      reqs, losses)


def test_eikonal_fn(ops):
    from nerf_atlas_amd.autograd import EikonalFn
    ref_fn = lambda v: ((v.norm(dim=0) - 1) ** 2).mean()
    losses = [("plain", lambda o: o[0]), ("scaled", lambda o: o[0] * 0.3)]
    for N in (1, 257, 5000, 0):                                                    # (N = 0: a NaN loss and an empty gradient, like torch)
        nrm = D.uniform((max(N, 1), 3), 6650 + N, 1.5)[:N]                        # stored [N, 3]: the node sees the [3, N] transpose
        for reqs in req_combos(1):
            node_case(f"EikonalFn N={N}", EikonalFn.apply, ref_fn, [(nrm, lambda l: l.t())], reqs, losses)
