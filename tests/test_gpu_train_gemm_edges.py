"""The split-bf16 training Linears at their edges (csrc/train_gemm.hip, train_gemm_tiled.h, train_fwd.hip, train_bwd.hip,
train_shared.h), through every entry point ops.py has for them, over the shape table of tests/train_gemm_ref.py -- each shape
asserted to run the path the table names, by the library's own predicates (ops.linear_f32_path / linear_dgrad_path /
linear_wgrad_path read what the entry points dispatch on).

A. exact addressing: integer operands make every product and partial sum exact in fp32; every result EQUALS the integer reference
   (torch.equal: a NaN, a dropped / doubled / misplaced / stale element all fail; +0 == -0 is the one thing not distinguished).
B. isolation: a NaN / +Inf / -Inf stays in its row (y, g_x) or column / row (dW, db); inputs surrounded by NaN and inputs at 4- and
   8-byte aligned bases give the plain run's bits; outputs inside sentinel-filled buffers leave the sentinel intact around them
   and none of it inside; a row scaled by 2^s gives exactly the scaled row.
C. every entry of the inexact cases within the derived per-entry bound of train_gemm_ref (no max-norm over the output).

The premises (exactness of the integer cases, the bound against an emulation) are CPU tests: tests/test_train_gemm_ref.py."""
import ctypes as C

import pytest
import torch

import train_gemm_ref as R

pytestmark = pytest.mark.gpu

SENT = -7777.25   # what no case computes: outputs and their surroundings are pre-filled with it


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops
    return ops


def check_paths(ops, c):
    """the shape runs where the table says it does, by the library's own dispatch predicates"""
    N, in0, in1, out = c.N, c.in0, c.in1, c.out
    if c.col0 == 0:
        assert ops.linear_f32_path(N, out) == c.fwd
        assert ops.linear_dgrad_path(N, out, in0, in1) == c.dgrad
        assert ops.linear_wgrad_path(N, out, in0, in1) == c.wgrad
        for act in R.ACTS:
            assert ops.linear_f32_path(N, out, in0, in1, act, packed=True) == (c.fwd_pk or R.K_STAGED), act
        assert ops.linear_dgrad_path(N, out, in0, in1, packed=True) == (c.dgrad_pk or R.K_STAGED)
        assert ops.train_gemm_packed_ok(N, out) == (c.fwd_pk is not None)
        assert ops.train_gemm_packed_ok(N, in0 + in1) == (c.dgrad_pk is not None)
    assert ops.linear_bwd_fused_ok(N, out, in0) == c.fused


def run_ops(ops, c, act, x0, x1, W, b, dY, kinds="ygw", exact32=False, autograd=False):
    """Every entry point that takes the shape -> {"<kind>:<entry>": tensor}, kind y [N, out] | g [N, in0 + in1] | dW [out, in0 + in1]
    | db [out].  W is [out, col0 + in0 + in1]; with col0 > 0 the source is a skip layer's second one (one-pass backward, columns
    col0.. of dW)."""
    N, in0, in1, out, col0 = c.N, c.in0, c.in1, c.out, c.col0
    r = {}
    cat = lambda a, b_: a if b_ is None else torch.cat([a, b_], 1)
    pf = pt = None
    if c.fwd_pk is not None:
        (pf,) = ops.train_pack_many([(W, False)])
    if c.dgrad_pk is not None or c.fused:
        (pt,) = ops.train_pack_many([(W, True)])
    ls_cols = col0 > 0 or c.wgrad == R.LS       # na_linear_wgrad_bf16x3_cols takes the batch
    if col0 == 0:
        if "y" in kinds:
            r["y:split"] = ops.linear_f32(x0, W, b, act, x1, split_bf16=True)
            if pf is not None:
                r["y:packed"] = ops.linear_f32(x0, W, b, act, x1, split_bf16=True, packed=pf)
            if exact32:
                r["y:fp32"] = ops.linear_f32(x0, W, b, act, x1)
        if "g" in kinds:
            r["g:split"] = cat(*ops.linear_dgrad(dY, W, x0, act, x1))
            if in1:   # one half requested at a time
                h0, z1 = ops.linear_dgrad(dY, W, x0, act, x1, want1=False)
                z0, h1 = ops.linear_dgrad(dY, W, x0, act, x1, want0=False)
                assert z0 is None and z1 is None
                r["g:split halves"] = cat(h0, h1)
            if c.dgrad_pk is not None:
                r["g:packed"] = cat(*ops.linear_dgrad(dY, W, x0, act, x1, packed_t=pt))
                if in1:   # one half requested at a time
                    h0, z1 = ops.linear_dgrad(dY, W, x0, act, x1, want1=False, packed_t=pt)
                    z0, h1 = ops.linear_dgrad(dY, W, x0, act, x1, want0=False, packed_t=pt)
                    assert z0 is None and z1 is None
                    r["g:packed halves"] = cat(h0, h1)
        if "w" in kinds:
            r["dW:split"], r["db:split"] = ops.linear_wgrad(x0, dY, act, x1, split_bf16=True)
            if exact32:
                r["dW:fp32"], r["db:fp32"] = ops.linear_wgrad(x0, dY, act, x1)
    if "w" in kinds and ls_cols and out <= 256 and in0 <= 256 and in1 <= 256:
        dW = torch.full((out, col0 + in0 + in1), SENT, device="cuda")
        ops.linear_wgrad_cols(x0, dY, act, dW, col0)
        if in1:
            ops.linear_wgrad_cols(x1, dY, act, dW, in0)
        assert bool((dW[:, :col0] == SENT).all()), "columns of the other source keep what they held"
        r["dW:cols"] = dW[:, col0:]
    if c.fused and ("g" in kinds or "w" in kinds):
        two = in1 > 0 and in0 % 64 == 0 and ops.linear_bwd_fused_ok(N, out, in1)   # the second source takes the one-pass kernel too
        if in1 == 0 or two:
            if col0 == 0:
                g0, dW, db = ops.linear_bwd_fused(dY, x0, act, pt, in1=in1)
            else:
                dW = torch.full((out, col0 + in0), SENT, device="cuda")
                g0, _, db = ops.linear_bwd_fused(dY, x0, act, pt, dW=dW, col0=col0)
                assert bool((dW[:, :col0] == SENT).all()), "columns of the other source keep what they held"
            g1 = ops.linear_bwd_fused(dY, x1, act, pt, dW=dW, col0=in0)[0] if two else None
            # the same pass without its reduction, every source's partial gradients summed by ONE launch
            q0, ws0, n0 = ops.linear_bwd_partials(dY, x0, act, pt, col0=col0)
            dW2 = torch.full((out, col0 + in0 + in1), SENT, device="cuda")
            db2 = torch.full((out,), SENT, device="cuda")
            ent = [(ws0, n0, out, in0, dW2, col0, db2)]
            q1 = None
            if two:
                q1, ws1, n1 = ops.linear_bwd_partials(dY, x1, act, pt, col0=in0, want_bias=False)
                ent.append((ws1, n1, out, in1, dW2, in0, None))
            ops.train_reduce_many(ent)
            assert bool((dW2[:, :col0] == SENT).all())
            if "g" in kinds:
                r["g:fused"], r["g:partials"] = cat(g0, g1), cat(q0, q1)
            if "w" in kinds:
                r["dW:fused"], r["dW:partials"], r["db:partials"] = dW[:, col0:], dW2[:, col0:], db2
                if db is not None:
                    r["db:fused"] = db
    if autograd and col0 == 0:
        from nerf_atlas_amd import autograd as ag
        leaves = [t.clone().requires_grad_() if t is not None else None for t in (x0, x1, W, b)]
        y = ag.LinearFn.apply(leaves[0], leaves[1], leaves[2], leaves[3], act, (pf, pt) if pf is not None else None)
        y.backward(dY)
        r["y:LinearFn"], r["g:LinearFn"] = y.detach(), cat(leaves[0].grad, leaves[1].grad if in1 else None)
        r["dW:LinearFn"], r["db:LinearFn"] = leaves[2].grad, leaves[3].grad
    return r


def to_dev(t):
    return None if t is None else t.float().cuda()


def sources(c, x):
    x = to_dev(x)
    return x[:, :c.in0].contiguous(), (x[:, c.in0:].contiguous() if c.in1 else None)


def assert_equal(r, refs, what):
    """every result equals its integer reference"""
    assert r, what
    for key, got in r.items():
        ref = refs[key.split(":")[0]]
        assert got.shape == ref.shape, (what, key, got.shape, ref.shape)
        if not torch.equal(got, ref):
            bad = (got != ref) | torch.isnan(got)
            i = tuple(int(v) for v in bad.nonzero()[0])
            pytest.fail(f"{what} {key}: {int(bad.sum())} of {bad.numel()} entries differ, first at {i}: got {float(got[i])}, "
                        f"reference {float(ref[i])}")


# ================================================================================================ A: exact addressing
@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_dense_integers_are_exact(ops, c):
    """Operands in [-8, 8] (LeakyReLU: inputs in [1, 8]): the three GEMMs and db against the integer matmul, no tolerance; the exact
    fp32 entry points and autograd.LinearFn through the same harness."""
    check_paths(ops, c)
    for act, positive in (("none", False), ("leaky_relu", True)):
        x, W, b, dY = R.dense_operands(c, positive)
        y, g, dW, db = R.dense_refs(c, x, W, b, dY)
        assert max(int(t.abs().max()) for t in (y, g, dW, db)) < 2 ** 24
        refs = {"y": to_dev(y), "g": to_dev(g), "dW": to_dev(dW), "db": to_dev(db)}
        x0, x1 = sources(c, x)
        r = run_ops(ops, c, act, x0, x1, to_dev(W), to_dev(b), to_dev(dY), exact32=True, autograd=True)
        assert_equal(r, refs, f"{R.case_id(c)} {act}")


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_one_hot_probes_are_exact(ops, c):
    """One nonzero per row against 16-bit integers (hi AND lo planes): every output entry is a single product, every (row, column)
    pair of the weight gradient receives at most one."""
    check_paths(ops, c)
    for act, positive in (("none", False), ("leaky_relu", True)):
        what = f"{R.case_id(c)} {act}"
        W_small = R.ints((c.out, c.col0 + c.in0 + c.in1), -8, 8, "W", c.out, c.in0)
        if c.col0 == 0:
            x, W, b, y = R.onehot_forward(c, positive)
            x0, x1 = sources(c, x)
            r = run_ops(ops, c, act, x0, x1, to_dev(W), to_dev(b), None, kinds="y", exact32=True)
            assert_equal(r, {"y": to_dev(y)}, what + " forward")
        dY, W, x, g = R.onehot_dgrad(c, positive)
        x0, x1 = sources(c, x)
        r = run_ops(ops, c, act, x0, x1, to_dev(W), None, to_dev(dY), kinds="g")
        if c.col0 == 0 or c.fused:
            assert_equal(r, {"g": to_dev(g)}, what + " input gradient")
        x, dY, dW, db = R.onehot_wgrad(c, positive)
        x0, x1 = sources(c, x)
        r = run_ops(ops, c, act, x0, x1, to_dev(W_small), None, to_dev(dY), kinds="w", exact32=True)
        assert_equal(r, {"dW": to_dev(dW), "db": to_dev(db)}, what + " weight gradient")


# ================================================================================================ e_act, measured
def test_sin_error_through_a_selection_matrix(ops):
    """e_act of the bound: the kernels' sin (forward, W = the identity: each output is ONE activation value times 1.0) and cos (input
    gradient, dY one-hot 1.0, W = 1: act'(x) times 1.0) against fp64 over the ranges the tests use.
    Measured on an MI355X (the maximum over 2 x 2^20 arguments per range and function):
        [-2, 2]    sin  3.930e-06   cos  2.095e-07
        [-30, 30]  sin  3.999e-06   cos  2.504e-07
    (the sine's figure is mostly the hi + lo split of the value, 2^-18 = 3.8e-6; the cosine is multiplied in after the sum)
    train_gemm_ref.E_SIN is twice the largest of them (the factor two for the finite sample); a fresh measurement must stay
    inside it."""
    assert ops.linear_f32_path(4096, 256) == R.LS
    eye = torch.eye(256, device="cuda")
    worst = {}
    for span in (2.0, 30.0):
        x = R.uniform((4096, 256), -span, span, "sin", int(span)).cuda()
        y = ops.linear_f32(x, eye, None, "sin", split_bf16=True)
        worst[span, "sin"] = float((y.double() - torch.sin(x.double())).abs().max())
        dY = torch.zeros(4096, 1, device="cuda")
        dY[:, 0] = 1.0
        g, _ = ops.linear_dgrad(dY, torch.ones(1, 256, device="cuda"), x, "sin")
        worst[span, "cos"] = float((g.double() - torch.cos(x.double())).abs().max())
        # the K-staged kernels share tact / tact_grad
        ys = ops.linear_f32(x[:1024], eye, None, "sin", split_bf16=True)
        assert ops.linear_f32_path(1024, 256) == R.K_STAGED
        worst[span, "sin"] = max(worst[span, "sin"], float((ys.double() - torch.sin(x[:1024].double())).abs().max()))
    print("measured e_act:", {f"{k[1]} [-{k[0]:g}, {k[0]:g}]": f"{v:.3e}" for k, v in worst.items()})
    assert R.E_SIN is not None and max(worst.values()) <= R.E_SIN, worst


# ================================================================================================ B + C: isolation and the per-entry bound
def rep_case(name):
    N, in0, in1, out = R.REPRESENTATIVES[name]
    return _named(name, N, in0, in1, out)


def _named(name, N, in0, in1, out):
    """a Case for a representative shape: its paths read from the library (asserted against the name below)"""
    from nerf_atlas_amd import ops
    pk = ops.train_gemm_packed_ok(N, out)
    pkt = ops.train_gemm_packed_ok(N, in0 + in1)
    return R.Case(name, N, in0, in1, out, 0, ops.linear_f32_path(N, out), ops.linear_dgrad_path(N, out, in0, in1),
                  ops.linear_wgrad_path(N, out, in0, in1), ops.linear_f32_path(N, out, in0, in1, "none", packed=True) if pk else None,
                  ops.linear_dgrad_path(N, out, in0, in1, packed=True) if pkt else None, ops.linear_bwd_fused_ok(N, out, in0))


REP_PATH = {"k_staged": ("fwd", R.K_STAGED), "ls": ("fwd_pk", R.LS), "narrow": ("fwd_pk", R.NARROW), "narrow_dgrad": ("dgrad_pk", R.NARROW),
            "narrow_x1": ("dgrad_pk", R.NARROW_X1), "resident": ("fwd_pk", R.RESIDENT), "resident_narrow": ("fwd_pk", R.RESIDENT),
            "bwd": ("fused", True), "bwd_wide": ("fused", True)}


def float_operands(c, act, span=2.0):
    K = c.in0 + c.in1
    x = R.uniform((c.N, K), -span, span, "x", c.N, K)
    W = R.uniform((c.out, K), -1.0, 1.0, "W", c.out, K) * (1.0 / K) ** 0.5
    b = R.uniform((c.out,), -1.0, 1.0, "b", c.out)
    dY = R.uniform((c.N, c.out), -1.0, 1.0, "dY", c.N, c.out)
    return x, W, b, dY


def assert_bounded(r, refs, what, atomic_ok=True):
    """non-finite exactly where the reference is, every other entry inside its bound; -> the worst ratio"""
    worst = 0.0
    for key, got in r.items():
        ref, bound = refs[key.split(":")[0]]
        got = got.cpu()
        assert got.shape == ref.shape, (what, key)
        bad_got, bad_ref = ~torch.isfinite(got), ~torch.isfinite(ref)
        if not torch.equal(bad_got, bad_ref):
            d = (bad_got != bad_ref).nonzero()
            i = tuple(int(v) for v in d[0])
            pytest.fail(f"{what} {key}: {len(d)} entries are non-finite on one side only, first at {i}: got {float(got[i])}, "
                        f"reference {float(ref[i])}")
        ratio = R.worst_ratio(got, ref, bound)
        assert ratio <= 1.0, f"{what} {key}: |error| / bound = {ratio:.3f}"
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("name", sorted(R.REPRESENTATIVES))
def test_every_entry_within_its_bound_and_non_finite_values_stay_in_place(ops, name, act):
    """Dense uniform inputs (negative ones under LeakyReLU, [-2, 2] and [-30, 30] under sin): every entry of every result within
    c * sum |a| |b| + e_act * sum |b|.  Then one NaN, one +Inf and one -Inf in x0, x1 and dY in turn (the NaN in the last row of
    the batch, the +Inf in the last column of a ragged row): the results are non-finite exactly where the fp64 reference is --
    rows of y and g_x, columns and rows of dW, entries of db -- and within the bound everywhere else."""
    c = rep_case(name)
    field, path = REP_PATH[name]
    assert getattr(c, field) == path, (name, c)
    for span in ((2.0, 30.0) if act == "sin" else (2.0,)):
        x, W, b, dY = float_operands(c, act, span)
        Wd, bd = W.cuda(), b.cuda()

        def run(xp, dYp, tag):
            x0, x1 = sources(c, xp)
            r = run_ops(ops, c, act, x0, x1, Wd, bd, dYp.cuda(), autograd=True)
            return assert_bounded(r, R.float_refs(xp, W, b, dYp, act), f"{name} {act} [-{span:g}, {span:g}] {tag}")
        worst = run(x, dY, "plain")
        print(f"{name} {act} span {span:g}: worst |error| / bound = {worst:.3f}")
        if span != 2.0:
            continue
        xp, _ = R.poison(x[:, :c.in0])
        run(torch.cat([xp, x[:, c.in0:]], 1), dY, "x0 poisoned")
        if c.in1:
            xp, _ = R.poison(x[:, c.in0:])
            run(torch.cat([x[:, :c.in0], xp], 1), dY, "x1 poisoned")
        run(x, R.poison(dY)[0], "dY poisoned")


def embed(t, lead=64):
    """t as a contiguous view inside a larger storage filled with NaN, `lead` floats in front and 64 behind"""
    buf = torch.full((t.numel() + lead + 64,), float("nan"), device="cuda")
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def assert_same_bits(r, plain, refs, what, c):
    """bit for bit the plain run; the K-staged weight gradient adds its sample slices with fp32 atomics in arrival order (its
    fixed-point mode has its own suite): held to the bound instead"""
    for key, got in r.items():
        if key.split(":")[0] in ("dW", "db") and key.split(":")[1] in ("split", "LinearFn") and c.wgrad == R.K_STAGED:
            assert_bounded({key: got}, refs, what)
        else:
            assert torch.equal(got, plain[key]), f"{what} {key}: differs from the plain run"


@pytest.mark.parametrize("act", R.ACTS)
@pytest.mark.parametrize("name", sorted(R.REPRESENTATIVES))
def test_inputs_surrounded_by_nan_give_the_plain_bits(ops, name, act):
    """Every input a contiguous view inside NaN-filled storage, 64 floats on either side: nothing outside the operands is read."""
    c = rep_case(name)
    x, W, b, dY = float_operands(c, act)
    refs = R.float_refs(x, W, b, dY, act)
    x0, x1 = sources(c, x)
    plain = run_ops(ops, c, act, x0, x1, W.cuda(), b.cuda(), dY.cuda(), autograd=True)
    r = run_ops(ops, c, act, embed(x0), embed(x1) if c.in1 else None, embed(W.cuda()), embed(b.cuda()), embed(dY.cuda()), autograd=True)
    assert_same_bits(r, plain, refs, f"{name} {act} embedded", c)


# (N, in0, in1, out): row slices x[n0:] of 38-, 69-, 3- and 1-column tensors (and of dY with 65 / 67 / 255 columns), n0 odd
SLICED = [("k_staged", 2047, 38, 3, 65), ("k_staged", 65, 1, 69, 67), ("ls", 2048 + 63, 69, 1, 67), ("ls", 2049, 3, 38, 255),
          ("narrow_dgrad", 2049, 69, 0, 256), ("narrow_x1", 2049, 256, 38, 256), ("resident", 8192 + 31, 256, 69, 256),
          ("resident_narrow", 8193, 38, 0, 256), ("resident_narrow", 8193, 1, 0, 256), ("bwd", 8192 + 33, 69, 0, 255),
          ("bwd", 8193, 3, 0, 65), ("bwd", 8193, 1, 0, 67), ("bwd", 8192 + 33, 38, 0, 256)]


@pytest.mark.parametrize("shape", SLICED, ids=lambda s: "%s-N%d-in%d+%d-out%d" % s)
def test_row_slices_at_4_and_8_byte_aligned_bases_give_the_plain_bits(ops, shape):
    """x[n0:] of a tensor whose row is not a multiple of 16 bytes starts 4 or 8 bytes off a 16-byte boundary, and is contiguous: the
    entry points take it as it is.  Every path may: a tensor of such a width has its rows n >= 1 at exactly these alignments
    already (row n of 38 columns starts 152 n bytes in), the kernels address a row as base + 4 * width * n and fetch it with
    dword-granular buffer loads (16-byte pieces at 4-byte alignment, train_gemm.hip load_piece / the dword branches of lstn, nrw,
    lsfw and lsbw for widths with width & 3 != 0; scalar loads in train_gemm_tiled.h) -- a base moved by n0 rows is the address of
    row n0.  The results must be the bits of the same values in a fresh allocation."""
    name, N, in0, in1, out = shape
    c = _named(name, N, in0, in1, out)
    field, path = REP_PATH[name]
    assert getattr(c, field) == path, (name, c)
    for act, n0 in (("leaky_relu", 1), ("sin", 3)):
        x, W, b, dY = float_operands(c, act)
        refs = R.float_refs(x, W, b, dY, act)
        x0, x1 = sources(c, x)
        dYd = dY.cuda()
        plain = run_ops(ops, c, act, x0, x1, W.cuda(), b.cuda(), dYd, autograd=True)

        def sliced(t):
            if t is None or t.shape[1] % 4 == 0:
                return t
            big = torch.full((t.shape[0] + n0, t.shape[1]), float("nan"), device="cuda")
            big[n0:] = t
            v = big[n0:]
            assert v.is_contiguous() and v.data_ptr() % 16 in (4, 8, 12)
            return v
        r = run_ops(ops, c, act, sliced(x0), sliced(x1), W.cuda(), b.cuda(), sliced(dYd), autograd=True)
        assert_same_bits(r, plain, refs, f"{name} {act} sliced at {n0}", c)


class Guarded:
    """an output at a 16-byte aligned offset inside a sentinel-filled buffer"""

    def __init__(self, *shape, pad=64, fill=SENT):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * pad,), SENT, device="cuda")
        self.t = self.buf[pad:pad + n].view(*shape)
        assert self.t.data_ptr() % 16 == 0
        self.pad, self.n = pad, n
        if fill != SENT:
            self.t.fill_(fill)

    def check(self, what, written=None):
        assert bool((self.buf[:self.pad] == SENT).all()) and bool((self.buf[self.pad + self.n:] == SENT).all()), f"{what}: written outside the output"
        w = self.t if written is None else written
        assert not bool((w == SENT).any()), f"{what}: part of the output was not written"


@pytest.mark.parametrize("name", sorted(R.REPRESENTATIVES))
def test_outputs_inside_sentinel_buffers_leave_their_surroundings_intact(ops, name):
    """Through the C ABI: y, g_x0, g_x1, dW and db at 16-byte aligned offsets inside buffers pre-filled with a sentinel -- the
    sentinel is intact on both sides, none of it survives inside, and the columns of the other source of dW keep it."""
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    c = rep_case(name)
    N, in0, in1, out = c.N, c.in0, c.in1, c.out
    K = in0 + in1
    act = ops.ACT["leaky_relu"]
    x, W, b, dY = float_operands(c, "leaky_relu")
    x0, x1 = sources(c, x)
    W, b, dY = W.cuda(), b.cuda(), dY.cuda()
    Wt = W.t().contiguous()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    ok = _lib.check
    pf, pt = ops.train_pack_many([(W, False), (W, True)])
    # forward
    for what, call in (("na_linear_bf16x3", lambda y: lib.na_linear_bf16x3(p(x0), in0, p(x1), in1, N, p(W), p(b), out, act, p(y), st)),
                       ("na_linear_f32", lambda y: lib.na_linear_f32(p(x0), in0, p(x1), in1, N, p(W), p(b), out, act, p(y), st)),
                       ("na_linear_bf16x3_pk", None if c.fwd_pk is None else
                        lambda y: lib.na_linear_bf16x3_pk(p(x0), in0, p(x1), in1, N, p(pf), p(b), out, act, p(y), st))):
        if call is not None:
            y = Guarded(N, out)
            ok(call(y.t))
            y.check(f"{name} {what} y")
    # input gradient: both halves, then one at a time
    for what, call in (("na_linear_dgrad_bf16x3", lambda a, b_: lib.na_linear_dgrad_bf16x3(p(dY), out, N, p(Wt), p(x0), in0, p(x1), in1, act, p(a), p(b_), st)),
                       ("na_linear_dgrad_bf16x3_pk", None if c.dgrad_pk is None else
                        lambda a, b_: lib.na_linear_dgrad_bf16x3_pk(p(dY), out, N, p(pt), p(x0), in0, p(x1), in1, act, p(a), p(b_), st))):
        if call is None:
            continue
        for want0, want1 in ((True, True), (True, False), (False, True)) if in1 else ((True, False),):
            g0, g1 = Guarded(N, in0), (Guarded(N, in1) if in1 else None)
            ok(call(g0.t if want0 else None, g1.t if (want1 and in1) else None))
            for g, want, tag in ((g0, want0, "g_x0"), (g1, want1, "g_x1")):
                if g is not None:
                    g.check(f"{name} {what} {tag}", written=g.t if want else g.t[:0])
                    assert want or bool((g.t == SENT).all()), f"{name} {what}: the unrequested {tag} was written"
    # weight gradient: written, accumulated (exact fp32), and one source's columns at a time
    dW, db = Guarded(out, K), Guarded(out)
    ok(lib.na_linear_wgrad_bf16x3_ow(p(x0), in0, p(x1), in1, N, p(dY), out, act, p(dW.t), p(db.t), st))
    dW.check(f"{name} na_linear_wgrad_bf16x3_ow dW")
    db.check(f"{name} na_linear_wgrad_bf16x3_ow db")
    dW, db = Guarded(out, K, fill=0.0), Guarded(out, fill=0.0)
    ok(lib.na_linear_wgrad(p(x0), in0, p(x1), in1, N, p(dY), out, act, p(dW.t), p(db.t), st))
    dW.check(f"{name} na_linear_wgrad dW")
    db.check(f"{name} na_linear_wgrad db")
    if c.wgrad == R.LS:
        for src, w, col0 in ((x0, in0, 0), (x1, in1, in0)):
            if w:
                dW = Guarded(out, K)
                ok(lib.na_linear_wgrad_bf16x3_cols(p(src), w, N, p(dY), out, act, C.c_void_p(dW.t.data_ptr() + 4 * col0), K, None, st))
                dW.check(f"{name} na_linear_wgrad_bf16x3_cols at {col0}", written=dW.t[:, col0:col0 + w])
                assert bool((dW.t[:, :col0] == SENT).all()) and bool((dW.t[:, col0 + w:] == SENT).all()), "the other source's columns keep the sentinel"
    # one-pass backward of each source that takes it: fused, and partials + one reduction
    for src, w, col0 in ((x0, in0, 0), (x1, in1, in0)):
        if not (w and ops.linear_bwd_fused_ok(N, out, w) and (col0 % 64 == 0)):
            continue
        wp = C.c_void_p(pt.data_ptr() + int(lib.na_train_packed_row_offset(col0, out)))
        ws = torch.empty(int(lib.na_linear_bwd_workspace_bytes(N, w)), device="cuda", dtype=torch.uint8)
        g, dW, db = Guarded(N, w), Guarded(out, K), Guarded(out)
        ok(lib.na_linear_bwd_bf16x3_pk(p(dY), out, N, wp, p(src), w, act, p(g.t), C.c_void_p(dW.t.data_ptr() + 4 * col0), K, p(db.t), p(ws), st))
        g.check(f"{name} na_linear_bwd_bf16x3_pk g_x at {col0}")
        db.check(f"{name} na_linear_bwd_bf16x3_pk db")
        dW.check(f"{name} na_linear_bwd_bf16x3_pk dW at {col0}", written=dW.t[:, col0:col0 + w])
        assert bool((dW.t[:, :col0] == SENT).all()) and bool((dW.t[:, col0 + w:] == SENT).all()), "the other source's columns keep the sentinel"
        g, dW, db = Guarded(N, w), Guarded(out, K), Guarded(out)
        ok(lib.na_linear_bwd_partials_bf16x3_pk(p(dY), out, N, wp, p(src), w, act, p(g.t), None, 1, p(ws), st))
        ops.train_reduce_many([(ws, int(lib.na_linear_bwd_partial_count(N, w)), out, w, dW.t, col0, db.t)])
        g.check(f"{name} na_linear_bwd_partials_bf16x3_pk g_x at {col0}")
        db.check(f"{name} na_train_reduce_many db")
        dW.check(f"{name} na_train_reduce_many dW at {col0}", written=dW.t[:, col0:col0 + w])
        assert bool((dW.t[:, :col0] == SENT).all()) and bool((dW.t[:, col0 + w:] == SENT).all()), "the other source's columns keep the sentinel"


@pytest.mark.parametrize("name", sorted(R.REPRESENTATIVES))
def test_a_row_scaled_by_a_power_of_two_is_the_scaled_row(ops, name):
    """Activation none, no bias, row n of x (of dY) times 2^s(n), s cycling over -100, -1, 0, 1, 100: row n of y (of g_x) is the
    unscaled run's row scaled, bit for bit -- any cross-row leak shows at 2^200 times its size.  Operands of 12 / 9 significant
    bits keep every hi, lo and product a normal number at 2^-100 (the smallest nonzero product is 2^-22 * 2^-100)."""
    c = rep_case(name)
    K = c.in0 + c.in1
    x = R.ints((c.N, K), -2047, 2047, "xs", c.N, K).float() / 1024
    dY = R.ints((c.N, c.out), -2047, 2047, "dYs", c.N, c.out).float() / 1024
    W = (R.ints((c.out, K), -511, 511, "Ws", c.out, K).float() / 4096).cuda()
    s = torch.tensor([-100, -1, 0, 1, 100])[torch.arange(c.N) % 5]
    scale = torch.ldexp(torch.ones(c.N), s)[:, None]
    x0, x1 = sources(c, x)
    plain = run_ops(ops, c, "none", x0, x1, W, None, dY.cuda(), kinds="yg")
    s0, s1 = sources(c, x * scale)
    r = {**run_ops(ops, c, "none", s0, s1, W, None, dY.cuda(), kinds="y"),
         **run_ops(ops, c, "none", x0, x1, W, None, (dY * scale).cuda(), kinds="g")}
    assert {k.split(":")[0] for k in r} == {"y", "g"}
    sc = scale.cuda()
    for key, got in r.items():
        want = plain[key] * sc
        assert bool(torch.isfinite(want).all())
        assert torch.equal(got, want), f"{name} {key}: {int((got != want).any(1).sum())} rows are not the scaled rows of the plain run"
