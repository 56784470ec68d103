"""The hash-table scatter (csrc/backward.hip hash_backward_kernel) and the other users of accumulate() (csrc/common.h) at their
edges, in the default mode (fp32 atomics) and in the deterministic mode (2^-40 fixed point), against plain fp64 references.

Scatter: every input of tests/scatter_ref.py through the three entry points (na_hash_encode_backward, _backward_rows at two odd
row pitches, _jvp_backward), every table entry held to the derived bound of scatter_ref.bound; level 0 of input G and the
limits of the fixed-point format (bypass at 2^20, |sum| < 2^23, non-finite addends) on exact integers, bit for bit."""
import contextlib

import pytest
import torch

import oracle as O
import scatter_ref as S
from oracle.procedural import proc_uniform

pytestmark = pytest.mark.gpu

ENTRIES = ("plain", "rows41", "rows77", "jvp")
NA_EWORKSPACE = -5   # include/nerf_atlas_amd.h


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@contextlib.contextmanager
def mode(det):
    """the deterministic mode is process-wide: always switched off again"""
    from nerf_atlas_amd import config
    if det:
        config.set_deterministic(True)
    try:
        yield
    finally:
        if det:
            config.set_deterministic(False)


def junk(shape, seed):
    return torch.from_numpy(proc_uniform(shape, seed, 1000.0))   # what the kernel must NOT read: large, so that it shows


def scatter(ops, entry, x, g, t):
    """one scatter through one entry point -> [8, 65536, 4] on the host"""
    N = x.shape[0]
    xc = x.cuda()
    if entry == "plain":   # rows [x's gradient (unused) | 32 feature gradients]
        out = ops.hash_encode_backward(xc, torch.cat([junk((N, 3), 41), g], dim=1).cuda(), True)
    elif entry in ("rows41", "rows77"):
        ld, col0 = (41, 6) if entry == "rows41" else (77, 9)
        rows = junk((N, ld), 42)
        rows[:, col0:col0 + 32] = g
        out = ops.hash_encode_backward_rows(xc, rows.cuda(), col0)
    else:
        out = ops.hash_encode_jvp_backward(xc, t.cuda(), g.cuda(), False)
    return out.cpu()


def run_all(ops, x, g, t, det, entries=ENTRIES):
    with mode(det):
        return {e: scatter(ops, e, x, g, t) for e in entries}


@pytest.mark.parametrize("name", S.CASES)
def test_scatter_meets_the_per_entry_bound_in_both_modes(ops, name):
    """Every table entry of every entry point within (k + 8) u mag (+ k 2^-40 + u |ref| in the deterministic mode) of the fp64
    reference; deterministic and default results within the sum of their bounds of each other; the rows entry bit-equal to the plain
    one in the deterministic mode; level 0 of input G (exact arithmetic) bit-equal to the reference everywhere."""
    x, g, t = S.case(name)
    got = {det: run_all(ops, x, g, t, det) for det in (False, True)}
    for entry in ENTRIES:
        tan = entry == "jvp"
        ref, mag, cnt = S.reference(name, tan)
        for det in (False, True):
            r = S.worst_ratio(got[det][entry], ref, mag, cnt, det, tan)
            print(f"\n[scatter {name} {entry} det={int(det)}] worst error / bound {r:.3f}")
            assert r <= 1.0, (name, entry, det, r)
            if name == "G":
                assert torch.equal(got[det][entry][0], ref[0].float()), (entry, det)
        both = S.bound(ref, mag, cnt, False, tan) + S.bound(ref, mag, cnt, True, tan)
        assert bool(((got[True][entry].double() - got[False][entry].double()).abs() <= both).all()), (name, entry)
    assert torch.equal(got[True]["rows41"], got[True]["plain"]) and torch.equal(got[True]["rows77"], got[True]["plain"])


@pytest.mark.parametrize("name", [c for c in S.CASES if c != "G"])
def test_deterministic_scatter_is_reproducible_and_independent_of_the_order_of_the_waves(ops, name):
    """Deterministic mode, N padded to whole waves: two calls give the same bits, and so does the input permuted in aligned chunks
    of 64 samples -- a wave is 64 consecutive samples, its merged sums depend on its own lanes only, everything behind it is
    integer addition.  The rows entry equals the plain entry bit for bit.
    The permutation says something for C, D65 and larger, E and F only: A's four chunks are identical (the permuted input IS the
    input) and B, D1, D63 are a single chunk -- for those this test is the repeat and the rows == plain property."""
    x, g, t = S.pad64(*S.case(name))
    n = x.shape[0]
    assert n % 64 == 0
    chunks = torch.from_numpy(S._order(n // 64, 3300))
    if torch.equal(chunks, torch.arange(n // 64)):   # (a seeded order of two or three chunks can be the identity)
        chunks = chunks.flip(0)
    perm = (chunks[:, None] * 64 + torch.arange(64)[None, :]).reshape(-1)
    assert n == 64 or not torch.equal(perm, torch.arange(n))
    a = run_all(ops, x, g, t, True)
    b = run_all(ops, x, g, t, True)
    c = run_all(ops, x[perm].contiguous(), g[perm].contiguous(), t[perm].contiguous(), True)
    for entry in ENTRIES:
        assert float(a[entry].abs().max()) > 0
        assert torch.equal(a[entry], b[entry]), (name, entry, "repeat")
        assert torch.equal(a[entry], c[entry]), (name, entry, "chunks of 64 permuted")
    assert torch.equal(a["rows41"], a["plain"]) and torch.equal(a["rows77"], a["plain"])


def test_fixed_point_limits_on_exact_integers(ops):
    """csrc/common.h: an addend of exactly 2^20 and one of 2^22 bypass the accumulator (as the merged sum of their wave, which is
    what the threshold sees: tests/test_scatter_ref.py asserts the merged sums on the CPU), the largest fp32 below 2^20 stays in
    it, twelve addends of 2^19 sum to 6291456 < 2^23 inside it -- each into a row that small-integer addends of other waves reach
    through the fixed-point path.  All level-0 arithmetic is exact (scatter_ref.limits_input), so level 0 must equal the reference bit for bit in
    both modes; the other levels meet the bound."""
    x, g = S.limits_input()
    ref, mag, cnt = S.scatter_ref(x, g)
    row = int(O.hash_corner_indices(x[:1])[0, 0, 0])
    for det in (False, True):
        got = run_all(ops, x, g, None, det, ("plain", "rows41"))
        for entry, out in got.items():
            print(f"\n[limits {entry} det={int(det)}] origin row {out[0, row].tolist()} expected {ref[0, row].tolist()}")
            assert torch.equal(out[0, row].double(), ref[0, row]), (entry, det)
            assert torch.equal(out[0], ref[0].float()), (entry, det)
            r = S.worst_ratio(out, ref, mag, cnt, det)
            assert r <= 1.0, (entry, det, r)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_gradient_reads_non_finite_in_exactly_the_entries_it_reaches(ops, bad):
    """One sample whose gradient at one level is NaN / +Inf: the kernel multiplies every corner weight by it like the reference does,
    so the set of non-finite table entries equals the fp64 reference's set in both modes (the deterministic mode sends such addends
    round the accumulator); every other entry still meets the bound."""
    x, g, t = S.case("D257")
    g = g.clone()
    g[100, 12:16] = bad
    g[37, 20:24] = bad
    for det in (False, True):
        got = run_all(ops, x, g, t, det)
        for entry in ENTRIES:
            tan = entry == "jvp"
            ref, mag, cnt = S.scatter_ref(x, g, t if tan else None)
            nonfinite = ~torch.isfinite(ref)
            assert int(nonfinite.sum()) >= 32 and torch.equal(nonfinite, ~torch.isfinite(mag))
            assert torch.equal(~torch.isfinite(got[entry]), nonfinite), (entry, det)
            r = S.worst_ratio(got[entry], ref, mag, cnt, det, tan, where=~nonfinite)
            print(f"\n[non-finite {bad} {entry} det={int(det)}] worst error / bound of the finite entries {r:.3f}")
            assert r <= 1.0, (entry, det, r)


# ------------------------------------------------------------------------------------------ weight gradients
IN0, IN1, OUT = 38, 3, 65
ACT64 = {"none": lambda v: v, "leaky_relu": lambda v: torch.where(v > 0, v, 0.01 * v), "sin": torch.sin}
# the bars of the default-mode tests of the same entry points, of the largest entry of the tensor:
#   exact fp32 (linear_wgrad_kernel):          2e-4, tests/test_gpu_backward.py::test_linear_backward
#   split bf16, K-staged (linear_tn_kernel):   3e-5, tests/test_gpu_train_gemm.py::test_layer_synchronous_gemms_vs_fp64
WGRAD_BAR = {False: 2e-4, True: 3e-5}


def _wgrad(ops, x0, x1, gy, act, bias, split, det):
    with mode(det):
        dW, db = ops.linear_wgrad(x0, gy, act, x1=x1, want_bias=bias, split_bf16=split)
        return dW.cpu(), (db.cpu() if bias else None)


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split_bf16"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["none", "leaky_relu", "sin"])
@pytest.mark.parametrize("N", [1100, 1900])
def test_weight_gradient_in_both_modes(ops, N, act, bias, split):
    """2 - 4 slices of N with a ragged last one, a concatenated input of 38 + 3 columns, 65 outputs: against fp64 at the bar of
    the existing default-mode test of the entry point (WGRAD_BAR), default and deterministic mode; deterministic repeats bit for
    bit and agrees with the default mode within twice the bar."""
    if split:
        assert not ops.train_gemm_packed_ok(N, OUT), "this batch must run the K-staged kernel (linear_tn_kernel)"
    x0 = torch.from_numpy(proc_uniform((N, IN0), 3401, 2.0))
    x1 = torch.from_numpy(proc_uniform((N, IN1), 3402, 2.0))
    gy = torch.from_numpy(proc_uniform((N, OUT), 3403, 1.0))
    dW_ref = gy.double().t() @ ACT64[act](torch.cat([x0, x1], dim=1).double())
    db_ref = gy.double().sum(dim=0)
    bar = WGRAD_BAR[split]
    args = (ops, x0.cuda(), x1.cuda(), gy.cuda(), act, bias, split)
    dW, db = _wgrad(*args, False)
    dWd, dbd = _wgrad(*args, True)
    dWd2, dbd2 = _wgrad(*args, True)
    rel = lambda a, r: float((a.double() - r).abs().max() / r.abs().max())
    print(f"\n[wgrad N={N} {act} split={int(split)}] dW default {rel(dW, dW_ref):.2e} deterministic {rel(dWd, dW_ref):.2e}")
    assert rel(dW, dW_ref) <= bar and rel(dWd, dW_ref) <= bar
    assert torch.equal(dWd, dWd2)
    assert rel(dWd, dW.double()) <= 2 * bar
    if bias:
        assert rel(db, db_ref) <= bar and rel(dbd, db_ref) <= bar
        assert torch.equal(dbd, dbd2)
        assert rel(dbd, db.double()) <= 2 * bar
    else:
        assert db is None and dbd is None


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "split_bf16"])
def test_weight_gradient_of_small_integers_is_exact_in_both_modes(ops, split):
    """x and dY integers of magnitude <= 256 (exact in bf16, so the split is exact), no activation: every product and every partial
    sum is an integer below 2^24, so dW and db must be exactly the integer result in both modes.  Entry (7, 5): 16 rows of the first
    slice hold 256 x 256, that slice's sum reaches 2^20 and bypasses the accumulator while the last slice adds through it."""
    N = 1100
    if split:
        assert not ops.train_gemm_packed_ok(N, OUT)
    x0 = torch.from_numpy(proc_uniform((N, IN0), 3411, 8.0)).round()
    x1 = torch.from_numpy(proc_uniform((N, IN1), 3412, 8.0)).round()
    gy = torch.from_numpy(proc_uniform((N, OUT), 3413, 8.0)).round()
    x0[:16, 5] = 256.0
    gy[:16, 7] = 256.0
    x0[16:, 5] = x0[16:, 5].abs() + 1.0   # (positive products: the first slice stays at 2^20 or more, the later slices add through
    gy[16:, 7] = gy[16:, 7].abs() + 1.0   # the fixed-point path; slices are 512 rows in the split-bf16 kernel, 1024 in the fp32 one)
    dW_ref = gy.double().t() @ torch.cat([x0, x1], dim=1).double()
    db_ref = gy.double().sum(dim=0)
    first = float((gy[:512, 7].double() * x0[:512, 5].double()).sum())
    assert first >= 2.0 ** 20 and float((gy[1024:, 7] * x0[1024:, 5]).sum()) > 0 and float(dW_ref.abs().max()) < 2.0 ** 24 and float(dW_ref[7, 5]) > first
    for det in (False, True):
        dW, db = _wgrad(ops, x0.cuda(), x1.cuda(), gy.cuda(), "none", True, split, det)
        assert torch.equal(dW.double(), dW_ref), (det, float((dW.double() - dW_ref).abs().max()))
        assert torch.equal(db.double(), db_ref), det


# ------------------------------------------------------------------------------------------ scalar reductions
REDUCE_N = (1, 255, 262144 + 77)   # the last: beyond eikonal's grid cap (1024 blocks of 256), the stride loop runs


def _twice(fn, det):
    with mode(det):
        return float(fn()), float(fn())


@pytest.mark.parametrize("N", REDUCE_N)
def test_eikonal_loss_in_both_modes(ops, N):
    """mean((|n| - 1)^2) against fp64.  No earlier test holds this operator alone, so the bar is derived: with len = |n| and
    d = len - 1, len carries <= 3 u relative (three squares, two sums, halved by the root, plus the root's own rounding), d another
    u |d|, so d * d is off by <= 2 |d| (3 u len + u |d|) + u d^2 <= 6 u len |d| + 4 u d^2;
    a thread adds <= 2 terms, the block tree 8 + 2 levels, the scale by 1/N and its rounding 2 more, the blocks' fp32 atomics
    <= (blocks - 1) u of the (all positive) total: (12 + blocks) u ref.  Deterministic: + blocks 2^-40 + u ref, bit-identical twice."""
    nrm = torch.from_numpy(proc_uniform((3, N), 3421, 1.5))
    ln = nrm.double().norm(dim=0)
    d = ln - 1.0
    ref = float((d * d).mean())
    blocks = min((N + 255) // 256, 1024)
    bar = float((6 * S.U * ln * d.abs() + 4 * S.U * d * d).mean()) + (12 + blocks) * S.U * ref
    nc = nrm.cuda()
    a, _ = _twice(lambda: ops.eikonal_loss(nc), False)
    b, b2 = _twice(lambda: ops.eikonal_loss(nc), True)
    print(f"\n[eikonal N={N}] error / bar: default {abs(a - ref) / bar:.3f} deterministic {abs(b - ref) / (bar + blocks * 2.0 ** -40 + S.U * ref):.3f}")
    assert abs(a - ref) <= bar
    assert abs(b - ref) <= bar + blocks * 2.0 ** -40 + S.U * ref and b == b2


@pytest.mark.parametrize("N", REDUCE_N)
def test_laplace_density_beta_gradient_in_both_modes(ops, N):
    """d/dbeta of the Laplace density against fp64 autograd at the bar of tests/test_gpu_backward.py::test_laplace_density_backward
    (2e-4 |ref| + 1e-2), default and deterministic; deterministic bit-identical twice; g_sdf is the same in both modes."""
    sdf = torch.from_numpy(proc_uniform((N,), 3431, 0.6))
    go = torch.from_numpy(proc_uniform((N,), 3432, 1.0))
    for beta in (0.1, 0.37):
        s = sdf.double().requires_grad_()
        b = torch.tensor(float(torch.tensor(beta)), dtype=torch.float64, requires_grad=True)   # (the fp32 value the kernel reads)
        ((1 / b * O.laplace_cdf(-s, b)) * go.double()).sum().backward()
        ref = float(b.grad)
        bar = 2e-4 * abs(ref) + 1e-2
        args = (sdf.cuda(), torch.tensor(beta).cuda(), go.cuda())
        a, _ = _twice(lambda: ops.laplace_density_backward(*args)[1], False)
        d, d2 = _twice(lambda: ops.laplace_density_backward(*args)[1], True)
        print(f"\n[laplace d/dbeta N={N} beta={beta}] ref {ref:.6g} default {a:.6g} deterministic {d:.6g}")
        assert abs(a - ref) <= bar and abs(d - ref) <= bar and d == d2
        with mode(True):
            gs_det = ops.laplace_density_backward(*args)[0]
        assert torch.equal(gs_det, ops.laplace_density_backward(*args)[0])


@pytest.mark.parametrize("N", REDUCE_N)
def test_row_sqnorm_mean_in_both_modes(ops, N):
    """mean of the squared row norms against fp64 at the bar of tests/test_gpu_ae.py::test_row_operators_against_autograd_in_fp64
    (2e-6 relative), default and deterministic; deterministic bit-identical twice."""
    x = torch.from_numpy(proc_uniform((N, 32), 3441, 2.0))
    ref = float(torch.linalg.norm(x.double(), dim=-1).square().mean())
    xc = x.cuda()
    a, _ = _twice(lambda: ops.row_sqnorm_mean(xc), False)
    b, b2 = _twice(lambda: ops.row_sqnorm_mean(xc), True)
    print(f"\n[row_sqnorm_mean N={N}] relative error: default {abs(a - ref) / ref:.2e} deterministic {abs(b - ref) / ref:.2e}")
    assert abs(a - ref) <= 2e-6 * ref and abs(b - ref) <= 2e-6 * ref and b == b2


# ------------------------------------------------------------------------------------------ workspace errors
def test_a_too_small_deterministic_workspace_is_refused_before_anything_is_written(ops):
    from nerf_atlas_amd import _lib, config
    lib = _lib.load()
    x, g, _ = S.case("D65")
    xc, gc = x.cuda(), g.cuda()
    ws = torch.zeros(4096, device="cuda", dtype=torch.uint8)
    out = torch.full((8, 65536, 4), 7.0, device="cuda")
    try:
        _lib.check(lib.na_set_deterministic(ws.data_ptr(), ws.numel()))
        with pytest.raises(_lib.NaError) as err:
            ops.hash_encode_backward(xc, gc, False)
        assert err.value.code == NA_EWORKSPACE and "deterministic workspace 4096 < 16777216 bytes" in str(err.value), str(err.value)
        rc = lib.na_hash_encode_backward(ops._ptr(xc), x.shape[0], ops._ptr(gc), 0, ops._ptr(out), ops._stream())
        assert rc == NA_EWORKSPACE
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and int(ws.count_nonzero()) == 0
    finally:
        config.set_deterministic(False)
    # the normal state is back: the default mode computes, the deterministic mode gets its own workspace again
    ref, mag, cnt = S.reference("D65", False)
    assert S.worst_ratio(ops.hash_encode_backward(xc, gc, False), ref, mag, cnt, False) <= 1.0
    with mode(True):
        assert S.worst_ratio(ops.hash_encode_backward(xc, gc, False), ref, mag, cnt, True) <= 1.0
