"""CPU tests of the premises tests/train_gemm_ref.py rests on (the GPU file tests/test_gpu_train_gemm_edges.py takes them as
given): the bf16 split holds every integer the exact cases use, no partial sum of an exact case leaves fp32's integers, a torch
emulation of the three-product split reproduces the integer references in either summation order, the fp64 BLAS product is the
int64 product, the table names every path, and the per-entry bound holds for the emulation with margin."""
import pytest
import torch

import train_gemm_ref as R


def test_hi_plus_lo_is_every_integer_below_2_17():
    v = torch.arange(-(2 ** 17) + 1, 2 ** 17, dtype=torch.float32)
    hi, lo = R.split(v)
    assert torch.equal(hi + lo, v)
    assert torch.equal(hi.to(torch.bfloat16).float(), hi) and torch.equal(lo.to(torch.bfloat16).float(), lo)
    small = torch.arange(-8, 9, dtype=torch.float32)
    assert torch.equal(R.split(small)[1], torch.zeros(17)), "the dense family leaves the lo plane empty"
    assert bool((R.split(v)[1] != 0).any()), "the 16-bit family uses it"


def test_no_partial_sum_of_an_exact_case_leaves_the_fp32_integers():
    assert max(c.N for c in R.CASES) <= R.N_MAX == 12001
    for c in R.CASES:
        K = c.in0 + c.in1
        assert R.max_partial_sum(max(K, c.out), c.N, 8, 8) < 2 ** 24, c         # dense: any GEMM of the three, any order
        assert 65535 * 4 + 8 < 2 ** 24 and c.N < 2 ** 24                         # one-hot: one product + bias; db = a count
    assert R.max_partial_sum(1025, R.N_MAX, 8, 8) == 768072


def test_fp64_blas_product_is_the_int64_product():
    for (n, k, m), top in (((65, 294, 257), 8), ((2049, 69, 64), 8), ((300, 1025, 16), 65535), ((12001, 3, 5), 65535)):
        a, b = R.ints((n, k), -top, top, "a", n, k), R.ints((k, m), -top, top, "b", k, m)
        assert torch.equal(R.int_matmul(a, b), torch.matmul(a, b))
    with pytest.raises(AssertionError):
        R.int_matmul(torch.full((1, 4), 2 ** 40), torch.full((4, 1), 2 ** 12))


SMALL = [c for c in R.CASES if c.group == "k_staged" and c.N in (2, 65) and c.out <= 65]


@pytest.mark.parametrize("c", SMALL, ids=R.case_id)
def test_emulated_split_reproduces_the_integer_references_in_either_order(c):
    for positive in (False, True):
        x, W, b, dY = R.dense_operands(c, positive)
        y, g, dW, db = R.dense_refs(c, x, W, b, dY)
        for rev in (False, True):
            assert torch.equal(R.emulate_gemm(x.float(), W.float(), rev) + b.float(), y.float())
            assert torch.equal(R.emulate_gemm(dY.float(), W.t().contiguous().float(), rev), g.float())
            assert torch.equal(R.emulate_gemm(dY.t().contiguous().float(), x.t().contiguous().float(), rev), dW.float())
        x, W, b, y = R.onehot_forward(c, positive)
        dY, Wg, xg, g = R.onehot_dgrad(c, positive)
        xw, dYw, dW, db = R.onehot_wgrad(c, positive)
        for rev in (False, True):
            assert torch.equal(R.emulate_gemm(x.float(), W.float(), rev) + b.float(), y.float())
            assert torch.equal(R.emulate_gemm(dY.float(), Wg.t().contiguous().float(), rev), g.float())
            assert torch.equal(R.emulate_gemm(dYw.t().contiguous().float(), xw.t().contiguous().float(), rev), dW.float())
        assert torch.equal(dYw.sum(0), db)


@pytest.mark.parametrize("c", [c for c in R.CASES if (c.N, c.group) in ((2047, "k_staged"), (2049, "narrow"), (8193, "bwd"))][::3], ids=R.case_id)
def test_one_hot_operands_are_what_they_claim(c):
    K = c.in0 + c.in1
    x, W, b, y = R.onehot_forward(c, False)
    assert bool(((x != 0).sum(1) == 1).all()) and int(W.abs().max()) <= 65535 and int(y.abs().max()) < 2 ** 24
    assert torch.equal(y, R.int_matmul(x, W.t().contiguous()) + b)
    dY, Wg, xg, g = R.onehot_dgrad(c, True)
    assert bool(((dY != 0).sum(1) == 1).all()) and bool((xg > 0).all())
    assert torch.equal(g, R.int_matmul(dY, Wg)[:, c.col0:])
    xw, dYw, dW, db = R.onehot_wgrad(c, False)
    hits = R.int_matmul((dYw != 0).long().t().contiguous(), (xw != 0).long())
    assert int(hits.max()) <= 1 and int(hits.sum()) == min(c.N, c.out * K), "each dW entry receives at most one product"
    assert bool((xw[c.N - 1] != 0).any()), "the last row of the batch is in use"
    assert torch.equal(dW, R.int_matmul(dYw.t().contiguous(), xw))


def test_table_names_every_path():
    P = lambda f: {getattr(c, f) for c in R.CASES}
    assert P("fwd") == {R.K_STAGED, R.LS, None} and P("dgrad") == {R.K_STAGED, R.LS, None} and P("wgrad") == {R.K_STAGED, R.LS, None}
    assert P("fwd_pk") == {None, R.LS, R.NARROW, R.RESIDENT}
    assert P("dgrad_pk") == {None, R.LS, R.NARROW, R.NARROW_X1}
    assert P("fused") == {False, True}
    # both sides of the two dispatch thresholds and of the widths where the path changes
    Ns = {c.N for c in R.CASES}
    assert {2047, 2048, 2049, 8191, 8192, 8193} <= Ns
    assert {(c.out, c.fwd_pk) for c in R.CASES if c.group == "narrow" and c.in0 == 256 and c.in1 == 0} >= {(128, R.NARROW), (129, R.LS)}
    assert any(c.fwd == R.K_STAGED and c.N == 2048 and c.out == 1025 for c in R.CASES)
    assert any(c.wgrad == R.K_STAGED and c.fwd == R.LS for c in R.CASES)
    assert {c.col0 for c in R.CASES if c.group == "bwd" and c.in0 <= 128} == {0, 64, 256}
    assert (38, 2) in {(c.in0, c.in1) for c in R.CASES}, "sources ragged, total not: K & 3 == 0 under the STRADDLE loader"
    assert len({R.case_id(c) for c in R.CASES}) == len(R.CASES)
    for name, (N, in0, in1, out) in R.REPRESENTATIVES.items():
        assert N <= R.N_MAX and (N % 64 != 0) and ((in0 + in1) % 4 != 0 or out % 4 != 0), name


@pytest.mark.parametrize("act", ["none", "leaky_relu"])
def test_bound_holds_for_the_emulation_with_margin(act):
    N, K, M = 48, 294, 40
    x, W = R.uniform((N, K), -2, 2, "x", 1), R.uniform((M, K), -0.1, 0.1, "W", 2)
    b, dY = R.uniform((M,), -1, 1, "b", 3), R.uniform((N, M), -1, 1, "dY", 4)
    refs = R.float_refs(x, W, b, dY, act)
    a32 = torch.where(x > 0, x, x * torch.tensor(0.01, dtype=torch.float32)) if act == "leaky_relu" else x
    d32 = torch.where(x > 0, 1.0, 0.01).float() if act == "leaky_relu" else torch.ones_like(x)
    worst = 0.0
    for rev in (False, True):
        got = {"y": R.emulate_gemm(a32, W, rev) + b, "g": R.emulate_gemm(dY, W.t().contiguous(), rev) * d32,
               "dW": R.emulate_gemm(dY.t().contiguous(), a32.t().contiguous(), rev), "db": dY.sum(0)}
        for k, v in got.items():
            worst = max(worst, R.worst_ratio(v, *refs[k]))
    assert 0.0 < worst < 0.5, worst
    # ... and is not slack by orders of magnitude: dropping the lo planes (a plain bf16 product) breaks it
    hi = lambda t: t.to(torch.bfloat16).float()
    assert R.worst_ratio(hi(a32) @ hi(W).t() + b, *refs["y"]) > 10.0


def test_non_finite_references_follow_torch():
    x = torch.tensor([[float("nan"), float("inf"), float("-inf"), -2.0, 3.0]], dtype=torch.float64)
    xl = x.clone().requires_grad_()
    torch.nn.functional.leaky_relu(xl, 0.01).sum().backward()
    assert torch.equal(R.dact64(x, "leaky_relu"), xl.grad) and float(R.dact64(x, "leaky_relu")[0, 0]) == 0.01
    a = R.act64(x, "leaky_relu")
    assert torch.isnan(a[0, 0]) and a[0, 1] == float("inf") and a[0, 2] == float("-inf")
    assert bool(torch.isnan(R.act64(x, "sin")[0, :3]).all()) and bool(torch.isnan(R.dact64(x, "sin")[0, :3]).all())
    t, spots = R.poison(torch.zeros(7, 5))
    assert sorted(r for r, _ in spots) == [1, 3, 6] and (6, 2) in spots and (3, 4) in spots and int((~torch.isfinite(t)).sum()) == 3
