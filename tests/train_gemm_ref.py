"""Case tables, operand builders and references of the split-bf16 training Linears (csrc/train_gemm.hip, train_gemm_tiled.h,
train_fwd.hip, train_bwd.hip, train_shared.h).  CPU only, fp64 / int64.  Imported by tests/test_train_gemm_ref.py (CPU: the
premises below) and tests/test_gpu_train_gemm_edges.py.

The operator:  y = act([x0 | x1]) . W^T + b,   g_x = (dY . W) * act'([x0 | x1]),   dW = dY^T . act([x0 | x1]),   db = sum_n dY.
The kernels split every operand v = hi + lo (hi = bf16(v), lo = bf16(v - hi), round to nearest even) and add the three products
hi*hi + hi*lo + lo*hi per k in fp32.

A. EXACT CASES.  Operands are small integers, so every product and every partial sum is an integer below 2^24: exact in fp32 in
any summation order, whatever the kernel's tiling.  The result must EQUAL the integer reference -- no tolerance.
  * dense: integers in [-8, 8] (bf16 holds them: lo = 0); the largest partial sum is 64 * max(K, N) + 8 = 768 072 at N = 12 001.
  * one-hot: one operand has one nonzero per row (+-2^s, s = 0..2, or a 16-bit integer), the other holds 16-bit integers (hi
    AND lo planes in use: hi + lo == v for every |v| < 2^17, tests/test_train_gemm_ref.py); every output entry is ONE product
    (+ the bias): |.| <= 65535 * 4 + 8 < 2^24.
  Activations: none, and LeakyReLU where it is the identity with derivative 1 -- strictly positive inputs; the zeros of a one-hot
  forward input pass it exactly too (leaky(0) = 0), and where the derivative matters the forward input is dense and positive.
  The integer matmul is done by the fp64 BLAS (torch's int64 matmul takes 0.4 s per 8192 x 256 x 256 product, there are ~10^3):
  every partial sum is an integer below 2^53, so the fp64 product IS the int64 product -- int_matmul asserts that bound, and the
  CPU test compares it with torch.matmul on int64.

C. THE PER-ENTRY BOUND of the inexact cases (derived, not fitted).  For an entry summing n terms a_k * b_k (a = act(x)):

    |got - ref| <= c(n) * sum_k |a_k| |b_k|  +  e_act * sum_k |b_k|         c(n) = 2 * 2^-17 + 2^-18 + c_act + n * 2^-24

  * 2 * 2^-17: each operand is replaced by hi + lo, off by at most 2^-17 |v| (split4's comment in train_shared.h; two bf16
    roundings of relative 2^-9 each give 2^-18, the comment's figure is kept)
  * 2^-18: the dropped lo * lo product, |lo| <= 2^-9 |v| per operand
  * n * 2^-24: fp32 accumulation of n terms, the standard worst case (n - 1) u sum |t_i|; n = K (or N for the weight gradient)
    + 2 for the bias and the multiplication by act'(x), which are folded into the sum as one more term each
  * c_act = 2^-23 for LeakyReLU: the kernels form 0.01f * x in fp32 (0.01f is 0.01 (1 + d), |d| < 2^-24, and one rounding);
    0 for none
  * e_act: the absolute error of the kernels' sin / cos (hardware v_sin_f32 on a reduced argument).  It cannot be derived; it is
    MEASURED on the GPU through a 0/1 selection matrix (test_gpu_train_gemm_edges.py::test_sin_error_through_a_selection_matrix)
    and the bound uses twice the recorded maximum, E_SIN.
"""
import collections

import torch

U = 2.0 ** -24
ACTS = ("none", "leaky_relu", "sin")
# max |kernel - fp64| of sin (forward through the identity matrix: the hi + lo split of the value is part of it) and cos (input
# gradient, multiplied in after the accumulation), measured on an MI355X over 2^20 arguments per range; E_SIN is twice the largest.
E_SIN_MEASURED = {("sin", 2.0): 3.930e-06, ("cos", 2.0): 2.095e-07, ("sin", 30.0): 3.999e-06, ("cos", 30.0): 2.504e-07}
E_SIN = 2.0 * max(E_SIN_MEASURED.values())

K_STAGED, LS, NARROW, NARROW_X1, RESIDENT = "k_staged", "ls", "narrow", "narrow_x1", "resident"

# One shape of the table.  fwd / dgrad / wgrad: the path of the unpacked entry points; fwd_pk / dgrad_pk: of the packed ones (None:
# the packed entry point refuses the shape); fused: the one-pass backward takes the source (ops.linear_bwd_fused_ok).
# col0 > 0: the source is the SECOND source of a skip layer whose first is col0 columns wide (one-pass backward cases only).
Case = collections.namedtuple("Case", "group N in0 in1 out col0 fwd dgrad wgrad fwd_pk dgrad_pk fused")


def case_id(c):
    return f"{c.group}-N{c.N}-in{c.in0}+{c.in1}-out{c.out}" + (f"-at{c.col0}" if c.col0 else "")


def _cases():
    t = []

    def add(group, N, in0, in1, out, fwd, dgrad, wgrad, fwd_pk, dgrad_pk, fused, col0=0):
        t.append(Case(group, N, in0, in1, out, col0, fwd, dgrad, wgrad, fwd_pk, dgrad_pk, fused))
    # K-staged: N < 2048 -- every GEMM on the tiled kernels, no packed form
    for N in (1, 2, 63, 64, 65, 2047):
        for in0, in1, out in ((1, 0, 1), (3, 1, 2), (38, 2, 65), (129, 0, 257)):
            add("k_staged", N, in0, in1, out, K_STAGED, K_STAGED, K_STAGED, None, None, False)
    # ... or an output wider than 1024 columns (the input gradient, 16 columns, and only it, is layer-synchronous)
    add("k_staged", 2048, 16, 0, 1025, K_STAGED, LS, K_STAGED, None, LS, False)
    # layer-synchronous streaming kernels; a weight gradient wider than 256 x 256 stays K-staged
    for N in (2048, 2049, 2048 + 63):
        for in0, in1, out in ((1, 0, 1), (38, 2, 65), (69, 3, 64), (5, 7, 1024), (127, 1, 64), (128, 129, 257), (256, 1, 2)):
            add("ls", N, in0, in1, out, LS, LS, LS if out <= 256 else K_STAGED, LS, LS, False)
    # row-stream narrow kernels (K = 256, M <= 128) behind the packed entry points; 129 is the first width that must not
    for N in (2048, 2049):
        for M in (1, 2, 63, 64, 65, 127, 128, 129):
            add("narrow", N, 256, 0, M, LS, LS, LS, NARROW if M <= 128 else LS, LS, False)      # forward 256 -> M
            add("narrow", N, M, 0, 256, LS, LS, LS, LS, NARROW if M <= 128 else LS, False)      # input gradient 256 -> M
        for in1 in (1, 38, 128):                                                               # a skip layer's second source
            add("narrow", N, 256, in1, 256, LS, LS, LS, LS, NARROW_X1, False)
    # register-resident forward (N >= 8192); 8191 takes the streaming / row-stream kernels
    for N in (8191, 8192, 8193, 8192 + 31):
        big = N >= 8192
        for in1 in (0, 1, 2, 3, 4, 80):
            add("resident", N, 256, in1, 256, LS, LS, LS, RESIDENT if big else LS, NARROW_X1 if in1 else LS, big)
        for in0 in (1, 2, 4, 80):
            add("resident", N, in0, 0, 256, LS, LS, LS, RESIDENT if big else LS, NARROW, big)
        for out in (1, 128):
            add("resident", N, 256, 0, out, LS, LS, LS, RESIDENT if big else NARROW, LS, big)
    # one-pass backward (N >= 8192); 8191 takes the two launches
    for N in (8191, 8192, 8193, 8192 + 33):
        big = N >= 8192
        for in0 in (1, 2, 127, 128, 256):
            for out in (1, 2, 255, 256):
                fwd_pk = RESIDENT if big and ((out == 256 and (in0 == 256 or in0 <= 80)) or (in0 == 256 and out <= 128)) else \
                    NARROW if in0 == 256 and out <= 128 else LS
                add("bwd", N, in0, 0, out, LS, LS, LS, fwd_pk, NARROW if (out == 256 and in0 <= 128) else LS, big)
                if in0 <= 128:
                    for col0 in (64, 256):
                        add("bwd", N, in0, 0, out, None, None, None, None, None, big, col0=col0)
    return t


CASES = _cases()
N_MAX = 12001   # the largest batch of the GPU file (the isolation cases of the one-pass kernels)

# One representative per path for the isolation / bound tests: ragged N and ragged widths.  (N, in0, in1, out)
REPRESENTATIVES = {
    "k_staged": (2047, 38, 3, 65),
    "ls": (2048 + 63, 69, 38, 67),
    "narrow": (2049, 256, 0, 65),
    "narrow_dgrad": (2049, 69, 0, 256),
    "narrow_x1": (2049, 256, 38, 256),
    "resident": (8192 + 31, 256, 69, 256),
    "resident_narrow": (8193, 38, 0, 256),
    "bwd": (12001, 69, 0, 255),
    "bwd_wide": (8192 + 33, 256, 0, 65),
}


def _gen(*key):
    s = 0x5EED
    for k in key:
        s = (s * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ints(shape, lo, hi, *key):
    """seeded integers in [lo, hi] as int64"""
    return torch.randint(lo, hi + 1, shape, generator=_gen(*key), dtype=torch.int64)


def int_matmul(a, b):
    """a @ b of int64 matrices, by the fp64 BLAS: exact while every partial sum stays below 2^53 (asserted)"""
    assert a.dtype == torch.int64 and b.dtype == torch.int64
    assert a.shape[1] * max(int(a.abs().max()), 1) * max(int(b.abs().max()), 1) < 2 ** 53
    return (a.double() @ b.double()).to(torch.int64)


def max_partial_sum(K, N, amax, bmax, bias=8):
    """the largest |partial sum| any order of the additions can meet in the three GEMMs of an exact case"""
    return max(K, N) * amax * bmax + bias


# ------------------------------------------------------------------------------------------------ A: exact operands
def dense_operands(c, positive):
    """x [N, in0 + in1], W [out, col0 + in0 + in1], b [out], dY [N, out]: int64 in [-8, 8]; positive: x in [1, 8] (LeakyReLU is the
    identity there, its derivative 1)"""
    K = c.in0 + c.in1
    x = ints((c.N, K), -8, 8, "x", c.N, K)
    if positive:
        x = x.abs() + (x == 0).long()
    W = ints((c.out, c.col0 + K), -8, 8, "W", c.out, c.col0 + K)
    b = ints((c.out,), -8, 8, "b", c.out)
    dY = ints((c.N, c.out), -8, 8, "dY", c.N, c.out)
    return x, W, b, dY


def dense_refs(c, x, W, b, dY):
    """(y, g_x, dW, db) int64; W's columns col0.. are the source's"""
    Ws = W[:, c.col0:]
    return int_matmul(x, Ws.t().contiguous()) + b, int_matmul(dY, Ws), int_matmul(dY.t().contiguous(), x), dY.sum(0)


def _pow2(n, positive):
    v = 2 ** (n % 3)
    return v if positive else torch.where((n // 3) % 2 == 1, -v, v)


def onehot_forward(c, positive):
    """x one-hot at column n mod K with +-2^s, W 16-bit integers: y[n, o] = W[o, n mod K] * x_n + b[o]"""
    K = c.in0 + c.in1
    n = torch.arange(c.N)
    v = _pow2(n, positive)
    x = torch.zeros(c.N, K, dtype=torch.int64)
    x[n, n % K] = v
    W = ints((c.out, K), -65535, 65535, "W16", c.out, K)
    b = ints((c.out,), -8, 8, "b", c.out)
    y = W.t()[n % K] * v[:, None] + b
    return x, W, b, y


def onehot_dgrad(c, positive):
    """dY one-hot at column n mod out with +-2^s: g_x[n, k] = W[n mod out, col0 + k] * dY_n; the forward input x is dense, positive
    where the activation is LeakyReLU (derivative 1)"""
    K = c.in0 + c.in1
    n = torch.arange(c.N)
    v = _pow2(n, False)
    dY = torch.zeros(c.N, c.out, dtype=torch.int64)
    dY[n, n % c.out] = v
    W = ints((c.out, c.col0 + K), -65535, 65535, "W16", c.out, c.col0 + K)
    x = ints((c.N, K), 1, 8, "xpos", c.N, K) if positive else ints((c.N, K), -8, 8, "x", c.N, K)
    g = W[n % c.out][:, c.col0:] * v[:, None]
    return dY, W, x, g


def onehot_wgrad(c, positive):
    """dY one-hot +-1, x one-hot 16-bit integers, the (o, k) pairs all different: dW[o, k] = dY_n x_n of the one row that holds the
    pair (0 elsewhere), db[o] = sum_n dY[n, o].  Rows are spread over the whole batch, the last row included; a batch with more
    rows than out * K pairs leaves the rest zero."""
    K = c.in0 + c.in1
    P = min(c.N, c.out * K)
    p = torch.arange(P)
    rows = c.N - 1 - (p * c.N) // P
    assert len(set(rows.tolist())) == P
    o, k = p % c.out, (p // c.out) % K
    # (p -> (o, k) is one-to-one on p < out * K)
    sgn = torch.where(p % 2 == 1, -1, 1)
    xv = ints((P,), 1, 65535, "x16", c.N, K)
    if not positive:
        xv = xv * torch.where((p // 2) % 2 == 1, -1, 1)
    dY = torch.zeros(c.N, c.out, dtype=torch.int64)
    x = torch.zeros(c.N, K, dtype=torch.int64)
    dY[rows, o] = sgn
    x[rows, k] = xv
    dW = torch.zeros(c.out, K, dtype=torch.int64)
    dW[o, k] = sgn * xv
    return x, dY, dW, dY.sum(0)


# ------------------------------------------------------------------------------------------------ the split, emulated
def split(v):
    """fp32 -> (hi, lo) fp32 holding bf16 values, round to nearest even (train_shared.h split4)"""
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    return hi, lo


def emulate_gemm(a, b, reverse=False):
    """sum_k a[n, k] b[m, k] as the kernels form it -- three bf16 products per k, added in fp32 one k after the other (forward or
    reversed order) -- on fp32 CPU tensors"""
    ah, al = split(a)
    bh, bl = split(b)
    K = a.shape[1]
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    for k in (range(K - 1, -1, -1) if reverse else range(K)):
        for p, q in ((ah, bh), (ah, bl), (al, bh)):
            acc = acc + p[:, k:k + 1] * q[:, k][None, :]
    return acc


# ------------------------------------------------------------------------------------------------ C: fp64 references and the bound
def act64(x, act):
    if act == "leaky_relu":
        return torch.where(x > 0, x, 0.01 * x)     # (NaN: NaN)
    if act == "sin":
        return torch.sin(x)                         # (+-Inf, NaN: NaN)
    return x


def dact64(x, act):
    if act == "leaky_relu":
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.01))   # (NaN: 0.01, as torch's leaky_relu backward)
    if act == "sin":
        return torch.cos(x)
    return torch.ones_like(x)


def c_of(n_terms, act):
    """the relative part of the bound (module docstring)"""
    return 2 * 2.0 ** -17 + 2.0 ** -18 + (2.0 ** -23 if act == "leaky_relu" else 0.0) + (n_terms + 2) * U


def e_act_of(act):
    if act != "sin":
        return 0.0
    assert E_SIN is not None, "E_SIN is measured on the GPU first"
    return E_SIN


def float_refs(x, W, b, dY, act, e_act=None):
    """fp64 references and per-entry bounds of the three GEMMs on fp32 CPU operands (any of them may hold non-finite values).
    -> dict name -> (ref, bound)"""
    e = e_act_of(act) if e_act is None else e_act
    xd, Wd, dYd = x.double(), W.double(), dY.double()
    a, da = act64(xd, act), dact64(xd, act)
    N, K = x.shape
    out = {}
    y = a @ Wd.t() + (b.double() if b is not None else 0.0)
    S = a.abs() @ Wd.abs().t() + (b.double().abs() if b is not None else 0.0)
    out["y"] = (y, c_of(K, act) * S + e * Wd.abs().sum(1)[None, :])
    acc = dYd @ Wd
    Sg = dYd.abs() @ Wd.abs()
    out["g"] = (acc * da, c_of(W.shape[0], act) * Sg * da.abs() + e * Sg)
    out["dW"] = (dYd.t() @ a, c_of(N, act) * (dYd.abs().t() @ a.abs()) + e * dYd.abs().sum(0)[:, None])
    out["db"] = (dYd.sum(0), (N + 2) * U * dYd.abs().sum(0))
    return out


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the finite entries of ref (a zero bound asks for equality)"""
    fin = torch.isfinite(ref)
    err = (got.double() - ref).abs()[fin]
    bd = bound[fin]
    r = torch.where(bd > 0, err / bd.clamp(min=1e-300), torch.where(err > 0, torch.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ B: non-finite placement
def poison(t, last_col=None):
    """One NaN, one +Inf and one -Inf at three distinct rows of a copy of t [N, C]: the NaN in the LAST row, the +Inf in the last
    valid column of a middle row, the -Inf in row 0 (or 1), column 0.  -> (poisoned copy, [(row, col)])"""
    N, C = t.shape
    assert N >= 3
    t = t.clone()
    spots = [(N - 1, C // 2, float("nan")), (N // 2, C - 1, float("inf")), (1 if N > 3 else 0, 0, float("-inf"))]
    for r, col, v in spots:
        t[r, col] = v
    return t, [(r, col) for r, col, _ in spots]


def uniform(shape, lo, hi, *key):
    return (torch.rand(shape, generator=_gen(*key), dtype=torch.float64) * (hi - lo) + lo).float()
