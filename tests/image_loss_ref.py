"""fp64 restatement of the loss wrapper (include/nerf_atlas_amd.h "The reference's loss wrapper") with a bound on what
an fp32 evaluation of the same definition may differ from it, and the input generators of the image-loss tests.

The definition (runner.py:552-594, src/utils.py:198-204, 279-314 of the reference), for got, ref [P,3]:
    gamma   (G != 1)  a = f(clamp(got, 1e-10)), b = f(ref);  f = sqrt at G == 0.5, pow(., G) otherwise
    tone    (if set)  v <- v / (1 + v)
    spaces            rgb: v | hsv: (0, 0, max v) | luminance: one channel | xyz: M v / 0.17697
    per space         l2 = mean d^2, l1 = mean |d|, rmse = sqrt(clamp(l2, 1e-10)) over P x channels (hsv 3, luminance 1)
    loss              mean over the spaces of the mean over the functions
The constants are the fp32 roundings the reference and the kernel multiply with (an fp32 matrix, Python floats times fp32 tensors).

THE BOUNDS are first-order forward error bounds, u = 2^-24, every operation of the fp32 evaluation counted where it happens and every
cancelling sum bounded relative to the sum of the |terms|, never to the result:
    sqrt 1 u, pow 4 u (a 2-ulp library function), a / (1 + a) 3 u (sum, quotient, and the sum's error through the quotient),
    a 3-term dot product 3 u sum |terms|, / 0.17697 one more, a difference u (|A| + |B|) plus the operands' errors,
    a sum of n non-negative terms `depth` u times the sum: depth = the terms one thread adds serially (channels x passes) + 6 (the
    wave's tree) + 3 (the four waves) + 2 (the division and the rounding of the mean; the rows are added in double),
    sqrt(clamp(mse)) E_mse / (2 rmse) + u rmse, and 4 u of the sum of the |terms| for the final combination.
The gradient's bound follows the backward kernel's expression the same way (see `restate`).  Where an fp32 evaluation may take the
other side of a kink -- |d| within its own error under l1, the two largest channels within their errors under hsv -- the bound
takes the whole jump: no element is excluded anywhere.  The result is doubled for the second-order terms.
"""
import numpy as np

U = 2.0 ** -24
SPACES = ("rgb", "hsv", "luminance", "xyz")          # bit order of NA_SPACE_*
CHANNELS = {"rgb": 3, "hsv": 3, "luminance": 1, "xyz": 3}
LUM = np.array([np.float32(0.2126), np.float32(0.7152), np.float32(0.0722)], dtype=np.float64)
XYZ = np.array([[0.49, 0.31, 0.2], [0.17697, 0.8124, 0.01063], [0.0, 0.01, 0.99]], dtype=np.float32).astype(np.float64)
XYZ_DIV = float(np.float32(0.17697))
CLAMP = float(np.float32(1e-10))
BLOCK, MAX_BLOCKS = 256, 256                          # csrc/image_loss.hip: kLossBlock, kLossMaxBlocks

# the table tools/gen_golden.py g30 records: (loss functions, colour spaces, tone map, gamma)
COMBOS = (
    [(("l2",), (s,), False, 1.0) for s in SPACES]
    + [(("l2",), ("rgb", "xyz", "hsv"), False, 1.0), (("l2",), ("luminance", "hsv"), False, 1.0)]
    + [(("l1",), ("rgb",), False, 1.0), (("rmse",), ("rgb",), False, 1.0), (("l2", "rmse"), ("rgb",), False, 1.0)]
    + [(("l2", "rmse"), ("rgb", "xyz", "hsv"), t, g) for t in (False, True) for g in (1.0, 0.5, 0.7, 2.2)]
    + [(("l1",), (s,), True, 0.5) for s in SPACES]
    + [(("l1",), ("luminance", "hsv"), True, 0.7), (("rmse",), ("luminance", "hsv"), False, 2.2), (("l1", "rmse"), ("xyz",), True, 2.2)]
)


def combo_name(c):
    return f"{'+'.join(c[0])}|{'+'.join(c[1])}|tone{int(c[2])}|G{c[3]}"


def kink_free_draw(P, seed):
    """got uniform in [1e-3, 1.2], ref in [0, 1] (fp32), every pixel redrawn until the two largest channels of got and of ref are more
    than 1e-3 apart, every |got_c - ref_c| > 1e-3 and |max got - max ref| > 1e-3"""
    rng = np.random.RandomState(seed)
    got, ref = np.empty((P, 3), np.float32), np.empty((P, 3), np.float32)
    todo = np.arange(P)
    while todo.size:
        g = rng.uniform(1e-3, 1.2, (todo.size, 3)).astype(np.float32)
        r = rng.uniform(0.0, 1.0, (todo.size, 3)).astype(np.float32)
        gs, rs = np.sort(g.astype(np.float64), axis=1), np.sort(r.astype(np.float64), axis=1)
        ok = ((gs[:, 2] - gs[:, 1] > 1e-3) & (rs[:, 2] - rs[:, 1] > 1e-3) & (np.abs(g.astype(np.float64) - r).min(axis=1) > 1e-3)
              & (np.abs(gs[:, 2] - rs[:, 2]) > 1e-3))
        got[todo[ok]], ref[todo[ok]] = g[ok], r[ok]
        todo = todo[~ok]
    return got, ref


def edge_set():
    """seven hand-made pixels: got == ref; a tied arg-max; got below and at the gamma step's clamp; a negative got; a zero label; all
    three channels tied.  Equal fp32 inputs stay equal through every step, so each tie resolves the same way in every precision."""
    got = np.array([[0.3, 0.5, 0.2], [0.6, 0.6, 0.1], [1e-12, 0.4, 0.7], [1e-10, 0.2, 0.9], [-0.25, 0.8, 0.3], [0.9, 0.05, 0.4],
                    [0.5, 0.5, 0.5]], dtype=np.float32)
    ref = np.array([[0.3, 0.5, 0.2], [0.2, 0.3, 0.9], [0.1, 0.2, 0.3], [0.5, 0.1, 0.3], [0.3, 0.3, 0.6], [0.0, 0.0, 0.0],
                    [0.25, 0.75, 0.5]], dtype=np.float32)
    return got, ref


def sum_depth(P, channels):
    blocks = min(-(-P // BLOCK), MAX_BLOCKS)
    passes = -(-P // (blocks * BLOCK))
    return channels * passes + 6 + 3 + 2


def _chain(x, G, tone_map, clamp):
    """(value, error bound, d value / d x, relative error bound of that derivative) per channel after the gamma step and the tone map"""
    x = x.astype(np.float64)
    if G == 1.0:
        a, ea, da, rda = x, np.zeros_like(x), np.ones_like(x), np.zeros_like(x)
    else:
        with np.errstate(invalid="ignore", divide="ignore"):
            xc = np.where(x < CLAMP, CLAMP, x) if clamp else x
            a = np.sqrt(xc) if G == 0.5 else np.power(xc, G)
            ea = (1 if G == 0.5 else 4) * U * np.abs(a)
            passes = (x >= CLAMP) if clamp else np.ones(x.shape, bool)
            da = np.where(passes, G * a / np.where(passes, x, 1.0), 0.0)
            rda = np.where(passes, ea / np.maximum(np.abs(a), 1e-300) + 2 * U, 0.0)
    if not tone_map:
        return a, ea, da, rda, np.ones_like(a), np.zeros_like(a)
    q = 1.0 + a
    b = a / q
    eb = ea / (q * q) + 3 * U * np.abs(b)
    dt = 1.0 / (q * q)
    rdt = 2 * (ea + U * np.abs(q)) / np.abs(q) + 2 * U   # q twice, its square, the quotient
    return b, eb, da, rda, dt, rdt


def _space(name, v, e):
    """(values [P,ch], error bounds [P,ch]) of a colour space of v +- e"""
    if name == "rgb":
        return v, e
    if name == "hsv":
        z = np.zeros((v.shape[0], 1))
        return np.concatenate([z, z, v.max(axis=1, keepdims=True)], axis=1), np.concatenate([z, z, e.max(axis=1, keepdims=True)], axis=1)
    if name == "luminance":
        return (v * LUM).sum(axis=1, keepdims=True), (e * LUM).sum(axis=1, keepdims=True) + 3 * U * (np.abs(v) * LUM).sum(axis=1, keepdims=True)
    val = v @ XYZ.T / XYZ_DIV
    return val, (e @ XYZ.T + 4 * U * (np.abs(v) @ XYZ.T)) / XYZ_DIV


def argmax_low(v):
    """torch.max's index: the lowest on a tie"""
    return np.argmax(v, axis=1)


def restate(got, ref, loss_fns, color_spaces, tone_map, gamma, g_up=1.0):
    """dict(loss, loss_bound, grad [P,3], grad_bound [P,3], stats[8]) in fp64 of fp32 inputs got, ref [P,3]"""
    P = got.shape[0]
    G = float(gamma)
    a, ea, da, rda, dta, rdta = _chain(got, G, tone_map, True)
    b, eb, *_ = _chain(ref, G, tone_map, False)
    L, S = len(loss_fns), len(color_spaces)
    w = g_up / (S * L)
    loss, loss_abs, loss_err = 0.0, 0.0, 0.0
    stats = np.zeros(8)
    gb = np.zeros((P, 3))     # d loss / d (the tone-mapped got), and its error bound, and the sum of the |terms| added into it
    egb = np.zeros((P, 3))
    sgb = np.zeros((P, 3))
    n_added = 0
    for name in color_spaces:
        ch = CHANNELS[name]
        n = float(P * ch)
        A, eA = _space(name, a, ea)
        B, eB = _space(name, b, eb)
        d = A - B
        ed = eA + eB + U * (np.abs(A) + np.abs(B))
        depth = sum_depth(P, 1 if name in ("hsv", "luminance") else 3)   # (hsv's two zero channels are not added)
        sq, ab = d * d, np.abs(d)
        mse, mae = sq.sum() / n, ab.sum() / n
        e_mse = ((2 * ab * ed + ed * ed + U * sq).sum() + depth * U * sq.sum()) / n
        e_mae = (ed.sum() + depth * U * ab.sum()) / n
        i = SPACES.index(name)
        stats[i], stats[4 + i] = mse, mae
        rmse = np.sqrt(max(mse, CLAMP))
        if mse + e_mse < CLAMP:
            e_rmse = U * rmse
        else:
            e_rmse = e_mse / (2 * rmse) + U * rmse
        k2, ek2, k1 = 0.0, 0.0, 0.0
        for fn in loss_fns:
            val, err = {"l2": (mse, e_mse), "l1": (mae, e_mae), "rmse": (rmse, e_rmse)}[fn]
            loss += val / (L * S)
            loss_abs += abs(val) / (L * S)
            loss_err += err / (L * S)
            if fn == "l2":
                k2 += 2.0 / n
                ek2 += 3 * U * 2.0 / n
            if fn == "l1":
                k1 += 1.0 / n
            if fn == "rmse" and mse >= CLAMP:
                k2 += 1.0 / (n * rmse)
                ek2 += (e_rmse / rmse + 4 * U) / (n * rmse)
                if mse - e_mse < CLAMP:   # an fp32 mean on the other side of the clamp: the whole term
                    ek2 += 1.0 / (n * rmse)
            elif fn == "rmse" and mse + e_mse >= CLAMP:
                ek2 += 1.0 / (n * np.sqrt(CLAMP))
        k2, ek2, k1 = w * k2, abs(w) * (ek2 + 2 * U * k2), w * k1
        # t = k2 d + k1 sign(d) per channel of the space
        t = k2 * d + k1 * np.sign(d)
        et = abs(k2) * ed + ek2 * ab + 2 * U * np.abs(k2 * d) + 3 * U * abs(k1) + U * np.abs(t)
        et = et + np.where(ed >= ab, 2 * abs(k1), 0.0) * (k1 != 0)   # a |d| inside its own error: sign(d) may differ
        if name == "rgb":
            terms, eterms = [t], [et]
        elif name == "hsv":
            k = argmax_low(a)
            onehot = np.eye(3)[k]
            terms, eterms = [onehot * t[:, 2:3]], [onehot * et[:, 2:3]]
            srt = np.sort(a, axis=1)
            near = (srt[:, 2] - srt[:, 1]) <= 2 * ea.max(axis=1)   # the two largest channels inside their errors: the term may move
            tied = srt[:, 2] == srt[:, 1]                              # (an exact tie resolves the same way everywhere)
            eterms[0] = eterms[0] + (near & ~tied)[:, None] * np.abs(t[:, 2:3])
        elif name == "luminance":
            terms, eterms = [t * LUM], [et * LUM + U * np.abs(t * LUM)]
        else:
            tq, etq = t / XYZ_DIV, et / XYZ_DIV + U * np.abs(t / XYZ_DIV)
            terms = [tq[:, j:j + 1] * XYZ[j] for j in range(3)]
            eterms = [etq[:, j:j + 1] * XYZ[j] + U * np.abs(terms[j]) for j in range(3)]
        for term, eterm in zip(terms, eterms):
            gb += term
            egb += eterm
            sgb += np.abs(term)
            n_added += 1
    egb = egb + n_added * U * sgb
    # g_got = (gb dt) da with dt = 1 / (1 + a)^2 and da = G a / x
    v, ev = gb * dta, egb * dta + np.abs(gb * dta) * (rdta + U)
    grad = v * da
    grad_bound = ev * np.abs(da) + np.abs(grad) * (rda + U)
    grad_bound = np.where(da == 0.0, 0.0, grad_bound)   # exactly 0 below the clamp
    loss_bound = loss_err + 4 * U * loss_abs
    return dict(loss=loss, loss_bound=2 * loss_bound, grad=grad, grad_bound=2 * grad_bound, stats=stats)
