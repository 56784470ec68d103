"""Plain fp64 restatement of the Fourier encoder's position gradient (csrc/fourier_grad.hip; src/utils.py:14-17 under autograd), the
ruler the tests normalise errors by, and the cases of tests/golden/g22_fourier_grad.npz.  Imported by tests/test_fourier_grad.py (CPU)
and tests/test_gpu_fourier_grad.py.

    enc(x) = [sin(x be) | cos(x be)],  be = scale * basis [D, F]
    gx[n, d] = sum_f be[d, f] (cos(m[n, f]) g_sin[n, f] - sin(m[n, f]) g_cos[n, f]),  m = x be

THE RULER.  An error of the argument m (its fp32 rounding: |m| reaches 10^2 - 10^3, half an ulp is 1.5e-5 - 3e-5) moves sin / cos by as
much, and term f of entry (n, d) by |be[d, f]| (|g_sin| + |g_cos|) times that.  So errors are measured per entry in units of

    ruler[n, d] = sum_f |be[d, f]| (|g_sin[n, f]| + |g_cos[n, f]|)

and `ref32_dev(case)` is the largest such ratio of the REFERENCE's own fp32 autograd against its fp64 autograd (both recorded by
tools/gen_golden.py g22): what fp32 arithmetic costs on this operator, whoever computes it.
"""
import functools
import itertools

import numpy as np

from conftest import load_golden

FS, DS, SCALES, SIGMAS = (128, 4, 6), (1, 2, 3), (1.0, 1.5), (16, 32)
CASES = list(itertools.product(FS, DS, SCALES, SIGMAS))


def tag(F, D, scale, sigma):
    return f"F{F}_D{D}_s{scale}_sig{sigma}"


@functools.lru_cache(maxsize=None)
def fixture():
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in load_golden("g22_fourier_grad").items()}


def case_inputs(F, D, scale, sigma):
    """(x [257, D], basis [D, F], g [257, 2F]) fp32, as the reference saw them"""
    h = fixture()
    return h[f"x{D}"], h[f"basis_{sigma}_{D}_{F}"], h[f"g{F}"]


def gx_ref(x, basis, scale, g):
    """fp64 gx [N, D] from fp32 or fp64 inputs (the reference's fp64 run: every input cast to double first)"""
    x, be, g = np.asarray(x, np.float64), scale * np.asarray(basis, np.float64), np.asarray(g, np.float64)
    F = be.shape[1]
    m = x @ be
    return (np.cos(m) * g[:, :F] - np.sin(m) * g[:, F:]) @ be.T


def ruler(basis, scale, g):
    be, g = np.abs(scale * np.asarray(basis, np.float64)), np.abs(np.asarray(g, np.float64))
    F = be.shape[1]
    return (g[:, :F] + g[:, F:]) @ be.T


@functools.lru_cache(maxsize=None)
def ref32_dev(F, D, scale, sigma):
    """largest |gx32 - gx_ref| / ruler over the 257 x D entries of a case: the reference's fp32 autograd against fp64"""
    h = fixture()
    x, basis, g = case_inputs(F, D, scale, sigma)
    return float((np.abs(h["gx32." + tag(F, D, scale, sigma)].astype(np.float64) - gx_ref(x, basis, scale, g)) / ruler(basis, scale, g)).max())
