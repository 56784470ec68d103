"""The fp64 reference of the hash-table scatter (tests/scatter_ref.py) against autograd of the oracle, and an fp32 / fixed-point
EMULATION of the scatter against the per-entry bound on the inputs the GPU tests use: the reference and the bound stand on
their own before a kernel is measured with them (tests/test_gpu_scatter.py).  No GPU."""
import pytest
import torch

import oracle as O
import scatter_ref as S
from oracle.procedural import proc_uniform


def _small():
    x = torch.from_numpy(proc_uniform((97, 3), 3001, 3.0))
    x[:5] = torch.tensor([[0.0, 0.0, 0.0], [-0.0625, 0.125, 1.0], [2.999, -2.999, 0.5], [-1e-6, 1e-6, 0.0], [0.03125, -0.03125, 3.0]])
    g = torch.from_numpy(proc_uniform((97, 32), 3002, 1.0))
    return x, g


def test_reference_equals_fp64_autograd_of_the_oracle():
    """oracle.hash_encode with fp32 positions and fp64 tables: the same cells as the reference (v = x * N_l in fp32), the corner
    weights in fp32 -- three roundings (1 - w, two products) -- everything else in fp64.  So |autograd - ref| <= ((1+u)^3 - 1) mag
    < 4 u mag per entry; a wrong index, corner order or weight is off by O(mag)."""
    x, g = _small()
    ref, mag, cnt = S.scatter_ref(x, g)
    tabs = [torch.zeros(65536, 4, dtype=torch.float64, requires_grad=True) for _ in range(8)]
    (O.hash_encode(x, tabs, include_input=False) * g.double()).sum().backward()
    auto = torch.stack([t.grad for t in tabs])
    assert float(auto.abs().max()) > 0.1
    assert bool(((auto - ref).abs() <= 4 * S.U * mag).all())
    # counts: 8 corners per sample and level, the same in the four columns; untouched rows are exactly zero
    assert torch.equal(cnt.sum(dim=1), torch.full((8, 4), 8.0 * x.shape[0], dtype=torch.float64))
    assert bool((ref[cnt == 0] == 0).all()) and bool((mag[cnt == 0] == 0).all()) and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    idx = O.hash_corner_indices(x)
    assert torch.equal(cnt[3, :, 0], torch.bincount(idx[3].reshape(-1), minlength=65536).double())


def test_tangent_reference_equals_fp64_autograd_of_the_directional_derivative():
    """d <g, J(x) e> / d tables through torch's fp64 double-backward of oracle.hash_encode.  There v = x * N_l is fp64: the cells are
    asserted to be the same, the fractional parts then differ by at most 2 u |v| (the rounding of the fp32 product and of N_l's
    cast), and the corner weight N_l <grad w_c, e> moves by at most 2 * that * N_l |e|_1.  Level 0 on dyadic points (v exact
    both ways) must agree to fp64 roundoff."""
    x, g = _small()
    e = torch.from_numpy(proc_uniform((97, 3), 3003, 1.0))
    x[5:40] = torch.round(x[5:40] * 64) / 64
    ref, mag, cnt = S.scatter_ref(x, g, e)
    res = O.hash_resolutions(8)
    for l in range(8):
        assert torch.equal((x.double() * res[l]).floor(), (x * res[l]).floor().double())
    tabs = [torch.zeros(65536, 4, dtype=torch.float64, requires_grad=True) for _ in range(8)]
    xd = x.double().requires_grad_()
    _, jv = torch.autograd.functional.jvp(lambda p: O.hash_encode(p, tabs, include_input=False), xd, e.double(), create_graph=True)
    (jv * g.double()).sum().backward()
    auto = torch.stack([t.grad for t in tabs])
    assert float(auto.abs().max()) > 1.0
    vmax, e1, gmax = 3.0 * 16.0, float(e.abs().sum(dim=1).max()), float(g.abs().max())
    for l in range(8):
        tol = cnt[l] * gmax * res[l] * e1 * 2 * (2 * S.U * vmax) + 1e-12 * mag[l]
        assert bool(((auto[l] - ref[l]).abs() <= tol).all()), l
    # dyadic points only, level 0: nothing is rounded before fp64
    ref0, mag0, _ = S.scatter_ref(x[5:40], g[5:40], e[5:40])
    tabs = [torch.zeros(65536, 4, dtype=torch.float64, requires_grad=True) for _ in range(8)]
    _, jv = torch.autograd.functional.jvp(lambda p: O.hash_encode(p, tabs, include_input=False), x[5:40].double().requires_grad_(),
                                          e[5:40].double(), create_graph=True)
    (jv * g[5:40].double()).sum().backward()
    assert bool(((tabs[0].grad - ref0[0]).abs() <= 1e-12 * mag0[0]).all())


def emulate(x, g, tangent, det, seed):
    """the scatter the way an fp32 kernel computes it: every addend in fp32 with the kernel's operation order, summed by index_add_
    in a permuted order (fp32), or rounded to 2^-40 fixed point, summed as int64 and folded to fp32 with one rounding"""
    N = x.shape[0]
    idx = O.hash_corner_indices(x)
    res = O.hash_resolutions(8)
    perm = torch.from_numpy(S._order(N, seed))
    out = torch.zeros(8, 65536, 4, dtype=torch.float32)
    for l in range(8):
        nl = torch.tensor(res[l], dtype=torch.float32)
        v = x * nl
        w = v - v.floor()
        iw = 1.0 - w
        e = None if tangent is None else tangent * nl
        gl = g[:, 4 * l:4 * l + 4]
        fix = torch.zeros(65536, 4, dtype=torch.int64)
        for c in range(8):
            b = S._corner_bits(c)
            ux, uy, uz = (w[:, a] if b[a] else iw[:, a] for a in range(3))
            if e is None:
                wt = ux * uy * uz
            else:
                sx, sy, sz = (e[:, a] if b[a] else -e[:, a] for a in range(3))
                wt = (sx * (uy * uz) + sy * (ux * uz)) + sz * (ux * uy)
            a = (wt[:, None] * gl)[perm]
            assert a.dtype == torch.float32
            if det:
                fix.index_add_(0, idx[l, c][perm], torch.round(a.double() * 2.0 ** 40).long())
            else:
                out[l].index_add_(0, idx[l, c][perm], a)
        if det:
            out[l] = (fix.double() * 2.0 ** -40).float()
    return out


@pytest.mark.parametrize("name", S.CASES)
def test_fp32_emulation_of_the_scatter_stays_inside_the_bound(name):
    """the bound of scatter_ref.bound is not something only an exact computation meets: a plain fp32 scatter in an arbitrary order,
    and one through 2^-40 fixed point, stay inside it on every input of the GPU tests (and are exact on level 0 of input G)"""
    x, g, t = S.case(name)
    for tan in (False, True):
        ref, mag, cnt = S.reference(name, tan)
        for det in (False, True):
            got = emulate(x, g, t if tan else None, det, 3200 + int(det))
            r = S.worst_ratio(got, ref, mag, cnt, det, tan)
            print(f"\n[emulation {name} tangent={int(tan)} det={int(det)}] worst error / bound {r:.3f}")
            assert r <= 1.0, (name, tan, det, r)
            if name == "G":
                assert torch.equal(got[0], ref[0].float()), (tan, det)


def test_inputs_reach_the_paths_they_are_aimed_at():
    """CPU-side facts about the inputs: E has LDS tag conflicts inside its one round, the rows A / B / C aim at keep k (k + 8) u << 1
    (a dropped addend stays visible), C has more than four cells per wave, F gives workgroup 256 exactly one sample"""
    assert S.tag_conflicts(S.case("E")[0]) >= 1
    print(f"\n[input E] {S.tag_conflicts(S.case('E')[0])} conflicting (level, LDS row) slots")
    for name in ("A", "B", "C"):
        k = float(S.reference(name, False)[2].max())
        assert k * (k + 8) * S.U < 0.01, (name, k)
    idx0 = O.hash_corner_indices(S.case("C")[0])[0, 0]
    assert all(len(torch.unique(idx0[w:w + 64])) > 4 for w in range(0, 192, 64))
    per = ((S.F_N + 511) // 512 + 255) // 256 * 256
    assert per == 512 and S.F_N - 256 * per == 1
    x, g = S.limits_input()
    ref, _, _ = S.scatter_ref(x, g)
    row = int(O.hash_corner_indices(x[:1])[0, 0, 0])
    # what reaches the threshold is a wave's merged sum over its lanes on the row (corner 0 has weight 1 on a vertex, the others 0)
    idx0 = O.hash_corner_indices(x)[0, 0]
    merged = torch.stack([g[w:w + 64, 0:4][idx0[w:w + 64] == row].double().sum(dim=0) for w in range(0, x.shape[0], 64)])
    below = float(torch.nextafter(torch.tensor(2.0 ** 20, dtype=torch.float32), torch.tensor(0.0)))
    assert merged[0].tolist() == [2.0 ** 20, 2.0 ** 22, below, 2.0 ** 19]      # exactly 2^20 and 2^22: bypass; just below: accumulator
    assert bool((merged[1:, 0:3].abs() < 1024).all()) and float(merged[1:, 0:3].abs().sum(dim=0).min()) > 0   # small integers, fixed point
    assert merged[:, 3].tolist() == [2.0 ** 19] * 12 + [0.0] * 4 and bool((merged.abs() < 2.0 ** 20).all(dim=1)[1:].all())
    assert all(int((idx0[w:w + 64] == row).sum()) > 1 for w in (64, 128, 192))   # waves of workgroup 0 share its LDS row
    assert float(ref[0, row, 3]) == 6291456.0 and float(ref[0, row, 0]) != 2.0 ** 20 and float(ref[0, row, 1]) != 2.0 ** 22
    assert float(ref[0, row, 2]) < 2.0 ** 20 and torch.equal(ref[0].float().double(), ref[0])   # every level-0 total is an fp32 number
