"""tests/voxel_sh_ref.py, the fp64 restatement the GPU tests of the per-voxel spherical-harmonic colour head compare against, checked on
the CPU: against torch fp64 autograd of a naive `gather rows -> basis -> sum` (outputs, both grids' gradients, the position gradient),
its scatter as the transpose of its gather, and order 0 as Y_0 times the RGB head's lookup."""
import pytest
import torch

import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H


def naive(pts, dirs, den, rgb, order, xyz=None):
    """raw [N,4] fp64 by gathering the 8 rows, expanding every coefficient and summing: no shared code with sample_ref behind the cells"""
    S = den.shape[0]
    ids, x32 = V.cells(pts, S)
    x = x32.double() if xyz is None else xyz
    rows = V.rows_of(ids, S)
    Y = P.basis(dirs, order)[0][torch.arange(pts.shape[0]) % dirs.shape[0]]
    pick = lambda v, pos: v if pos else 1 - v
    w = torch.stack([pick(x[:, 0], V.bit_i(u, 0)) * pick(x[:, 1], V.bit_i(u, 1)) * pick(x[:, 2], V.bit_i(u, 2)) for u in range(8)], dim=-1)
    d = (w * den.reshape(S ** 3)[rows]).sum(-1)
    out = [d]
    NK = H.nk(order)
    flat = rgb.reshape(S ** 3, 3 * NK)
    for c in range(3):
        coeff = (w[..., None] * flat[rows][..., c * NK:(c + 1) * NK]).sum(1)   # the interpolated coefficients [N,NK]
        out.append((coeff * Y).sum(-1))
    return torch.stack(out, dim=-1)


@pytest.mark.parametrize("order", H.ORDERS)
@pytest.mark.parametrize("S", (2, 4, 16))
def test_restatement_equals_fp64_autograd_of_the_naive_lookup(S, order):
    N, R = 65, 13
    den, rgb = H.grid_values(S, order)
    dirs = H.directions(R)
    pts = V.uniform_points(N)
    g = H.grads(N).double()
    dd, rr = den.double().requires_grad_(True), rgb.double().requires_grad_(True)
    xyz = V.cells(pts, S)[1].double().requires_grad_(True)
    raw = naive(pts, dirs, dd, rr, order, xyz)
    ref, mag = H.sample_ref(pts, dirs, den, rgb, order)
    scale = float(mag.max())
    assert float((raw.detach() - ref).abs().max()) <= 1e-12 * scale
    (raw * g).sum().backward()
    sref, smag, _ = H.scatter_ref(pts, dirs, g.float(), S, order)
    got = torch.cat([dd.grad.reshape(S ** 3, 1), rr.grad.reshape(S ** 3, -1)], dim=-1)
    assert float((got - sref).abs().max()) <= 1e-12 * max(float(smag.max()), 1.0)
    pref, _ = H.pts_grad_ref(pts, dirs, den, rgb, g.float(), order)
    assert float((xyz.grad / (V.GRID_RADIUS * 2 / S) - pref).abs().max()) <= 1e-9 * float(pref.abs().max())


@pytest.mark.parametrize("order", (0, 2, 4))
def test_scatter_is_the_transpose_of_the_gather(order):
    S, N, R = 4, 63, 9
    den, rgb = H.grid_values(S, order)
    dirs, pts, g = H.directions(R), V.uniform_points(N), H.grads(N)
    raw, _ = H.sample_ref(pts, dirs, den, rgb, order)
    sref, _, _ = H.scatter_ref(pts, dirs, g, S, order)
    grid = torch.cat([den.double().reshape(S ** 3, 1), rgb.double().reshape(S ** 3, -1)], dim=-1)
    lhs, rhs = float((raw * g.double()).sum()), float((sref * grid).sum())
    assert abs(lhs - rhs) <= 1e-11 * max(abs(lhs), 1.0)


def test_order_0_is_y0_times_the_rgb_heads_lookup():
    S, N = 16, 257
    den, rgb = H.grid_values(S, 0)
    pts = V.uniform_points(N)
    raw, mag = H.sample_ref(pts, H.directions(1), den, rgb, 0)
    lead, _ = V.sample_ref(pts, den, rgb)
    y0 = float(P.basis(torch.tensor([[0.0, 0.0, 1.0]]), 0)[0][0, 0])
    assert torch.equal(raw[:, 0], lead[:, 0])
    assert float((raw[:, 1:] - y0 * lead[:, 1:]).abs().max()) <= 1e-14 * float(mag.max())   # (fp64 roundings of extrapolated sums)


def test_special_directions_sit_on_the_cancellation_cones():
    d = H.directions(7).double()
    n = d / d.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    assert float(d[0].abs().max()) == 0.0
    assert abs(float(n[2, 0] ** 2 - n[2, 1] ** 2)) <= 1e-7
    z = float(n[3, 2])
    assert abs(35 * z ** 4 - 30 * z ** 2 + 3) <= 1e-5
    Y, Ya = P.basis(H.directions(7), 4)
    assert float(Y[3, 20].abs()) <= 1e-5 * float(Ya[3, 20]) and float(Y[2, 8].abs()) <= 1e-6 * float(Ya[2, 8])
