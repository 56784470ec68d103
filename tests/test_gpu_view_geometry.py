"""The View MLP's geometry operand of the f16x layer-synchronous renderer (csrc/ls_sched_plain.inc, MODEL 0 and 6): ONE wave of a
sample group builds a block's [x, y, z, elev, azim] B fragment and parks it in LDS (raw for view.init, through the sine for
view.L0), the four row-group waves read it back.  The shapes are the ones at which a parked fragment can go wrong: a ragged
second block (clamped step index), blocks of two rays in one pass (the per-block ray constants differ), sample groups without a
valid ray, the mip schedule (the geometry pair runs behind the IPE groups, in a phase of its own), explicit sample positions.

Every case: f16x against the CPU oracle at the renderer tests' bar (1e-4 L-inf on colour, alpha and weights:
test_gpu_render_ls.py), f16x against bf16x3 on the same engine -- whose waves still build the fragment in registers -- and two
consecutive calls bit for bit.  The cross-precision bound is the triangle of the two 1e-4 bars, 2e-4.  The mip renderer exists
in f16x only (the library refuses every other precision), so that case has no bf16x3 leg."""
import math

import pytest
import torch

import oracle as O
from conftest import load_golden, golden_params

pytestmark = pytest.mark.gpu
BAR = 1e-4
SIZE = 800
FOCAL = 0.5 * SIZE / math.tan(0.5 * 0.6911)
C2W = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]])


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def plain():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops
    from test_gpu_render_ls import pack_ls
    p = golden_params(load_golden("g11_plain_view_b1"))
    packed = {prec: pack_ls(ops, p, prec) for prec in ("f16x", "bf16x3")}
    return ops, p, packed


def _rays(crop):
    return O.nerf_camera_rays(O.pixel_grid(SIZE, crop), C2W, FOCAL, SIZE)


def _check(run, ref, aux):
    """run(prec) -> (out, alpha, weights) on the GPU"""
    x = run("f16x")
    for got, want in zip(x, (ref, aux["alpha"], aux["weights"])):
        err = float((got.cpu() - want).abs().max())
        print(f"f16x vs oracle {err:.3e}")
        assert err <= BAR
    again = run("f16x")
    assert all(torch.equal(a, b) for a, b in zip(x, again))
    y = run("bf16x3")
    for a, b in zip(x, y):
        err = float((a - b).abs().max())
        print(f"f16x vs bf16x3 {err:.3e}")
        assert err <= 2 * BAR


# T = 33: the second block holds ONE step, the other 31 lanes read the clamped step | T = 96, 5 rays: three blocks per ray against two
# per pass, so a ray's last block shares its pass with a block of another ray index (here the clamped one past the batch) | 3 rays:
# two workgroups = four sample groups, one of them without a valid ray | T = 96, 520 rays: more rays than the 512 sample groups of a
# full grid, so the groups 0..7 carry a second REAL ray whose first block shares a pass with the first ray's last
@pytest.mark.parametrize("T,crop", [(33, (380, 390, 3, 3)), (96, (400, 398, 1, 5)), (64, (10, 20, 1, 3)), (96, (380, 390, 20, 26))])
def test_parked_geometry_fragment_vs_oracle_and_bf16x3(plain, T, crop):
    ops, p, packed = plain
    rays = _rays(crop)
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    aux = {}
    ref = O.plain_nerf(p, rays, 2.0, 6.0, T, "view", act="upshifted", bg="white", aux=aux)
    rg = rays.cuda()
    _check(lambda prec: ops.render_plain_view_ls(rg, ts, packed[prec][1], packed[prec][0], prec, "upshifted", "white", want_weights=True),
           ref, aux)


def test_parked_geometry_fragment_explicit_points(plain):
    """T = 32, positions handed in (the D-NeRF canonical half): the builder wave reads them where the four waves did"""
    ops, p, packed = plain
    T = 32
    rays = load_golden("g11_plain_view_b1")["rays"]
    r_o, r_d = rays.split([3, 3], dim=-1)
    ts_c, _ = O.compute_ts(2.0, 6.0, T)
    g = torch.Generator().manual_seed(7)
    pts = O.compute_pts(r_o, r_d, ts_c) + 0.05 * torch.randn(T, *rays.shape[:-1], 3, generator=g)
    aux = {}
    ref = O.plain_nerf_from_pts(p, pts, ts_c, r_o, r_d, "view", act="upshifted", aux=aux)
    rg, tg, pg = rays.cuda(), ts_c.cuda(), pts.cuda()
    _check(lambda prec: ops.render_plain_view_ls(rg, tg, packed[prec][1], packed[prec][0], prec, "upshifted", "black", want_weights=True, pts=pg),
           ref, aux)


def test_parked_geometry_fragment_mip():
    """MODEL 6 at T = 64 with 4 rays (a 2 x 2 crop: the pixel radius needs two rows): f16x only"""
    import nerf_atlas_amd.nerf as nerf
    from nerf_atlas_amd import ops
    from nerf_atlas_amd.utils import ConicGaussian
    from oracle.procedural import proc_param
    m = nerf.PlainNeRF(steps=16, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted", mip=ConicGaussian()).cuda().eval()
    params = {}
    for k, v in m.state_dict().items():
        if k.endswith("primes") or v.numel() == 0:
            continue
        params[k] = torch.from_numpy(proc_param(k, tuple(v.shape)))
        v.copy_(params[k])
    T = 64
    rays = _rays((397, 1, 2, 2))
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    packed, tables, rg = m.packed_mip_ls("f16x"), m.first.enc.tables(), rays.cuda()
    run = lambda: ops.render_plain_mip_ls(rg, ts, tables, packed, "f16x", "cone", float("nan"), 0, 16, "upshifted", "white", want_weights=True)
    aux = {}
    ref = O.plain_nerf(params, rays, 2.0, 6.0, T, "view", act="upshifted", bg="white", mip="cone", aux=aux)
    x = run()
    for got, want in zip(x, (ref, aux["alpha"], aux["weights"])):
        err = float((got.cpu() - want).abs().max())
        print(f"mip f16x vs oracle {err:.3e}")
        assert err <= BAR
    assert all(torch.equal(a, b) for a, b in zip(x, run()))
