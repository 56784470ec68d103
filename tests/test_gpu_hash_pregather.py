"""The [hash | x] group of the f16x headline renderer (csrc/ls_sched_plain.inc MODEL 0, csrc/ls_kernel.h `pregather`): the shadow wave
of a block encodes the block's samples of pass p + 1 during view.out of pass p -- positions from the NEXT pass's ray and steps, the
conversion into an LDS region the owner wave still reads two things from (the density, the compositing partials), the raw values
carried in registers across the barrier into their stash.  The shapes are the ones at which that can go wrong: a single block, a
ragged second block of the last pass, a pass whose two blocks belong to two rays, sample groups without a ray, more rays than
sample groups (the encode for pass p + 1 uses another ray's origin and direction than pass p), two rays in every pass, per-ray steps,
a row band rendered alone, both backgrounds, a saturating hash feature (the conversion that raises the flag runs in another wave and
phase now) and the mip schedule, which shares the schedule file and keeps the encoder in its exposed phase.

Bars (tests/test_gpu_view_geometry.py): f16x against the CPU oracle 1e-4 L-inf on colour, alpha and weights; f16x against bf16x3 --
whose waves encode in the exposed phase -- the triangle of the two bars, 2e-4; the same launch twice bit for bit."""
import math

import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu
BAR = 1e-4
SIZE = 800
FOCAL = 0.5 * SIZE / math.tan(0.5 * 0.6911)
C2W = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]])
ACT = "upshifted"


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def plain():
    """a 64-wide PlainNeRF(view), seed 2: the model, its parameters for the oracle, its streams in both parity modes"""
    assert torch.cuda.is_available()
    import nerf_atlas_amd.nerf as nerf
    from nerf_atlas_amd import ops
    from test_gpu_render_ls import pack_ls
    torch.manual_seed(2)
    m = nerf.PlainNeRF(steps=32, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind=ACT).cuda().eval()
    p = {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if not k.endswith("primes") and v.numel() > 0}
    packed = {prec: pack_ls(ops, p, prec) for prec in ("f16x", "bf16x3")}
    return ops, p, packed, m


def _rays(crop):
    return O.nerf_camera_rays(O.pixel_grid(SIZE, crop), C2W, FOCAL, SIZE)


def _crop(n):
    """n rays of the frame's centre rows"""
    if n <= 800:
        return (400, 398 if n <= 5 else 0, 1, n)
    assert n % 2 == 0
    return (399, 0, 2, n // 2)


def _check(run, ref, aux):
    """run(prec) -> (out, alpha, weights) on the GPU"""
    x = run("f16x")
    for name, got, want in zip(("out", "alpha", "weights"), x, (ref, aux["alpha"], aux["weights"])):
        err = float((got.cpu() - want).abs().max())
        print(f"f16x vs oracle [{name}] {err:.3e}")
        assert err <= BAR, (name, err)
    again = run("f16x")
    assert all(torch.equal(a, b) for a, b in zip(x, again))
    y = run("bf16x3")
    for name, a, b in zip(("out", "alpha", "weights"), x, y):
        err = float((a - b).abs().max())
        print(f"f16x vs bf16x3 [{name}] {err:.3e}")
        assert err <= 2 * BAR, (name, err)


def _shared_steps(plain, n, T, bg):
    ops, p, packed, _ = plain
    rays = _rays(_crop(n))
    assert rays.numel() // 6 == n
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    aux = {}
    ref = O.plain_nerf(p, rays, 2.0, 6.0, T, "view", act=ACT, bg=bg, aux=aux)
    rg = rays.cuda()
    _check(lambda prec: ops.render_plain_view_ls(rg, ts, packed[prec][1], packed[prec][0], prec, ACT, bg, want_weights=True), ref, aux)


# 32 steps: one block per ray | 64: one pass per ray | 96: three blocks per ray against two per pass, so every second pass holds the
# blocks of two rays | 128: two passes per ray.  1 .. 5 rays: two workgroups = four sample groups, some without a ray; with 5 rays
# group 0 carries a second ray, and behind the last ray's last block the next pass has no block to encode.
@pytest.mark.parametrize("bg", ["white", "black"])
@pytest.mark.parametrize("T", [32, 64, 96, 128])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_few_rays(plain, n, T, bg):
    _shared_steps(plain, n, T, bg)


# 520 rays x 64 steps: a full grid has 512 sample groups, so eight of them go on from one ray to the next -- the encode under the
# first ray's view.out takes the second ray's origin and direction | 1030 rays x 32 steps: every pass holds two rays
@pytest.mark.parametrize("n,T,bg", [(520, 64, "white"), (520, 64, "black"), (1030, 32, "white")])
def test_more_rays_than_sample_groups(plain, n, T, bg):
    _shared_steps(plain, n, T, bg)


@pytest.mark.parametrize("n", [5, 520])
def test_per_ray_steps_coarse_fine(plain, n):
    """forward_coarse_fine with 32 + 32 steps: the fine pass reads its steps per ray (na_render_plain_view_ls_rayts), through the
    same ts_load as the shared steps.  Both parity modes render the fine pass on the f16x run's steps."""
    from nerf_atlas_amd import config
    ops, p, packed, m = plain
    rays = _rays(_crop(n))
    rg = rays.cuda()
    config.set_precision("f16x")
    try:
        out = m.forward_coarse_fine(rg, 32)
        ts_ray = m.ts_ray.clone()
        assert ts_ray.shape == tuple(rays.shape[:-1]) + (64,)
        assert torch.equal(out, m.forward_coarse_fine(rg, 32)) and torch.equal(ts_ray, m.ts_ray)
    finally:
        config.set_precision("bf16x3")
    bg = m._kernel_bg()
    aux = {}
    ref = O.plain_nerf_rayts(p, rays, ts_ray.cpu().movedim(-1, 0).contiguous(), "view", act=ACT, bg=bg, aux=aux)
    err = float((out.cpu() - ref).abs().max())
    print(f"forward_coarse_fine f16x vs oracle on its own steps {err:.3e}")
    assert err <= BAR
    _check(lambda prec: ops.render_plain_view_ls_rayts(rg, ts_ray, packed[prec][1], packed[prec][0], prec, ACT, bg, want_weights=True),
           ref, aux)


def test_band_alone_equals_the_rows_of_the_full_render(plain):
    """40 x 40 rays, rows 10..19: what the shadow encodes for the band's first pass does not depend on what came before the band"""
    ops, _, packed, _ = plain
    ts, _ = ops.compute_ts(2.0, 6.0, 64, "cuda")
    tables, stream = packed["f16x"][1], packed["f16x"][0]
    run = lambda crop: ops.render_plain_view_ls(_rays(crop).cuda(), ts, tables, stream, "f16x", ACT, "white", want_weights=True)
    full = run((380, 380, 40, 40))
    band = run((390, 380, 10, 40))
    assert torch.equal(band[0], full[0][:, 10:20])                    # colour [1, rows, cols, 3]
    assert torch.equal(band[1], full[1][:, :, 10:20]) and torch.equal(band[2], full[2][:, :, 10:20])  # alpha, weights [T, 1, rows, cols]


def test_a_saturating_hash_feature_is_still_loud(plain):
    """tables scaled until the encoder's features leave the half range: the frame must be the NaN one (tests/test_gpu_range.py),
    and the next launch with the model's own tables is clean"""
    ops, p, packed, _ = plain
    from test_gpu_render_ls import pack_ls
    bad = {k: v.clone() for k, v in p.items()}
    for i in range(8):
        w = bad[f"first.enc.embs.{i}.weight"]
        bad[f"first.enc.embs.{i}.weight"] = w * (1e7 / float(w.abs().mean()))
    assert all(bool(torch.isfinite(bad[f"first.enc.embs.{i}.weight"]).all()) for i in range(8))
    stream, tables = pack_ls(ops, bad, "f16x")
    rays = _rays(_crop(5)).cuda()
    ts, _ = ops.compute_ts(2.0, 6.0, 96, "cuda")
    out, _, _ = ops.render_plain_view_ls(rays, ts, tables, stream, "f16x", ACT, "black", want_weights=False)
    assert torch.isnan(out).all()
    good, _, _ = ops.render_plain_view_ls(rays, ts, packed["f16x"][1], packed["f16x"][0], "f16x", ACT, "black", want_weights=False)
    assert torch.isfinite(good).all()


def test_mip_schedule_still_encodes_in_its_exposed_phase():
    """MODEL 6 includes the same schedule file and keeps hash_group_ep: 5 rays (a 5 x 1 crop: the pixel radius needs two rows) x 64
    steps against the oracle, f16x only (the library has no other mip renderer)"""
    import nerf_atlas_amd.nerf as nerf
    from nerf_atlas_amd import ops
    from nerf_atlas_amd.utils import ConicGaussian
    from oracle.procedural import proc_param
    m = nerf.PlainNeRF(steps=16, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind=ACT, mip=ConicGaussian()).cuda().eval()
    params = {}
    for k, v in m.state_dict().items():
        if k.endswith("primes") or v.numel() == 0:
            continue
        params[k] = torch.from_numpy(proc_param(k, tuple(v.shape)))
        v.copy_(params[k])
    T = 64
    rays = _rays((397, 1, 5, 1))
    ts, _ = ops.compute_ts(2.0, 6.0, T, "cuda")
    packed, tables, rg = m.packed_mip_ls("f16x"), m.first.enc.tables(), rays.cuda()
    run = lambda: ops.render_plain_mip_ls(rg, ts, tables, packed, "f16x", "cone", float("nan"), 0, 16, ACT, "white", want_weights=True)
    aux = {}
    ref = O.plain_nerf(params, rays, 2.0, 6.0, T, "view", act=ACT, bg="white", mip="cone", aux=aux)
    x = run()
    for got, want in zip(x, (ref, aux["alpha"], aux["weights"])):
        err = float((got.cpu() - want).abs().max())
        print(f"mip f16x vs oracle {err:.3e}")
        assert err <= BAR
    assert all(torch.equal(a, b) for a, b in zip(x, run()))
