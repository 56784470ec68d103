"""SSIM / MS-SSIM on the GPU (csrc/ssim.hip) against tests/ssim_ref.py and its derived bounds: na_ssim forward and backward at the shapes
where the tiling can go wrong (the kernel's tile is 16 x 16: one map pixel, a single row of pixels, exactly one tile, a tile plus one in
each axis, N = 3, C = 1 / 3 / 4), the exact cases, NaN containment, reproducibility, the return codes, na_image_halve, ops.ms_ssim,
--loss-fns ssim through autograd and one short run of the runner with --msssim-loss."""
import ctypes as C

import numpy as np
import pytest
import torch

import ssim_ref as R

pytestmark = pytest.mark.gpu

NA_OK, NA_ENULL, NA_EUNSUPPORTED, NA_EWORKSPACE = 0, -2, -3, -5   # include/nerf_atlas_amd.h
C1, C2 = 1e-4, 9e-4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


def gpu_pair(case):
    x, y = R.image_pair(*case)
    return x.cuda(), y.cuda()


@pytest.mark.parametrize("case", R.SSIM_CASES)
def test_ssim_forward_within_the_bounds(ops, case):
    s_ref, cs_ref, bs, bc = R.ssim_reference(case)
    s, cs = ops.ssim(*gpu_pair(case))
    assert tuple(s.shape) == (case[0], case[3]) and s.dtype == torch.float32
    rs, rc = R.worst_ratio(s, s_ref, bs), R.worst_ratio(cs, cs_ref, bc)
    print(f"{case}: ssim err {float((s.cpu().double() - s_ref).abs().max()):.2e} (bound {float(bs.max()):.2e}, ratio {rs:.3f}); "
          f"cs err {float((cs.cpu().double() - cs_ref).abs().max()):.2e} (bound {float(bc.max()):.2e}, ratio {rc:.3f})")
    assert rs <= 1 and rc <= 1


@pytest.mark.parametrize("case", R.SSIM_CASES)
def test_ssim_backward_within_the_bounds(ops, case):
    g_ref, bound = R.grad_reference(case)
    x, y = gpu_pair(case)
    g_x = ops.ssim_backward(x, y, R.upstream(case[0], case[3]).cuda())
    assert g_x.shape == x.shape
    ratio = R.worst_ratio(g_x, g_ref, bound)
    # the border of g_x is under fewer windows (the corner pixel under one): checked on its own, and it must not be empty
    edge = torch.zeros(g_ref.shape[1:3], dtype=torch.bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    r_edge = R.worst_ratio(g_x.cpu()[:, edge], g_ref[:, edge], bound[:, edge])
    print(f"{case}: g_x err {float((g_x.cpu().double() - g_ref).abs().max()):.2e} of {float(g_ref.abs().max()):.2e} "
          f"(ratio {ratio:.3f}, border {r_edge:.3f})")
    assert ratio <= 1 and r_edge <= 1
    assert int((g_x.cpu()[:, edge] != 0).sum()) > 0 and float(g_ref[:, -1, -1].abs().max()) > 0


def test_exact_cases(ops):
    x, _ = gpu_pair((3, 18, 18, 3))
    s, cs = ops.ssim(x, x.clone())
    assert bool((s == 1).all()) and bool((cs == 1).all()), "identical images"
    z = torch.zeros(2, 27, 43, 4, device="cuda")
    s, cs = ops.ssim(z, z.clone())
    assert bool((s == 1).all()) and bool((cs == 1).all()), "all-zero images"
    z, o = torch.zeros(1, 12, 15, 1), torch.ones(1, 12, 15, 1)
    s, _ = ops.ssim(z.cuda(), o.cuda())
    want = C1 / (1 + C1)
    # the fp32 table's 121 products sum to 1 - defect: the DEFINITION sits defect / C2 + 2 defect (relative) off C1 / (1 + C1)
    defect = 1.0 - float(R.window().sum()) ** 2
    bound = float(R.ssim_bounds(z, o)[0].max()) + want * (defect / C2 + 2 * defect)
    print(f"x = 0, y = 1: {float(s):.9e} vs {want:.9e}, bound {bound:.2e}")
    assert abs(float(s.double()) - want) <= bound


def test_nan_stays_in_its_own_image_and_channel(ops):
    case = (3, 18, 18, 3)
    x, y = gpu_pair(case)
    clean_s, clean_cs = ops.ssim(x, y)
    x = x.clone()
    x[1, 9, 4, 2] = float("nan")
    s, cs = ops.ssim(x, y)
    hit = torch.zeros(3, 3, dtype=torch.bool, device="cuda")
    hit[1, 2] = True
    assert bool((torch.isnan(s) == hit).all()) and bool((torch.isnan(cs) == hit).all())
    assert torch.equal(s[~hit], clean_s[~hit]) and torch.equal(cs[~hit], clean_cs[~hit])


def test_two_runs_agree_bit_for_bit(ops):
    from nerf_atlas_amd import config
    x, y = gpu_pair((1, 176, 163, 3))
    g = R.upstream(1, 3).cuda()
    first = (*ops.ssim(x, y), ops.ssim_backward(x, y, g), ops.ms_ssim(x, y))
    again = (*ops.ssim(x, y), ops.ssim_backward(x, y, g), ops.ms_ssim(x, y))
    config.set_deterministic(True)
    try:
        det = (*ops.ssim(x, y), ops.ssim_backward(x, y, g), ops.ms_ssim(x, y))
    finally:
        config.set_deterministic(False)
    for a, b, c in zip(first, again, det):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_return_codes(ops):
    from nerf_atlas_amd import _lib
    lib = _lib.load()
    x, y = gpu_pair((1, 11, 13, 3))
    out = torch.zeros(1, 3, 2, device="cuda")
    ws = torch.zeros(64, device="cuda")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    err = lambda: lib.na_last_error().decode()
    fwd = lambda xx, yy, N, H, W, Cn, oo, ww, nb=256: lib.na_ssim(p(xx), p(yy), N, H, W, Cn, 1.0, p(oo), p(ww), nb, None)
    assert fwd(x, y, 1, 10, 13, 3, out, ws) == NA_EUNSUPPORTED and fwd(x, y, 1, 11, 10, 3, out, ws) == NA_EUNSUPPORTED
    assert fwd(x, y, 1, 11, 13, 0, out, ws) == NA_EUNSUPPORTED and fwd(x, y, 1, 11, 13, 5, out, ws) == NA_EUNSUPPORTED
    assert fwd(None, None, 0, 11, 13, 3, None, None, 0) == NA_OK
    for name, args in (("x", (None, y, out, ws)), ("y", (x, None, out, ws)), ("out", (x, y, None, ws)), ("workspace", (x, y, out, None))):
        assert fwd(args[0], args[1], 1, 11, 13, 3, args[2], args[3]) == NA_ENULL
        assert f"na_ssim: {name} is NULL" in err(), err()
    need = lib.na_ssim_workspace_bytes(1, 11, 13, 3)
    assert need == 3 * 2 * 4 and lib.na_ssim_workspace_bytes(2, 27, 43, 4) == 2 * 4 * (2 * 3) * 2 * 4 and lib.na_ssim_workspace_bytes(1, 10, 13, 3) == 0
    assert fwd(x, y, 1, 11, 13, 3, out, ws, need - 1) == NA_EWORKSPACE
    g, gx = torch.ones(1, 3, device="cuda"), torch.zeros_like(x)
    bwd = lambda xx, yy, gg, N, H, W, Cn, oo: lib.na_ssim_backward(p(xx), p(yy), p(gg), N, H, W, Cn, 1.0, p(oo), None)
    assert bwd(x, y, g, 1, 10, 13, 3, gx) == NA_EUNSUPPORTED and bwd(x, y, g, 1, 11, 13, 5, gx) == NA_EUNSUPPORTED
    assert bwd(None, None, None, 0, 11, 13, 3, None) == NA_OK
    for name, args in (("x", (None, y, g, gx)), ("y", (x, None, g, gx)), ("g", (x, y, None, gx)), ("g_x", (x, y, g, None))):
        assert bwd(args[0], args[1], args[2], 1, 11, 13, 3, args[3]) == NA_ENULL
        assert f"na_ssim_backward: {name} is NULL" in err(), err()
    ox = torch.zeros(1, 6, 7, 3, device="cuda")
    halve = lambda xx, yy, N, Cn, a, b: lib.na_image_halve(p(xx), p(yy), N, 11, 13, Cn, p(a), p(b), None)
    assert halve(x, None, 1, 5, ox, None) == NA_EUNSUPPORTED and halve(None, None, 0, 3, None, None) == NA_OK
    assert halve(None, None, 1, 3, ox, None) == NA_ENULL and "na_image_halve: x is NULL" in err()
    assert halve(x, None, 1, 3, None, None) == NA_ENULL and "na_image_halve: out_x is NULL" in err()
    assert halve(x, y, 1, 3, ox, None) == NA_ENULL and "out_y" in err()
    torch.cuda.synchronize()
    assert int(out.count_nonzero()) == 0 and int(gx.count_nonzero()) == 0 and int(ox.count_nonzero()) == 0, "a refused call wrote"
    with pytest.raises(ValueError):
        ops.ssim(x[:, :10], y[:, :10])
    with pytest.raises(ValueError):
        ops.ssim(torch.zeros(1, 11, 11, 5, device="cuda"), torch.zeros(1, 11, 11, 5, device="cuda"))


@pytest.mark.parametrize("shape", ((2, 12, 12, 3), (1, 11, 12, 1), (2, 13, 11, 4)))
def test_image_halve(ops, shape):
    x, y = R.image_pair(*shape)
    hx, hy = ops.image_halve(x.cuda(), y.cuda())
    assert tuple(hx.shape) == (shape[0], shape[1] // 2 + shape[1] % 2, shape[2] // 2 + shape[2] % 2, shape[3])
    rx, ry = R.worst_ratio(hx, R.halve_ref(x), R.halve_bound(x)), R.worst_ratio(hy, R.halve_ref(y), R.halve_bound(y))
    print(f"{shape}: ratios {rx:.3f} {ry:.3f}")
    assert rx <= 1 and ry <= 1
    assert torch.equal(ops.image_halve(x.cuda()), hx)   # one image alone


@pytest.mark.parametrize("case", R.MS_CASES)
def test_ms_ssim_within_the_bound(ops, case):
    ref, bound = R.ms_reference(case)
    got = ops.ms_ssim(*gpu_pair(case))
    ratio = R.worst_ratio(got, ref, bound)
    print(f"{case}: ms-ssim {got.flatten().tolist()} err {float((got.cpu().double() - ref).abs().max()):.2e} (bound {float(bound.max()):.2e}, ratio {ratio:.3f})")
    assert tuple(got.shape) == (case[0], case[3]) and ratio <= 1


def test_ms_ssim_size_check_and_relu(ops):
    z = torch.zeros(1, 160, 161, 3, device="cuda")
    with pytest.raises(ValueError, match="larger than 160"):
        ops.ms_ssim(z, z)
    x, y = R.noise_pair(1, 161, 161, 3)
    got = ops.ms_ssim(x.cuda(), y.cuda())
    assert bool((got == 0).all()), got


def test_ssim_loss_gradient_is_the_references(ops):
    from nerf_atlas_amd import train as T
    case = (2, 16, 16, 3)
    x, y = R.image_pair(*case)
    xg = x.cuda().requires_grad_(True)
    loss = T.load_loss_fn(T.make_args(loss_fns=["ssim"]))(xg, y.cuda())
    loss.backward()
    gup = torch.full((2, 3), -1.0 / 6.0, dtype=torch.float64)
    g_ref = R.ssim_grad_ref(x, y, gup)
    bound = R.ssim_grad_terms(x, y, gup)[1] + R.U * g_ref.abs()          # (+ u: the fp32 rounding of 1 / 6)
    s_ref, _, bs, _ = R.ssim_reference(case)
    ratio = R.worst_ratio(xg.grad, g_ref, bound)
    l_err = abs(float(loss.detach().double()) - (1 - float(s_ref.mean())))
    l_bound = float(bs.mean()) + 8 * R.U                                     # (the mean of six and 1 - mean, in fp32)
    print(f"loss {float(loss.detach()):.7f} err {l_err:.2e} (bound {l_bound:.2e}); gradient ratio {ratio:.3f}")
    assert l_err <= l_bound and ratio <= 1
    # averaged with another entry, as --loss-fns l2 ssim does
    both = T.load_loss_fn(T.make_args(loss_fns=["l2", "ssim"]))(x.cuda(), y.cuda())
    assert abs(float(both) - 0.5 * (float(torch.nn.functional.mse_loss(x, y)) + float(loss.detach()))) <= 1e-6


def test_runner_reports_ssim_and_ms_ssim(ops, tmp_path):
    """--model voxel --refl-kind pos --loss-fns l2 ssim --msssim-loss on the analytic Blender-format scene at 176 x 176"""
    from tools.make_scene import make_scene
    from nerf_atlas_amd import runner
    data = make_scene(str(tmp_path / "s"), size=176, n_train=3, n_test=2) + "/"
    argv = ["-d", data, "--size", "176", "--crop-size", "16", "--test-crop-size", "176", "--batch-size", "2", "--steps", "24", "--epochs", "4",
            "--quiet", "--model", "voxel", "--refl-kind", "pos", "-lr", "1e-2", "--loss-fns", "l2", "ssim"]
    res = runner.main(argv + ["--msssim-loss", "--outdir", str(tmp_path / "a")])
    assert len(res["losses"]) == 4 and all(np.isfinite(res["losses"]))
    frames = torch.stack([f.cpu() for f in res["frames"]])
    labels = res["test_labels"][..., :3].cpu()
    s_ref, _ = R.ssim_ref(frames, labels)
    bs, _ = R.ssim_bounds(frames, labels)
    ms_ref, ms_bound = R.ms_ssim_bound(frames, labels)
    got_s = torch.tensor(res["test_ssim"], dtype=torch.float64)
    r_s = R.worst_ratio(got_s, s_ref.mean(dim=1), bs.mean(dim=1) + 4 * R.U)    # (+ the fp32 mean over three channels)
    ms_err, ms_b = abs(res["test_msssim"] - float(ms_ref.mean())), float(ms_bound.mean()) + 4 * R.U
    print(f"test_ssim {res['test_ssim']} (ratio {r_s:.3f}); test_msssim {res['test_msssim']:.7f} err {ms_err:.2e} (bound {ms_b:.2e})")
    assert len(res["test_ssim"]) == 2 and r_s <= 1 and ms_err <= ms_b
    txt = (tmp_path / "a" / "results.txt").read_text()
    assert txt.endswith(f"\nms-ssim {res['test_msssim']:.03f}") and txt.count("ms-ssim") == 1 and txt.count("PSNR") == 2
    res = runner.main(argv + ["--outdir", str(tmp_path / "b")])
    assert "test_ssim" not in res and "test_msssim" not in res
    assert "ms-ssim" not in (tmp_path / "b" / "results.txt").read_text()


def test_small_frames_fail_softly(ops, capsys):
    from nerf_atlas_amd import train as T
    x, y = gpu_pair((2, 26, 26, 3))
    ssims, ms = T.test_similarity(list(x), y)
    assert len(ssims) == 2 and ms is None and "msssim failed:" in capsys.readouterr().out
