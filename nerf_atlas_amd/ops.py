"""Torch-tensor wrappers over the C ABI (include/nerf_atlas_amd.h).

PyTorch is only the memory/stream plumbing here: every function checks its tensors (cuda, fp32,
contiguous), passes raw device pointers + the current HIP stream to the HIP library and returns the
output tensor.  There is no eager/CPU fallback.
"""
import ctypes as C
import math
import struct
from typing import Optional, Sequence

import torch

from . import _lib, config
from ._lib import NaMlpDesc, check

ACT = {"none": 0, "leaky_relu": 1, "sin": 2}
ENC = {"none": 0, "hash": 1, "fourier": 2}
# (f16: everything but the register-engine renderer na_render_plain_view; f16x: render_ls_pack / render_plain_view_ls only)
PREC = {"bf16": 0, "bf16x3": 1, "f16": 2, "f16x": 3}
LAYOUT = {"generic": 0, "plain_first": 1, "plain_view": 2}
BG = {"black": 0, "white": 1}
SIGMOID = {"normal": 0, "thin": 1, "fat": 2, "tanh": 3, "upshifted": 4, "relu": 5, "sin": 6, "leaky_relu": 7,
           "upshifted_softplus": 8, "upshifted_relu": 9, "cyclic": 10, "identity": 11}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class F16xSaturated(_lib.NaError):
    """An f16x launch met an activation beyond the IEEE-half range (its output is the NaN frame): config.set_f16x_on_saturation."""


def _f16x_guard(precision: str, out: torch.Tensor, what: str):
    """config.f16x_on_saturation "raise" / "rerender_bf16x3": read one element of the launch's output back (the range guard poisons
    the whole of it) and raise when it is the flagged frame.  "nan" (default): nothing, no synchronisation."""
    if precision == "f16x" and config.f16x_on_saturation != "nan" and out.numel() > 0:
        if bool(torch.isnan(out.reshape(-1)[0])):
            raise F16xSaturated(f"{what}: an activation left the half range (f16x output poisoned); render these weights in bf16x3")


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA(HIP) tensor: the hot path has no CPU implementation")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------- rays / samples
def raygen(c2w: torch.Tensor, focal: float, size: int, crop, noise: Optional[torch.Tensor] = None,
           with_noise: float = 0.0) -> torch.Tensor:
    """rays[B,h,w,6] for crop (t,l,h,w) clipped to the image like the reference's slicing (runner.py:490-503,
    src/cameras.py:45-66)."""
    lib = _lib.load()
    c2w = _f32(c2w, "c2w")
    B = c2w.shape[0]
    t, l, h, w = crop
    h = max(0, min(h, size - t))
    w = max(0, min(w, size - l))
    rays = torch.empty(B, h, w, 6, device=c2w.device, dtype=torch.float32)
    nz = None
    if noise is not None and with_noise:
        nz = _f32(noise, "noise")
        assert nz.shape == (h, w, 2), nz.shape
    check(lib.na_raygen(_ptr(c2w), B, float(focal), int(size), t, l, h, w, _ptr(nz), float(with_noise or 0.0),
                        _ptr(rays), _stream()))
    return rays


def raygen_dtu(pose: torch.Tensor, intrinsic: torch.Tensor, size: int, crop) -> torch.Tensor:
    lib = _lib.load()
    pose, intrinsic = _f32(pose, "pose"), _f32(intrinsic, "intrinsic")
    B = pose.shape[0]
    t, l, h, w = crop
    h = max(0, min(h, size - t))
    w = max(0, min(w, size - l))
    rays = torch.empty(B, h, w, 6, device=pose.device, dtype=torch.float32)
    check(lib.na_raygen_dtu(_ptr(pose), _ptr(intrinsic), B, int(size), t, l, h, w, _ptr(rays), _stream()))
    return rays


def compute_ts(near: float, far: float, steps: int, device, lindisp: bool = False, perturb: float = 0.0,
               rand: Optional[torch.Tensor] = None, want_mids: bool = False):
    lib = _lib.load()
    ts = torch.empty(steps, device=device, dtype=torch.float32)
    mids = torch.empty(max(steps - 1, 0), device=device, dtype=torch.float32) if (want_mids or perturb > 0) else None
    if perturb > 0:
        rand = _f32(rand, "rand")
        assert rand.shape == (steps,)
    check(lib.na_compute_ts(float(near), float(far), int(steps), int(lindisp), float(perturb), _ptr(rand), _ptr(ts),
                            _ptr(mids), _stream()))
    return ts, (mids if perturb > 0 else None)


def compute_pts(rays: torch.Tensor, ts: torch.Tensor) -> torch.Tensor:
    """pts[T, *rays.shape[:-1], 3] (src/nerf.py:50-55)."""
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    R = rays.numel() // 6
    T = ts.shape[0]
    pts = torch.empty((T,) + tuple(rays.shape[:-1]) + (3,), device=rays.device, dtype=torch.float32)
    check(lib.na_compute_pts(_ptr(rays), _ptr(ts), T, R, _ptr(pts), _stream()))
    return pts


# ------------------------------------------------------------------------------------------------- encoders
def hash_encode(x: torch.Tensor, tables: torch.Tensor, include_input: bool = True, want_indices: bool = False):
    lib = _lib.load()
    x, tables = _f32(x, "x"), _f32(tables, "tables")
    assert x.shape[-1] == 3 and tables.shape == (8, 65536, 4), (x.shape, tables.shape)
    N = x.numel() // 3
    out = torch.empty(tuple(x.shape[:-1]) + (32 + 3 * int(include_input),), device=x.device, dtype=torch.float32)
    idx = torch.empty(8, 8, N, device=x.device, dtype=torch.int64) if want_indices else None
    check(lib.na_hash_encode(_ptr(x), N, _ptr(tables), int(include_input), _ptr(out), _ptr(idx), _stream()))
    return (out, idx) if want_indices else out


def hash_encode_rows(x: torch.Tensor, tables: torch.Tensor, include_input: bool = True, lead: int = 1) -> torch.Tensor:
    """[N, 32 + 3 (include_input + lead)] rows [x (lead) | x (include_input) | features]: with lead = 1 the init rows cat([p, enc(p)])
    of a hash-encoded SkipConnMLP, written by the encoder (na_hash_encode_rows)."""
    lib = _lib.load()
    x, tables = _f32(x, "x"), _f32(tables, "tables")
    assert x.dim() == 2 and x.shape[-1] == 3 and tables.shape == (8, 65536, 4), (x.shape, tables.shape)
    N = x.shape[0]
    out = torch.empty(N, 32 + 3 * (int(include_input) + lead), device=x.device, dtype=torch.float32)
    check(lib.na_hash_encode_rows(_ptr(x), N, _ptr(tables), int(include_input), lead, _ptr(out), _stream()))
    return out


def plain_head_rows(first_out: torch.Tensor, pts: torch.Tensor, dirs: torch.Tensor):
    """first_out [N, 1 + C], pts [N = T x R, 3], dirs [R, 3] -> (density [N], rows [N, 5 + C] = [x | elev, azim | first_out[:, 1:]])."""
    lib = _lib.load()
    first_out, pts, dirs = _f32(first_out, "first_out"), _f32(pts, "pts"), _f32(dirs, "dirs")
    N, C = first_out.shape[0], first_out.shape[1] - 1
    R = dirs.numel() // 3
    assert pts.numel() == 3 * N and N % R == 0, (pts.shape, dirs.shape, N)
    density = torch.empty(N, device=pts.device, dtype=torch.float32)
    rows = torch.empty(N, 5 + C, device=pts.device, dtype=torch.float32)
    check(lib.na_plain_head_rows(_ptr(first_out), _ptr(pts), _ptr(dirs), N, R, C, _ptr(density), _ptr(rows), _stream()))
    return density, rows


def plain_head_rows_backward(g_density, g_rows: torch.Tensor, want_pts: bool):
    lib = _lib.load()
    g_rows = _f32(g_rows, "g_rows")
    N, C = g_rows.shape[0], g_rows.shape[1] - 5
    g_density = None if g_density is None else _f32(g_density, "g_density")
    g_first = torch.empty(N, 1 + C, device=g_rows.device, dtype=torch.float32)
    g_pts = torch.empty(N, 3, device=g_rows.device, dtype=torch.float32) if want_pts else None
    check(lib.na_plain_head_rows_backward(None if g_density is None else _ptr(g_density), _ptr(g_rows), N, C, _ptr(g_first),
                                          None if g_pts is None else _ptr(g_pts), _stream()))
    return g_first, g_pts


def hash_encode_backward_rows(x: torch.Tensor, g_rows: torch.Tensor, col0: int) -> torch.Tensor:
    """tables gradient from the 32 feature columns col0.. of wider gradient rows, read in place"""
    lib = _lib.load()
    x, g_rows = _f32(x, "x"), _f32(g_rows, "g_rows")
    N = x.numel() // 3
    assert g_rows.dim() == 2 and g_rows.shape[0] == N
    tg = torch.zeros(8, 65536, 4, device=x.device, dtype=torch.float32)
    check(lib.na_hash_encode_backward_rows(_ptr(x), N, _ptr(g_rows), g_rows.shape[1], col0, _ptr(tg), _stream()))
    return tg


def hash_encode_backward_input_rows(x: torch.Tensor, tables: torch.Tensor, g_rows: torch.Tensor, include_input: bool, lead: int) -> torch.Tensor:
    lib = _lib.load()
    x, tables, g_rows = _f32(x, "x"), _f32(tables, "tables"), _f32(g_rows, "g_rows")
    N = x.numel() // 3
    assert g_rows.dim() == 2 and g_rows.shape[0] == N
    gx = torch.empty_like(x)
    check(lib.na_hash_encode_backward_input_rows(_ptr(x), N, _ptr(tables), _ptr(g_rows), g_rows.shape[1], int(include_input), lead,
                                                 _ptr(gx), _stream()))
    return gx


def fourier_encode(x: torch.Tensor, basis: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    lib = _lib.load()
    x, basis = _f32(x, "x"), _f32(basis, "basis")
    D, F = basis.shape
    assert x.shape[-1] == D
    N = x.numel() // D
    out = torch.empty(tuple(x.shape[:-1]) + (2 * F,), device=x.device, dtype=torch.float32)
    check(lib.na_fourier_encode(_ptr(x), N, D, _ptr(basis), F, float(scale), _ptr(out), _stream()))
    return out


def _fourier_args(x: torch.Tensor, basis: torch.Tensor):
    x, basis = _f32(x, "x"), _f32(basis, "basis")
    D, F = basis.shape
    assert x.dim() == 2 and x.shape[1] == D and 1 <= D <= 8, (x.shape, basis.shape)
    return x, basis, D, F


def fourier_rows(x: torch.Tensor, basis: torch.Tensor, scale: float = 1.0, latent: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, D + 2F + L] rows [x | sin(x B) | cos(x B) | latent]: the init rows cat([p, enc(p), latent]) of a Fourier-encoded SkipConnMLP,
    written by one launch (na_fourier_rows).  latent [N, L]: a column slice of a wider buffer goes down with its row pitch."""
    lib = _lib.load()
    x, basis, D, F = _fourier_args(x, basis)
    N, L, lat_ld = x.shape[0], 0, 0
    if latent is not None and latent.shape[-1] > 0:
        latent, lat_ld = _rows(latent, latent.shape[-1], "latent")
        L = latent.shape[1]
        assert latent.shape[0] == N, (latent.shape, N)
    else:
        latent = None
    rows = torch.empty(N, D + 2 * F + L, device=x.device, dtype=torch.float32)
    check(lib.na_fourier_rows(_ptr(x), N, D, _ptr(basis), F, float(scale), _ptr(latent), L, lat_ld, _ptr(rows), _stream()))
    return rows


def fourier_encode_backward_input(x: torch.Tensor, basis: torch.Tensor, scale: float, g: torch.Tensor, col0: int = 0, lead: bool = False,
                                  saved: Optional[torch.Tensor] = None, saved_col0: int = 0) -> torch.Tensor:
    """g_x [N, D] of the Fourier features w.r.t. the positions: the 2F columns [g_sin | g_cos] at col0 of the gradient rows g [N, g_ld],
    read in place; lead: g[:, :D] (the raw columns of init rows) is added.  saved [N, s_ld]: read sin / cos back from these rows (their
    sine columns at saved_col0) instead of recomputing them -- the alternative tools/fourier_grad_bench.py measures."""
    lib = _lib.load()
    x, basis, D, F = _fourier_args(x, basis)
    g = _f32(g, "g")
    N = x.shape[0]
    assert g.dim() == 2 and g.shape[0] == N and g.shape[1] >= col0 + 2 * F and col0 >= (D if lead else 0), (g.shape, col0, lead, D, F)
    gx = torch.empty_like(x)
    if saved is None:
        check(lib.na_fourier_encode_backward_input(_ptr(x), N, D, _ptr(basis), F, float(scale), _ptr(g), g.shape[1], col0, int(lead),
                                                   _ptr(gx), _stream()))
    else:
        saved = _f32(saved, "saved")
        assert saved.dim() == 2 and saved.shape[0] == N and saved.shape[1] >= saved_col0 + 2 * F, (saved.shape, saved_col0, F)
        check(lib.na_fourier_encode_backward_input_saved(_ptr(x), N, D, _ptr(basis), F, float(scale), _ptr(g), g.shape[1], col0, int(lead),
                                                         _ptr(saved), saved.shape[1], saved_col0, _ptr(gx), _stream()))
    return gx


def positional_encode(x: torch.Tensor, bands: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x, bands = _f32(x, "x"), _f32(bands, "bands")
    D, NB = x.shape[-1], bands.shape[0]
    N = x.numel() // D
    out = torch.empty(tuple(x.shape[:-1]) + (2 * D * NB,), device=x.device, dtype=torch.float32)
    check(lib.na_positional_encode(_ptr(x), N, D, _ptr(bands), NB, _ptr(out), _stream()))
    return out


def view_elaz(dirs: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    dirs = _f32(dirs, "dirs")
    N = dirs.numel() // 3
    out = torch.empty(tuple(dirs.shape[:-1]) + (2,), device=dirs.device, dtype=torch.float32)
    check(lib.na_view_elaz(_ptr(dirs), N, _ptr(out), _stream()))
    return out


def view_rows(pts: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """[..., R, 5] rows [x, y, z, elev, azim]: pts [..., R, 3] with one direction per ray dirs [R, 3] (na_view_rows)."""
    lib = _lib.load()
    pts, dirs = _f32(pts, "pts"), _f32(dirs, "dirs")
    R = dirs.shape[0]
    assert pts.shape[-2] == R and pts.shape[-1] == 3 and dirs.shape == (R, 3)
    out = torch.empty(tuple(pts.shape[:-1]) + (5,), device=pts.device, dtype=torch.float32)
    check(lib.na_view_rows(_ptr(pts), _ptr(dirs), pts.numel() // 3, R, _ptr(out), _stream()))
    return out


def sigmoid(x: torch.Tensor, kind: str) -> torch.Tensor:
    lib = _lib.load()
    if kind not in SIGMOID:
        raise NotImplementedError(f"Unknown sigmoid kind({kind})")
    x = _f32(x, "x")
    out = torch.empty_like(x)
    check(lib.na_sigmoid(_ptr(x), x.numel(), SIGMOID[kind], _ptr(out), _stream()))
    return out


MIP_KIND = {"cylinder": 0, "cone": 1}


def mip_encode(rays: torch.Tensor, ts: torch.Tensor, kind: str, t_end: float, min_deg: int = 0, max_deg: int = 16):
    """rays [B,H,W,6] of ONE crop -> [T,B,H,W,6*(max_deg-min_deg)] (intended layout)."""
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    B, H, W, _ = rays.shape
    T = ts.shape[0]
    out = torch.empty(T, B, H, W, 6 * (max_deg - min_deg), device=rays.device, dtype=torch.float32)
    check(lib.na_mip_encode(_ptr(rays), B, H, W, _ptr(ts), T, MIP_KIND[kind], float(t_end), min_deg,
                            max_deg, _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------- compositing
def composite(density: torch.Tensor, feat: torch.Tensor, ts: torch.Tensor, rays: torch.Tensor, softplus: bool = True,
              bg: str = "black", want_weights: bool = True, rand: Optional[torch.Tensor] = None):
    """density [T,...], feat [T,...,C], rays [...,6] -> (out [...,C], alpha [T,...], weights [T,...]).
    bg "random" (src/nerf.py:99-103) takes the per-ray uniform draw `rand` [..., 1]."""
    lib = _lib.load()
    density, feat, ts, rays = _f32(density, "density"), _f32(feat, "feat"), _f32(ts, "ts"), _f32(rays, "rays")
    T = ts.shape[0]
    Cn = feat.shape[-1]
    R = rays.numel() // 6
    assert density.numel() == T * R and feat.numel() == T * R * Cn, (density.shape, feat.shape, rays.shape)
    if bg not in BG and bg != "random":
        raise NotImplementedError(bg)
    out = torch.empty(tuple(rays.shape[:-1]) + (Cn,), device=rays.device, dtype=torch.float32)
    alpha = torch.empty_like(density) if want_weights else None
    weights = torch.empty_like(density) if want_weights else None
    if bg == "random":
        rand = _f32(rand, "rand")
        assert rand.numel() == R, (rand.shape, rays.shape)
        check(lib.na_composite_random_bg(_ptr(density), _ptr(feat), _ptr(ts), _ptr(rays), T, R, Cn, 0 if softplus else 1,
                                         _ptr(rand), _ptr(alpha), _ptr(weights), _ptr(out), _stream()))
        return out, alpha, weights
    check(lib.na_composite(_ptr(density), _ptr(feat), _ptr(ts), _ptr(rays), T, R, Cn, 0 if softplus else 1, BG[bg],
                           _ptr(alpha), _ptr(weights), _ptr(out), _stream()))
    return out, alpha, weights


def sky_random(weights: torch.Tensor, rand: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """out[..., :] += rand[..., 0] * (1 - sum(weights[:-1])) in place (src/nerf.py:101-103); weights [T,...], rand [...,1]."""
    lib = _lib.load()
    weights, rand = _f32(weights, "weights"), _f32(rand, "rand")
    assert out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda
    T = weights.shape[0]
    R = weights.numel() // T
    assert rand.numel() == R and out.numel() % R == 0, (weights.shape, rand.shape, out.shape)
    check(lib.na_sky_random(_ptr(weights), _ptr(rand), T, R, out.numel() // R, _ptr(out), _stream()))
    return out


def integrate(weights: torch.Tensor, other: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    weights, other = _f32(weights, "weights"), _f32(other, "other")
    T = weights.shape[0]
    R = weights.numel() // T
    Cn = other.shape[-1]
    out = torch.empty(tuple(weights.shape[1:]) + (Cn,), device=weights.device, dtype=torch.float32)
    check(lib.na_integrate(_ptr(weights), _ptr(other), T, R, Cn, _ptr(out), _stream()))
    return out


def normalize3(v: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    v = _f32(v, "v")
    out = torch.empty_like(v)
    check(lib.na_normalize3(_ptr(v), v.numel() // 3, _ptr(out), _stream()))
    return out


def pos_linear_combine(lin: torch.Tensor, pos: torch.Tensor, C_out: int) -> torch.Tensor:
    """(sigmoid(lin)/2 + 0.5) * pos[..., :C_out]; pos may be wider (its first C_out columns are used, by row pitch)."""
    if torch.is_grad_enabled() and (lin.requires_grad or pos.requires_grad):
        raise RuntimeError("ops.pos_linear_combine is not differentiable: go through autograd.PosLinearCombineFn")
    lib = _lib.load()
    lin = _f32(lin, "lin")
    pos2, ld = _rows(pos, pos.shape[-1], "pos")
    N = lin.numel()
    assert pos2.shape[0] == N and C_out <= pos.shape[-1]
    out = torch.empty(tuple(lin.shape[:-1]) + (C_out,), device=lin.device, dtype=torch.float32)
    check(lib.na_pos_linear_combine(_ptr(lin), _ptr(pos2), ld, N, C_out, _ptr(out), _stream()))
    return out


def pos_linear_combine_backward(lin: torch.Tensor, pos: torch.Tensor, g: torch.Tensor, C_out: int, want_lin=True,
                                want_pos=True):
    """Gradients of pos_linear_combine w.r.t. lin [...,1] and pos [...,W] (columns >= C_out get zeros)."""
    lib = _lib.load()
    lin, g = _f32(lin, "lin"), _f32(g, "g")
    pos2, ld = _rows(pos, pos.shape[-1], "pos")
    N = lin.numel()
    g_lin = torch.empty_like(lin) if want_lin else None
    g_pos = torch.empty(pos.shape, device=pos.device, dtype=torch.float32) if want_pos else None
    check(lib.na_pos_linear_combine_backward(_ptr(lin), _ptr(pos2), ld, _ptr(g), N, C_out,
                                             _ptr(g_lin) if want_lin else None, _ptr(g_pos) if want_pos else None,
                                             pos.shape[-1], _stream()))
    return g_lin, g_pos


def laplace_density(sdf: torch.Tensor, beta: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    sdf = _f32(sdf, "sdf")
    beta = _f32(beta.reshape(1), "beta")
    out = torch.empty_like(sdf)
    check(lib.na_laplace_density(_ptr(sdf), sdf.numel(), _ptr(beta), _ptr(out), _stream()))
    return out


def bezier_warp(est: torch.Tensor, pts: torch.Tensor, t: torch.Tensor, n_ctrl: int, n_rl: int = 0):
    """est [...,>=1+3n] (rigidity | control points), pts [...,3], t [...] -> (pts', dp, rigidity); with n_rl > 0 (DynamicNeRF's
    refl_latent: est [..., >= 2 + (3 + n_rl) n] = ... | enc_rigidity | latent control rows) -> (pts', dp, rigidity, refl_latent [..., n_rl])."""
    lib = _lib.load()
    est, pts, t = _f32(est, "est"), _f32(pts, "pts"), _f32(t, "t")
    N = pts.numel() // 3
    assert t.numel() == N and est.numel() // est.shape[-1] == N
    out = torch.empty_like(pts)
    dp = torch.empty_like(pts)
    rig = torch.empty(tuple(pts.shape[:-1]) + (1,), device=pts.device, dtype=torch.float32)
    if n_rl > 0:
        enc = torch.empty(tuple(pts.shape[:-1]) + (n_rl,), device=pts.device, dtype=torch.float32)
        check(lib.na_bezier_warp_latent(_ptr(est), est.shape[-1], _ptr(pts), _ptr(t), N, n_ctrl, n_rl, _ptr(out), _ptr(dp), _ptr(rig),
                                        _ptr(enc), _stream()))
        return out, dp, rig, enc
    check(lib.na_bezier_warp(_ptr(est), est.shape[-1], _ptr(pts), _ptr(t), N, n_ctrl, _ptr(out), _ptr(dp), _ptr(rig),
                             _stream()))
    return out, dp, rig


# ------------------------------------------------------------------------------------------------- SDF marching
def ray_points(r_o: torch.Tensor, r_d: torch.Tensor, t) -> torch.Tensor:
    """r_o + r_d * t; t a float or a per-ray tensor [..., 1] / [...]."""
    lib = _lib.load()
    r_o, r_d = _f32(r_o, "r_o"), _f32(r_d, "r_d")
    R = r_o.numel() // 3
    pts = torch.empty_like(r_o)
    if torch.is_tensor(t):
        t = _f32(t, "t")
        assert t.numel() == R
        check(lib.na_ray_points(_ptr(r_o), _ptr(r_d), _ptr(t), 0.0, R, _ptr(pts), _stream()))
    else:
        check(lib.na_ray_points(_ptr(r_o), _ptr(r_d), None, float(t), R, _ptr(pts), _stream()))
    return pts


def compact_rays(live: torch.Tensor, idx: torch.Tensor, count: torch.Tensor) -> int:
    """idx[:n] = ascending indices of the rays with live != 0 (uint8 mask of any shape); returns n -- one host read of the
    device counter (the reference's boolean-mask indexing synchronises at the same point).  idx: int32 [R + 256], count: int32 [1]."""
    lib = _lib.load()
    assert live.dtype == torch.uint8 and live.is_contiguous() and idx.dtype == torch.int32 and idx.numel() >= live.numel() + 256
    check(lib.na_compact_rays(_ptr(live), live.numel(), _ptr(idx), _ptr(count), _stream()))
    return int(count.item())


def ray_points_indexed(r_o, r_d, t_ray, idx, n: int) -> torch.Tensor:
    """[n,3] positions r_o + r_d * t of the compacted rays idx[:n]"""
    lib = _lib.load()
    pts = torch.empty(n, 3, device=r_o.device, dtype=torch.float32)
    check(lib.na_ray_points_indexed(_ptr(r_o), _ptr(r_d), _ptr(t_ray), _ptr(idx), n, _ptr(pts), _stream()))
    return pts


def sphere_march_update_indexed(sdf, idx, n: int, eps: float, far: float, dist, hits, rem):
    lib = _lib.load()
    sdf, stride = _sdf_col(sdf)
    check(lib.na_sphere_march_update_indexed(_ptr(sdf), stride, _ptr(idx), n, float(eps), float(far), _ptr(dist), _ptr(hits),
                                             _ptr(rem), _stream()))


def bisection_update_indexed(sdf_mid, idx, n: int, eps: float, low, high, sdf_low, sdf_high, z, todo):
    lib = _lib.load()
    sdf_mid, stride = _sdf_col(sdf_mid)
    check(lib.na_bisection_update_indexed(_ptr(sdf_mid), stride, _ptr(idx), n, float(eps), _ptr(low), _ptr(high), _ptr(sdf_low),
                                          _ptr(sdf_high), _ptr(z), _ptr(todo), _stream()))


def _sdf_col(sdf: torch.Tensor):
    sdf = _f32(sdf, "sdf")
    return sdf, (sdf.shape[-1] if sdf.dim() > 1 else 1)


def sphere_march_update(sdf, eps: float, far: float, dist, hits, rem):
    lib = _lib.load()
    sdf, stride = _sdf_col(sdf)
    check(lib.na_sphere_march_update(_ptr(sdf), stride, dist.numel(), float(eps), float(far), _ptr(dist), _ptr(hits),
                                     _ptr(rem), _stream()))


def sign_change_update(sdf, step: int, curr_min, idxs, last_pos, first_neg):
    lib = _lib.load()
    sdf, stride = _sdf_col(sdf)
    check(lib.na_sign_change_update(_ptr(sdf), stride, curr_min.numel(), int(step), _ptr(curr_min), _ptr(idxs),
                                    _ptr(last_pos), _ptr(first_neg), _stream()))


def bisection_update(sdf_mid, eps: float, low, high, sdf_low, sdf_high, z, todo):
    lib = _lib.load()
    stride = 1
    if sdf_mid is not None:
        sdf_mid, stride = _sdf_col(sdf_mid)
    check(lib.na_bisection_update(_ptr(sdf_mid), stride, low.numel(), float(eps), _ptr(low), _ptr(high), _ptr(sdf_low),
                                  _ptr(sdf_high), _ptr(z), _ptr(todo), _stream()))


# ------------------------------------------------------------------------------------------------- MLP


# ---------------------------------------------------------------------------------------- N4 lights / occlusion
def point_light(x: torch.Tensor, center: torch.Tensor, intensity: torch.Tensor, distance_decay: bool = True):
    """src/lights.py:118-132: (unit direction to the light, distance [..., 1], spectrum [..., 3]) for points x [..., 3];
    center / intensity hold one light ([3]) or one per point (x.shape)."""
    lib = _lib.load()
    x, center, intensity = _f32(x, "x"), _f32(center, "center"), _f32(intensity, "intensity")
    N = x.numel() // 3
    strides = []
    for t, name in ((center, "center"), (intensity, "intensity")):
        assert t.numel() in (3, 3 * N), f"{name}: one light or one per point"
        strides.append(3 if (t.numel() == 3 * N and N > 1) else 0)
    d = torch.empty_like(x)
    dist = torch.empty(tuple(x.shape[:-1]) + (1,), device=x.device, dtype=torch.float32)
    spectrum = torch.empty_like(x)
    check(lib.na_point_light(_ptr(x), _ptr(center), strides[0], _ptr(intensity), strides[1], int(bool(distance_decay)), N,
                             _ptr(d), _ptr(dist), _ptr(spectrum), _stream()))
    return d, dist, spectrum


def occlusion_apply(spectrum: torch.Tensor, visible: Optional[torch.Tensor] = None, raw_att: Optional[torch.Tensor] = None,
                    att_mode: int = 0, hidden_value: float = 0.0) -> torch.Tensor:
    """spectrum * a(raw_att) * v(visible): see include/nerf_atlas_amd.h (src/renderers.py:40-45,65-67,82-83,118-121)."""
    lib = _lib.load()
    spectrum = _f32(spectrum, "spectrum")
    N = spectrum.numel() // 3
    vis = None
    if visible is not None:
        assert visible.dtype == torch.bool and visible.numel() == N and visible.is_cuda
        vis = visible.contiguous().view(torch.uint8)
    if raw_att is not None:
        raw_att = _f32(raw_att, "raw_att")
        assert raw_att.numel() == N
    out = torch.empty_like(spectrum)
    check(lib.na_occlusion_apply(_ptr(spectrum), _ptr(vis), _ptr(raw_att), int(att_mode), float(hidden_value), N, _ptr(out),
                                 _stream()))
    return out


def linear_f32(x0: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor], pre_act: str = "none",
               x1: Optional[torch.Tensor] = None, split_bf16: bool = False, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = W . act([x0 | x1]) + b: exact fp32 (f32 MFMA), or with split_bf16 the 3-product bf16 split used by the
    training step (relative error ~2^-16, 5x the matrix-core rate).  packed: W as train_pack_many left it (split_bf16 only)."""
    lib = _lib.load()
    x0, W = _f32(x0, "x0"), _f32(W, "W")
    N = x0.shape[0]
    in0 = x0.shape[1]
    in1 = 0
    if x1 is not None:
        x1 = _f32(x1, "x1")
        in1 = x1.shape[1]
    assert W.shape[1] == in0 + in1, (W.shape, in0, in1)
    if b is not None:
        b = _f32(b, "b")
    y = torch.empty(N, W.shape[0], device=x0.device, dtype=torch.float32)
    if split_bf16 and packed is not None:
        check(lib.na_linear_bf16x3_pk(_ptr(x0), in0, _ptr(x1), in1, N, _ptr(packed), _ptr(b), W.shape[0], ACT[pre_act], _ptr(y),
                                      _stream()))
        return y
    fn = lib.na_linear_bf16x3 if split_bf16 else lib.na_linear_f32
    check(fn(_ptr(x0), in0, _ptr(x1), in1, N, _ptr(W), _ptr(b), W.shape[0], ACT[pre_act], _ptr(y), _stream()))
    return y


def linear_f32_rows(x0: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor], pre_act: str = "none",
                    x1: Optional[torch.Tensor] = None, b_rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y [N, out] = W . act([x0 | x1]) + bias, exact fp32 like linear_f32 (na_linear_f32_rows).  x0 [..., in0] / x1 [..., in1] may be
    column slices of wider buffers (`first_out[..., 1:]`): their row pitch goes down, no copy.  bias: b [out], or b_rows [R, out]
    added as b_rows[n % R] (sample-major rows n = t R + r), or none."""
    lib = _lib.load()
    W = _f32(W, "W")
    out = W.shape[0]
    x0, ld0 = _rows(x0, x0.shape[-1], "x0")
    N, in0 = x0.shape
    in1, ld1 = 0, 0
    if x1 is not None:
        x1, ld1 = _rows(x1, x1.shape[-1], "x1")
        in1 = x1.shape[1]
        assert x1.shape[0] == N, (x1.shape, N)
    assert W.dim() == 2 and W.shape[1] == in0 + in1, (W.shape, in0, in1)
    assert b is None or b_rows is None, "pass the broadcast bias or the per-ray bias, not both"
    R = 1
    if b is not None:
        b = _f32(b, "b")
        assert b.shape == (out,), b.shape
    if b_rows is not None:
        b_rows = _f32(b_rows, "b_rows")
        assert b_rows.dim() == 2 and b_rows.shape[1] == out and b_rows.shape[0] >= 1 and N % b_rows.shape[0] == 0, (b_rows.shape, N, out)
        R = b_rows.shape[0]
    y = torch.empty(N, out, device=x0.device, dtype=torch.float32)
    check(lib.na_linear_f32_rows(_ptr(x0), in0, ld0, _ptr(x1), in1, ld1, N, _ptr(W), _ptr(b), _ptr(b_rows), R, out, ACT[pre_act],
                                 _ptr(y), _stream()))
    return y


# ------------------------------------------------------------------------------------------------- spherical-harmonic head
def _sh_dirs(dirs: torch.Tensor, N: int):
    dirs = _f32(dirs, "dirs")
    assert dirs.dim() == 2 and dirs.shape[1] == 3 and dirs.shape[0] >= 1 and N % dirs.shape[0] == 0, (dirs.shape, N)
    return dirs


def sh_shade(coeffs: torch.Tensor, dirs: torch.Tensor, order: int, kind: str, want_pre: bool = False):
    """rgb [..., 3] = sigmoid_kind(eval_sh(order, coeffs.reshape(..., 3, K), normalize(dirs))) (na_sh_shade).  coeffs [..., 3 K]
    channel-major, a column slice of a wider buffer allowed; dirs [R, 3] un-normalised, one per ray of the sample-major rows
    (row n -> ray n % R; R = N: one direction per sample).  want_pre: also the [..., 3] sums in front of the activation."""
    lib = _lib.load()
    if kind not in SIGMOID:
        raise NotImplementedError(f"Unknown sigmoid kind({kind})")
    if not 0 <= order <= 4:
        raise ValueError(f"spherical-harmonic order {order} outside 0..4")
    K3 = 3 * (order + 1) ** 2
    assert coeffs.shape[-1] == K3, (coeffs.shape, order)
    c2, ld = _rows(coeffs, K3, "coeffs")
    N = c2.shape[0]
    dirs = _sh_dirs(dirs, N)
    rgb = torch.empty(tuple(coeffs.shape[:-1]) + (3,), device=coeffs.device, dtype=torch.float32)
    pre = torch.empty_like(rgb) if want_pre else None
    check(lib.na_sh_shade(_ptr(c2), ld, _ptr(dirs), N, dirs.shape[0], order, SIGMOID[kind], _ptr(rgb), _ptr(pre), _stream()))
    return (rgb, pre) if want_pre else rgb


def sh_shade_backward(g_rgb: torch.Tensor, pre: torch.Tensor, dirs: torch.Tensor, order: int, kind: str) -> torch.Tensor:
    """g_coeffs [N, 3 K] of sh_shade given g_rgb [N, 3] and the saved pre-activation sums [N, 3] (na_sh_shade_backward)."""
    lib = _lib.load()
    g_rgb, pre = _f32(g_rgb, "g_rgb"), _f32(pre, "pre")
    assert g_rgb.shape == pre.shape and g_rgb.shape[-1] == 3 and 0 <= order <= 4, (g_rgb.shape, pre.shape, order)
    N = g_rgb.numel() // 3
    dirs = _sh_dirs(dirs, N)
    out = torch.empty(N, 3 * (order + 1) ** 2, device=g_rgb.device, dtype=torch.float32)
    check(lib.na_sh_shade_backward(_ptr(g_rgb), _ptr(pre), _ptr(dirs), N, dirs.shape[0], order, SIGMOID[kind], _ptr(out), _stream()))
    return out


def _view_cols(w: torch.Tensor, width: int, name: str):
    """the view columns of a Linear's weight, as the column slice they are: (tensor, row pitch)"""
    if not w.is_cuda or w.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 CUDA(HIP) tensor")
    assert w.dim() == 2 and w.shape[1] == width, (name, w.shape, width)
    if w.stride(1) != 1 or w.stride(0) < width:
        w = w.contiguous()
    return w, w.stride(0)


def sh_view_terms(dirs: torch.Tensor, basis: torch.Tensor, scale: float, w_init: torch.Tensor, b_init: torch.Tensor,
                  w_a: torch.Tensor, b_a: torch.Tensor, w_b: torch.Tensor, b_b: torch.Tensor) -> torch.Tensor:
    """terms [3, R, hidden] (na_sh_view_terms): the per-ray part of the spherical-harmonic head's three wide Linears.  dirs [R, 3];
    basis [2, F]; w_init [hidden, 2 + 2 F] = init.weight[:, :2 + 2 F] and w_a / w_b = the view columns of the two skip Linears, all
    three passed as the column slices they are; b_*: the Linears' biases."""
    lib = _lib.load()
    dirs, basis = _f32(dirs, "dirs"), _f32(basis, "basis")
    assert dirs.dim() == 2 and dirs.shape[1] == 3 and basis.dim() == 2 and basis.shape[0] == 2, (dirs.shape, basis.shape)
    R, F = dirs.shape[0], basis.shape[1]
    hidden = w_init.shape[0]
    w_init, ld_init = _view_cols(w_init, 2 + 2 * F, "w_init")
    w_a, ld_a = _view_cols(w_a, 2 + 2 * F, "w_a")
    w_b, ld_b = _view_cols(w_b, 2 + 2 * F, "w_b")
    assert w_a.shape[0] == hidden and w_b.shape[0] == hidden and ld_a == ld_b, (w_a.shape, w_b.shape, ld_a, ld_b)
    b_init, b_a, b_b = _f32(b_init, "b_init"), _f32(b_a, "b_a"), _f32(b_b, "b_b")
    assert b_init.shape == b_a.shape == b_b.shape == (hidden,), (b_init.shape, b_a.shape, b_b.shape)
    terms = torch.empty(3, R, hidden, device=dirs.device, dtype=torch.float32)
    check(lib.na_sh_view_terms(_ptr(dirs), R, _ptr(basis), F, float(scale), _ptr(w_init), ld_init, _ptr(b_init), _ptr(w_a), _ptr(b_a),
                               _ptr(w_b), _ptr(b_b), ld_a, hidden, _ptr(terms), _stream()))
    return terms


def train_gemm_packed_ok(N: int, M: int) -> bool:
    """Does a batch of N rows with M output columns run the training GEMMs that take packed operands (na_train_gemm_packed_ok)?"""
    return bool(_lib.load().na_train_gemm_packed_ok(int(N), int(M)))


TRAIN_PATH = {0: "k_staged", 1: "ls", 2: "narrow", 3: "narrow_x1", 4: "resident"}   # include/nerf_atlas_amd.h NA_TRAIN_PATH_*


def linear_f32_path(N: int, out: int, in0: int = 0, in1: int = 0, pre_act: str = "none", packed: bool = False) -> str:
    """The kernel family linear_f32(split_bf16=True) runs this shape on (na_linear_bf16x3_path / _pk_path)."""
    lib = _lib.load()
    return TRAIN_PATH[lib.na_linear_bf16x3_pk_path(int(N), int(out), int(in0), int(in1), ACT[pre_act]) if packed
                      else lib.na_linear_bf16x3_path(int(N), int(out))]


def linear_dgrad_path(N: int, out: int, in0: int, in1: int = 0, packed: bool = False) -> str:
    """The kernel family linear_dgrad runs this shape on (na_linear_dgrad_bf16x3_path / _pk_path)."""
    lib = _lib.load()
    return TRAIN_PATH[lib.na_linear_dgrad_bf16x3_pk_path(int(N), int(out), int(in0), int(in1)) if packed
                      else lib.na_linear_dgrad_bf16x3_path(int(N), int(in0) + int(in1))]


def linear_wgrad_path(N: int, out: int, in0: int, in1: int = 0) -> str:
    """The kernel family linear_wgrad(split_bf16=True) runs this shape on (na_linear_wgrad_bf16x3_path)."""
    return TRAIN_PATH[_lib.load().na_linear_wgrad_bf16x3_path(int(N), int(out), int(in0), int(in1))]


def train_pack_many(mats):
    """ONE launch packs every B operand of a training step (na_train_pack_many).  mats: [(W [rows, cols] fp32 contiguous,
    transposed)] -- the operand is W itself (a forward's [out, in]) or, with transposed, W^T (an input gradient's [in, out], read
    straight from W).  Returns the packed operands as uint8 views of one buffer (None where the shape has no packed form)."""
    lib = _lib.load()
    n = len(mats)
    if n == 0:
        return []
    Ws = [_f32(w.detach(), "W") for w, _ in mats]
    Ms = [int(w.shape[1] if t else w.shape[0]) for (w, t) in mats]
    Ks = [int(w.shape[0] if t else w.shape[1]) for (w, t) in mats]
    sizes = [int(lib.na_train_packed_bytes(m, k)) for m, k in zip(Ms, Ks)]
    offs, total = [], 0
    for sz in sizes:
        offs.append(total)
        total += (sz + 255) & ~255
    buf = torch.empty(max(total, 16), device=Ws[0].device, dtype=torch.uint8)
    views = [buf[o:o + sz] if sz else None for o, sz in zip(offs, sizes)]
    idx = [i for i, sz in enumerate(sizes) if sz]
    if idx:
        k = len(idx)
        check(lib.na_train_pack_many(k, (C.c_void_p * k)(*[Ws[i].data_ptr() for i in idx]), (C.c_int * k)(*[Ms[i] for i in idx]),
                                     (C.c_int * k)(*[Ks[i] for i in idx]), (C.c_int * k)(*[int(Ws[i].shape[1]) for i in idx]),
                                     (C.c_int * k)(*[int(bool(mats[i][1])) for i in idx]),
                                     (C.c_void_p * k)(*[views[i].data_ptr() for i in idx]), _stream()))
    return views


def linear_dgrad(dY: torch.Tensor, W: torch.Tensor, x0: torch.Tensor, pre_act: str = "none",
                 x1: Optional[torch.Tensor] = None, want0: bool = True, want1: bool = True, packed_t: Optional[torch.Tensor] = None):
    """(g_x0 [N,in0] | None, g_x1 [N,in1] | None) = (dY . W) * act'([x0|x1]) for y = W . act([x0|x1]) + b.
    packed_t: W^T as train_pack_many left it (no transposing copy, no pack launch)."""
    lib = _lib.load()
    dY, W, x0 = _f32(dY, "dY"), _f32(W, "W"), _f32(x0, "x0")
    N, in0 = x0.shape
    in1 = 0
    if x1 is not None:
        x1 = _f32(x1, "x1")
        in1 = x1.shape[1]
    out = dY.shape[1]
    assert W.shape == (out, in0 + in1) and dY.shape[0] == N
    g0 = torch.empty_like(x0) if want0 else None
    g1 = torch.empty_like(x1) if (want1 and x1 is not None) else None
    if g0 is None and g1 is None:
        return None, None
    if packed_t is not None:
        check(lib.na_linear_dgrad_bf16x3_pk(_ptr(dY), out, N, _ptr(packed_t), _ptr(x0), in0, _ptr(x1), in1, ACT[pre_act], _ptr(g0),
                                            _ptr(g1), _stream()))
        return g0, g1
    Wt = W.t().contiguous()  # [in, out]: the K-contiguous operand of the input-gradient GEMM (<= 0.6 MB)
    check(lib.na_linear_dgrad_bf16x3(_ptr(dY), out, N, _ptr(Wt), _ptr(x0), in0, _ptr(x1), in1, ACT[pre_act], _ptr(g0), _ptr(g1),
                              _stream()))
    return g0, g1


def linear_bwd_fused_ok(N: int, out: int, in0: int) -> bool:
    """Does (N, out, in0) run the one-pass input-gradient + weight-gradient kernel (na_linear_bwd_fused_ok)?"""
    return bool(_lib.load().na_linear_bwd_fused_ok(int(N), int(out), int(in0)))


def linear_bwd_fused(dY: torch.Tensor, x0: torch.Tensor, pre_act: str, packed_t: torch.Tensor, in1: int = 0, want_bias: bool = True,
                     dW: Optional[torch.Tensor] = None, col0: int = 0):
    """(g_x [N,in0], dW, db | None) of one source x0 of y = W . act([.. x0 ..]) + b in one pass over dY and x0
    (na_linear_bwd_bf16x3_pk): in0 = 256, or a narrow source of <= 128 columns.  packed_t: W^T as train_pack_many left it.
    dW None: a fresh [out, in0 + in1] buffer whose columns 0..in0-1 are WRITTEN (in1 columns of a second source left to the caller);
    dW given: its columns col0..col0+in0-1 are written (the second source of a skip layer: col0 = the first source's width)."""
    lib = _lib.load()
    dY, x0 = _f32(dY, "dY"), _f32(x0, "x0")
    N, in0 = x0.shape
    out = dY.shape[1]
    db = None
    if dW is None:
        assert col0 == 0
        ld = in0 + in1
        nW = out * ld
        pad = (-nW) % 4
        acc = torch.empty(nW + pad + (out if want_bias else 0), device=x0.device, dtype=torch.float32)
        dW = acc[:nW].view(out, ld)
        db = acc[nW + pad:] if want_bias else None
    else:
        assert dW.is_contiguous() and dW.shape[0] == out and col0 % 64 == 0 and col0 + in0 <= dW.shape[1]
    g0 = torch.empty_like(x0)
    wp = packed_t.data_ptr() + int(lib.na_train_packed_row_offset(col0, out))
    # (the partial gradients' workspace from torch's allocator: stream-ordered reuse for microseconds; hipMallocAsync inside the
    # call cost 230 us of host time)
    ws = torch.empty(int(lib.na_linear_bwd_workspace_bytes(N, in0)), device=x0.device, dtype=torch.uint8)
    check(lib.na_linear_bwd_bf16x3_pk(_ptr(dY), out, N, wp, _ptr(x0), in0, ACT[pre_act], _ptr(g0), dW.data_ptr() + 4 * col0, dW.shape[1],
                                      _ptr(db), _ptr(ws), _stream()))
    return g0, dW, db


def linear_bwd_partials(dY: torch.Tensor, x0: torch.Tensor, pre_act: str, packed_t: torch.Tensor, col0: int = 0, want_bias: bool = True,
                        add: Optional[torch.Tensor] = None):
    """The one-pass backward of a source WITHOUT its reduction (na_linear_bwd_partials_bf16x3_pk): (g_x [N, in0], workspace holding
    the partial gradients, number of partials).  train_reduce_many sums the partials of many Linears in one launch."""
    lib = _lib.load()
    dY, x0 = _f32(dY, "dY"), _f32(x0, "x0")
    N, in0 = x0.shape
    out = dY.shape[1]
    nbytes = int(lib.na_linear_bwd_workspace_bytes(N, in0))
    ws = torch.empty(nbytes, device=x0.device, dtype=torch.uint8)
    g0 = torch.empty_like(x0)
    wp = packed_t.data_ptr() + int(lib.na_train_packed_row_offset(col0, out))
    if add is not None:  # (another consumer's gradient of x0: summed into g_x inside the kernel; narrow sources / outputs only)
        add = _f32(add, "add")
        assert add.shape == x0.shape
    check(lib.na_linear_bwd_partials_bf16x3_pk(_ptr(dY), out, N, wp, _ptr(x0), in0, ACT[pre_act], _ptr(g0), _ptr(add), int(want_bias),
                                               _ptr(ws), _stream()))
    return g0, ws, int(lib.na_linear_bwd_partial_count(N, in0))


def train_reduce_many(entries):
    """entries: [(workspace, partials, out, in, dW [out, ld] contiguous, col0, db | None)]: dW[:, col0:col0+in] and db WRITTEN, all
    entries by one launch (na_train_reduce_many)."""
    lib = _lib.load()
    n = len(entries)
    if n == 0:
        return
    vp, ip = C.c_void_p * n, C.c_int * n
    check(lib.na_train_reduce_many(
        n, vp(*[e[0].data_ptr() for e in entries]), ip(*[int(e[1]) for e in entries]), ip(*[int(e[2]) for e in entries]),
        ip(*[int(e[3]) for e in entries]), ip(*[int(e[4].shape[1]) for e in entries]),
        vp(*[e[4].data_ptr() + 4 * int(e[5]) for e in entries]), vp(*[(e[6].data_ptr() if e[6] is not None else None) for e in entries]),
        _stream()))


def adam_step(params, grads, exp_avgs, exp_avg_sqs, one_minus_beta1: float, beta2: float, one_minus_beta2: float,
              bias_correction2_sqrt: float, eps: float, neg_step_size: float, fma_mask: int):
    """torch's foreach Adam update of every tensor by ONE launch (na_adam_step): lists of contiguous fp32 device tensors."""
    optim_check("adam", params, grads, exp_avgs, exp_avg_sqs)
    lib = _lib.load()
    n = len(params)
    if n == 0:
        return
    vp, ip = C.c_void_p * n, C.c_int64 * n
    check(lib.na_adam_step(n, vp(*[t.data_ptr() for t in params]), vp(*[t.data_ptr() for t in grads]), vp(*[t.data_ptr() for t in exp_avgs]),
                           vp(*[t.data_ptr() for t in exp_avg_sqs]), ip(*[t.numel() for t in params]), float(one_minus_beta1), float(beta2),
                           float(one_minus_beta2), float(bias_correction2_sqrt), float(eps), float(neg_step_size), int(fma_mask), _stream()))


OPTIM_RULES = {"sgd": 0, "rmsprop": 1, "adam": 2, "adamw": 3}   # include/nerf_atlas_amd.h NA_OPTIM_*
_OPTIM_STATES = {"sgd": 0, "rmsprop": 1, "adam": 2, "adamw": 2}
_OPTIM_SCALARS = {"sgd": 1, "rmsprop": 4, "adam": 7, "adamw": 7}


def optim_check(rule: str, params, grads, state0=(), state1=(), known: int = 0):
    """The argument checks of optim_step (and adam_step) on their own, for a caller that must know the call will be taken before it
    changes anything: every list as long as `params` (an unused state list empty), contiguous fp32 device tensors, the shapes of a
    slot equal.  known: the first `known` lists are already known to hold contiguous fp32 device tensors (the host time of a step is
    part of its price); their shapes are still compared.  Raises ValueError."""
    if rule not in OPTIM_RULES:
        raise ValueError(f"optim_step: unknown update rule {rule!r} (one of {sorted(OPTIM_RULES)})")
    lists = (params, grads, state0, state1)[:2 + _OPTIM_STATES[rule]]
    if any(len(l) != len(params) for l in lists) or any(len(l) for l in (state0, state1)[_OPTIM_STATES[rule]:]):
        raise ValueError(f"optim_step: rule {rule!r} takes params, grads and {_OPTIM_STATES[rule]} state lists of one length")
    f32 = torch.float32
    for slot in zip(*lists):
        shape = slot[0].shape if isinstance(slot[0], torch.Tensor) else None
        for t in slot[known:]:
            if not (isinstance(t, torch.Tensor) and not t.is_sparse and t.is_cuda and t.dtype is f32 and t.is_contiguous()):
                raise ValueError("optim_step: contiguous fp32 device tensors only")
        for t in slot[1:]:
            if t.shape != shape:
                raise ValueError(f"optim_step: the tensors of a slot differ in shape ({tuple(t.shape)} vs {tuple(slot[0].shape)})")


def optim_step(rule: str, params, grads, state0, state1, scalars, fma_mask: int, checked: bool = False):
    """One optimiser step of every tensor by ONE launch per 48 non-empty tensors (na_optim_step; csrc/optim.hip): `rule` "sgd" /
    "rmsprop" / "adam" / "adamw", lists of contiguous fp32 device tensors (state0: square_avg or exp_avg, state1: exp_avg_sq; empty
    where the rule has none), the rule's scalars in the header's order as the doubles torch's Python computes.  The gradients are
    not written.  checked: optim_check has already passed on these lists."""
    if not checked:
        optim_check(rule, params, grads, state0, state1)
    lib = _lib.load()
    if len(scalars) != _OPTIM_SCALARS[rule]:
        raise ValueError(f"optim_step: rule {rule!r} takes {_OPTIM_SCALARS[rule]} scalars, got {len(scalars)}")
    n = len(params)
    if n == 0:
        return
    vp, ip, dp = C.c_void_p * n, C.c_int64 * n, C.c_double * len(scalars)
    ptrs = lambda ts: vp(*[t.data_ptr() for t in ts]) if len(ts) else None
    check(lib.na_optim_step(OPTIM_RULES[rule], n, ptrs(params), ptrs(grads), ptrs(state0), ptrs(state1), ip(*[t.numel() for t in params]),
                            dp(*[float(s) for s in scalars]), len(scalars), int(fma_mask), _stream()))


def linear_wgrad_cols(x: torch.Tensor, dY: torch.Tensor, pre_act: str, dW: torch.Tensor, col0: int):
    """dW[:, col0:col0 + x.shape[1]] = dY^T . act(x) WRITTEN (na_linear_wgrad_bf16x3_cols): one source of a concatenated input."""
    lib = _lib.load()
    x, dY = _f32(x, "x"), _f32(dY, "dY")
    N, k = x.shape
    out = dY.shape[1]
    assert dW.is_contiguous() and dW.shape[0] == out and col0 + k <= dW.shape[1]
    check(lib.na_linear_wgrad_bf16x3_cols(_ptr(x), k, N, _ptr(dY), out, ACT[pre_act], dW.data_ptr() + 4 * col0, dW.shape[1], None,
                                          _stream()))
    return dW


# ------------------------------------------------------------------------------------------------- backward
def act_backward(x: torch.Tensor, g: torch.Tensor, act: str) -> torch.Tensor:
    lib = _lib.load()
    x, g = _f32(x, "x"), _f32(g, "g")
    assert x.shape == g.shape
    out = torch.empty_like(x)
    check(lib.na_act_backward(_ptr(x), _ptr(g), x.numel(), ACT[act], _ptr(out), _stream()))
    return out


def sigmoid_backward(x: torch.Tensor, g: torch.Tensor, kind: str) -> torch.Tensor:
    lib = _lib.load()
    x, g = _f32(x, "x"), _f32(g, "g")
    out = torch.empty_like(x)
    check(lib.na_sigmoid_backward(_ptr(x), _ptr(g), x.numel(), SIGMOID[kind], _ptr(out), _stream()))
    return out


def linear_wgrad(x0: torch.Tensor, dY: torch.Tensor, pre_act: str = "none", x1: Optional[torch.Tensor] = None,
                 want_bias: bool = True, split_bf16: bool = False):
    """(dW [out, in0+in1], db [out]) for y = W . act([x0|x1]) + b; exact fp32 or the split-bf16 GEMM."""
    lib = _lib.load()
    x0, dY = _f32(x0, "x0"), _f32(dY, "dY")
    N, in0 = x0.shape
    in1 = 0
    if x1 is not None:
        x1 = _f32(x1, "x1")
        in1 = x1.shape[1]
    out = dY.shape[1]
    # (one buffer for both results: db sits behind dW, on a 16-byte boundary; the split-bf16 entry point WRITES them -- round 5:
    # no zero fill --, the exact-fp32 one accumulates)
    nW = out * (in0 + in1)
    pad = (-nW) % 4
    alloc = torch.empty if split_bf16 else torch.zeros
    acc = alloc(nW + pad + (out if want_bias else 0), device=x0.device, dtype=torch.float32)
    dW = acc[:nW].view(out, in0 + in1)
    db = acc[nW + pad:] if want_bias else None
    fn = lib.na_linear_wgrad_bf16x3_ow if split_bf16 else lib.na_linear_wgrad
    check(fn(_ptr(x0), in0, _ptr(x1), in1, N, _ptr(dY), out, ACT[pre_act], _ptr(dW), _ptr(db), _stream()))
    return dW, db


def hash_encode_backward(x: torch.Tensor, g_out: torch.Tensor, include_input: bool = True) -> torch.Tensor:
    lib = _lib.load()
    x, g_out = _f32(x, "x"), _f32(g_out, "g_out")
    N = x.numel() // 3
    tg = torch.zeros(8, 65536, 4, device=x.device, dtype=torch.float32)
    check(lib.na_hash_encode_backward(_ptr(x), N, _ptr(g_out), int(include_input), _ptr(tg), _stream()))
    return tg


def hash_encode_backward_input(x: torch.Tensor, tables: torch.Tensor, g_out: torch.Tensor,
                               include_input: bool = True) -> torch.Tensor:
    lib = _lib.load()
    x, tables, g_out = _f32(x, "x"), _f32(tables, "tables"), _f32(g_out, "g_out")
    N = x.numel() // 3
    gx = torch.empty_like(x)
    check(lib.na_hash_encode_backward_input(_ptr(x), N, _ptr(tables), _ptr(g_out), int(include_input), _ptr(gx),
                                            _stream()))
    return gx


def hash_encode_jvp(x: torch.Tensor, tables: torch.Tensor, tangent: torch.Tensor, include_input: bool = True) -> torch.Tensor:
    """d hash_encode(x)/dx . tangent, rows [tangent | per-level features] like hash_encode's output."""
    lib = _lib.load()
    x, tables, tangent = _f32(x, "x"), _f32(tables, "tables"), _f32(tangent, "tangent")
    assert tangent.shape == x.shape and x.shape[-1] == 3 and tuple(tables.shape) == (8, 65536, 4)
    N = x.numel() // 3
    out = torch.empty(tuple(x.shape[:-1]) + (32 + 3 * int(include_input),), device=x.device, dtype=torch.float32)
    check(lib.na_hash_encode_jvp(_ptr(x), N, _ptr(tables), _ptr(tangent), int(include_input), _ptr(out), _stream()))
    return out


def hash_encode_jvp_backward(x: torch.Tensor, tangent: torch.Tensor, g_t: torch.Tensor, include_input: bool = True) -> torch.Tensor:
    """d <g_t, J(x).tangent> / d tables -> [8, 65536, 4]."""
    lib = _lib.load()
    x, tangent, g_t = _f32(x, "x"), _f32(tangent, "tangent"), _f32(g_t, "g_t")
    N = x.numel() // 3
    assert g_t.numel() == N * (32 + 3 * int(include_input))
    grad = torch.zeros(8, 65536, 4, device=x.device, dtype=torch.float32)
    check(lib.na_hash_encode_jvp_backward(_ptr(x), _ptr(tangent), N, _ptr(g_t), int(include_input), _ptr(grad), _stream()))
    return grad


def ffjord_div(est: torch.Tensor, est_tangent: torch.Tensor, t: torch.Tensor, e: torch.Tensor, n_ctrl: int) -> torch.Tensor:
    """<e, d(rigid_dp)/dx . e> per point (runner.py:697-700): est / est_tangent [..., S], t [...], e [..., 3]."""
    lib = _lib.load()
    est, est_tangent, t, e = _f32(est, "est"), _f32(est_tangent, "est_tangent"), _f32(t, "t"), _f32(e, "e")
    S = est.shape[-1]
    N = est.numel() // S
    assert est_tangent.shape == est.shape and t.numel() == N and e.numel() == 3 * N
    out = torch.empty(est.shape[:-1], device=est.device, dtype=torch.float32)
    check(lib.na_ffjord_div(_ptr(est), _ptr(est_tangent), S, _ptr(t), _ptr(e), N, int(n_ctrl), _ptr(out), _stream()))
    return out


def laplace_density_backward(sdf: torch.Tensor, beta: torch.Tensor, g: torch.Tensor, want_beta: bool = True):
    """-> (g_sdf, g_beta [1] or None)."""
    lib = _lib.load()
    sdf, g = _f32(sdf, "sdf"), _f32(g, "g")
    beta = _f32(beta.reshape(1), "beta")
    g_sdf = torch.empty_like(sdf)
    g_beta = torch.zeros(1, device=sdf.device, dtype=torch.float32) if want_beta else None
    check(lib.na_laplace_density_backward(_ptr(sdf), sdf.numel(), _ptr(beta), _ptr(g), _ptr(g_sdf),
                                          _ptr(g_beta) if want_beta else None, _stream()))
    return g_sdf, g_beta


def bezier_warp_backward(est: torch.Tensor, t: torch.Tensor, n_ctrl: int, g_pts=None, g_dp=None, g_rig=None, n_rl: int = 0, g_enc=None):
    lib = _lib.load()
    est, t = _f32(est, "est"), _f32(t, "t")
    N = t.numel()
    g_pts = None if g_pts is None else _f32(g_pts, "g_pts")
    g_dp = None if g_dp is None else _f32(g_dp, "g_dp")
    g_rig = None if g_rig is None else _f32(g_rig, "g_rig")
    g_est = torch.empty_like(est)
    opt = lambda g: None if g is None else _ptr(g)
    if n_rl > 0:
        g_enc = None if g_enc is None else _f32(g_enc, "g_enc")
        assert g_enc is None or g_enc.numel() == N * n_rl
        check(lib.na_bezier_warp_latent_backward(_ptr(est), est.shape[-1], _ptr(t), N, n_ctrl, n_rl, opt(g_pts), opt(g_dp), opt(g_rig),
                                                 opt(g_enc), _ptr(g_est), _stream()))
        return g_est
    check(lib.na_bezier_warp_backward(_ptr(est), est.shape[-1], _ptr(t), N, n_ctrl, opt(g_pts), opt(g_dp), opt(g_rig), _ptr(g_est),
                                      _stream()))
    return g_est


def composite_backward(density, feat, ts, rays, g_out, softplus: bool = True, bg: str = "black", rand=None):
    lib = _lib.load()
    density, feat, ts, rays, g_out = (_f32(density, "density"), _f32(feat, "feat"), _f32(ts, "ts"), _f32(rays, "rays"),
                                      _f32(g_out, "g_out"))
    T = ts.shape[0]
    Cn = feat.shape[-1]
    R = rays.numel() // 6
    gd = torch.empty_like(density)
    gf = torch.empty_like(feat)
    if bg == "random":
        rand = _f32(rand, "rand")
        check(lib.na_composite_random_bg_backward(_ptr(density), _ptr(feat), _ptr(ts), _ptr(rays), T, R, Cn, 0 if softplus else 1,
                                                  _ptr(rand), _ptr(g_out), _ptr(gd), _ptr(gf), _stream()))
        return gd, gf
    check(lib.na_composite_backward(_ptr(density), _ptr(feat), _ptr(ts), _ptr(rays), T, R, Cn, 0 if softplus else 1, BG[bg],
                                    _ptr(g_out), _ptr(gd), _ptr(gf), _stream()))
    return gd, gf


def make_desc(in_size, enc_kind, enc_dims, latent_size, num_layers, hidden, out_size, skip, activation,
              layout="generic") -> NaMlpDesc:
    return NaMlpDesc(in_size, ENC[enc_kind], enc_dims, latent_size, num_layers, hidden, out_size, skip,
                     ACT[activation], LAYOUT[layout])


def mlp_packed_bytes(desc: NaMlpDesc, precision: str) -> int:
    return int(_lib.load().na_mlp_packed_bytes(C.byref(desc), PREC[precision]))


def mlp_pack(desc: NaMlpDesc, precision: str, weights: Sequence[torch.Tensor],
             biases: Sequence[torch.Tensor]) -> torch.Tensor:
    """weights/biases in the order init, layers[0..L-1], out (nn.Linear layout).  Returns the packed stream."""
    lib = _lib.load()
    nbytes = mlp_packed_bytes(desc, precision)
    if nbytes == 0:
        raise _lib.NaError(-3, "this SkipConnMLP shape has no MFMA kernel (use linear_f32 per layer)")
    ws = [_f32(w.detach(), "weight") for w in weights]
    bs = [_f32(b.detach(), "bias") for b in biases]
    n = desc.num_layers + 2
    assert len(ws) == n and len(bs) == n
    packed = torch.empty(nbytes, device=ws[0].device, dtype=torch.uint8)
    wp = (C.c_void_p * n)(*[w.data_ptr() for w in ws])
    bp = (C.c_void_p * n)(*[b.data_ptr() for b in bs])
    check(lib.na_mlp_pack(C.byref(desc), PREC[precision], wp, bp, _ptr(packed), _stream()))
    return packed


def _rows(t: torch.Tensor, width: int, name: str):
    """[N, width] rows of a float32 CUDA tensor WITHOUT copying when it is a column slice of a wider row-major buffer
    (unit stride along the last dim, one constant row pitch); returns (tensor, pitch in floats)."""
    if not t.is_cuda:
        raise ValueError(f"{name} must be a CUDA(HIP) tensor: the hot path has no CPU implementation")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    v = t.reshape(-1, width)  # a view whenever the strides allow it
    if v.numel() == 0 or (v.stride(1) == 1 and v.stride(0) >= width):
        return v, (v.stride(0) if v.shape[0] > 1 else max(v.stride(0), width))
    v = v.contiguous()
    return v, width


def mlp_forward(desc: NaMlpDesc, precision: str, packed: torch.Tensor, p: torch.Tensor,
                latent: Optional[torch.Tensor] = None, enc_params: Optional[torch.Tensor] = None, mip=None) -> torch.Tensor:
    """Fused SkipConnMLP forward.  p [..., in_size] and latent [..., latent_size] may be column slices of wider
    buffers (e.g. `first_out[..., 1:]`): their row pitch is passed down instead of making them contiguous.
    mip = (rays [B,H,W,6], ts [T], kind, t_end, min_deg, max_deg): the leading 6*(max_deg-min_deg) latent columns are the
    IPE of the samples, generated in the kernel's prologue; `latent` then holds only the remaining columns (or is None)."""
    lib = _lib.load()
    p2, p_ld = _rows(p, desc.in_size, "p")
    N = p2.shape[0]
    gen = 0
    mdesc = None
    if mip is not None:
        rays, ts, kind, t_end, min_deg, max_deg = mip
        rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
        assert rays.dim() == 4 and rays.shape[-1] == 6
        B, H, W = rays.shape[:3]
        gen = 6 * (max_deg - min_deg)
        mdesc = _lib.NaMipDesc(rays.data_ptr(), ts.data_ptr(), B, H, W, ts.shape[0], MIP_KIND[kind], min_deg, max_deg,
                               float(t_end))
    lat2, lat_ld = (None, 0)
    if latent is not None:
        lat2, lat_ld = _rows(latent, desc.latent_size - gen, "latent")
        assert lat2.shape[0] == N
    if enc_params is not None:
        enc_params = _f32(enc_params, "enc_params")
    y = torch.empty(tuple(p.shape[:-1]) + (desc.out_size,), device=p.device, dtype=torch.float32)
    check(lib.na_mlp_forward_mip(C.byref(desc), PREC[precision], _ptr(packed), _ptr(p2), p_ld, _ptr(lat2), lat_ld,
                                 _ptr(enc_params), None if mdesc is None else C.cast(C.byref(mdesc), C.c_void_p), N, _ptr(y),
                                 _stream()))
    return y


# ------------------------------------------------------------------------------------------------- fused renderer
def render_plain_view(rays: torch.Tensor, ts: torch.Tensor, hash_tables: torch.Tensor, packed_first: torch.Tensor,
                      packed_view: torch.Tensor, precision: str, sigmoid_kind: str = "thin", bg: str = "black",
                      want_weights: bool = False, workspace: Optional[torch.Tensor] = None,
                      pts: Optional[torch.Tensor] = None):
    """PlainNeRF(view) forward, fully fused (src/nerf.py:326-361).  rays [...,6] -> (rgb [...,3], alpha, weights).
    pts [T,...,3]: explicit sample positions (from_pts with deformed points) instead of o + t d."""
    lib = _lib.load()
    rays, ts, hash_tables = _f32(rays, "rays"), _f32(ts, "ts"), _f32(hash_tables, "hash_tables")
    R = rays.numel() // 6
    T = ts.shape[0]
    if bg not in BG:
        raise NotImplementedError(bg)
    nbytes = int(lib.na_render_workspace_bytes(T, R))
    if workspace is None:
        workspace = torch.empty(nbytes, device=rays.device, dtype=torch.uint8)
    out = torch.empty(tuple(rays.shape[:-1]) + (3,), device=rays.device, dtype=torch.float32)
    shape_t = (T,) + tuple(rays.shape[:-1])
    alpha = torch.empty(shape_t, device=rays.device, dtype=torch.float32) if want_weights else None
    weights = torch.empty(shape_t, device=rays.device, dtype=torch.float32) if want_weights else None
    if pts is not None:
        pts = _f32(pts, "pts")
        assert pts.numel() == T * R * 3, (pts.shape, T, R)
        check(lib.na_render_plain_view_pts(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(hash_tables), _ptr(packed_first),
                                           _ptr(packed_view), PREC[precision], SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha),
                                           _ptr(weights), _ptr(out), _ptr(workspace), workspace.numel(), _stream()))
        return out, alpha, weights
    check(lib.na_render_plain_view(_ptr(rays), R, _ptr(ts), T, _ptr(hash_tables), _ptr(packed_first), _ptr(packed_view),
                                   PREC[precision], SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights), _ptr(out),
                                   _ptr(workspace), workspace.numel(), _stream()))
    return out, alpha, weights


# ---- the layer-synchronous engine (csrc/render_ls.hip): what its pack and render wrappers share
# Linear shapes [out, in] ({init, layers.*, out}) of the MLPs the schedules are built for
_H = [(256, 256)]
_LS_SHAPES = {
    "first": [(256, 38), (256, 294)] + 3 * _H + [(65, 256)],
    "view": [(256, 69), (256, 325)] + 3 * _H + [(3, 256)],
    "mip_first": [(256, 134), (256, 390)] + 3 * _H + [(65, 256)],
    "mip_view": [(256, 165), (256, 421)] + 3 * _H + [(3, 256)],
    "pos": [(256, 102), (256, 358)] + 2 * _H + [(256, 358)] + _H + [(3, 256)],
    "tiny": [(256, 3), (256, 259)] + 2 * _H + [(256, 259)] + 2 * _H + [(4, 256)],
    "siren": [(256, 3), (256, 259)] + 2 * _H + [(256, 259)] + _H + [(65, 256)],
    "fourier": [(256, 259), (256, 515)] + 2 * _H + [(256, 515)] + 2 * _H + [(65, 256)],
}


def _ls_pack(what: str, symbol: str, precision: str, groups, shapes, *extra, bias_required: bool = False) -> torch.Tensor:
    """One weight stream of the layer-synchronous engine: groups = [(weights, biases)] per MLP, shapes = the Linear shapes each
    must have, extra = the entry's own integers; calls `symbol`(precision, w0, b0[, w1, b1], *extra, packed, stream)."""
    lib = _lib.load()
    keep = []
    for (ws, bs), shp in zip(groups, shapes):
        assert len(ws) == len(shp) and len(bs) == len(shp), f"{what}: {len(shp)} Linears, got {len(ws)} weights / {len(bs)} biases"
        keep += [[_f32(w.detach(), "weight") for w in ws],
                 [None if b is None and not bias_required else _f32(b.detach(), "bias") for b in bs]]
    for w, shp in zip(sum(keep[0::2], []), sum(shapes, [])):
        if tuple(w.shape) != tuple(shp):
            raise ValueError(f"{what}: weight shape {tuple(w.shape)} != {tuple(shp)}")
    nbytes = int(getattr(lib, symbol.replace("_pack", "_packed_bytes"))(PREC[precision]))
    if nbytes == 0:
        raise _lib.NaError(f"{what}: precision {precision} not supported")
    arrs = [(C.c_void_p * len(lst))(*[0 if t is None else t.data_ptr() for t in lst]) for lst in keep]
    packed = torch.empty(nbytes, device=keep[0][0].device, dtype=torch.uint8)
    check(getattr(lib, symbol)(PREC[precision], *arrs, *extra, _ptr(packed), _stream()))
    return packed


def _ls_batch(rays: torch.Tensor, T: int, pts: Optional[torch.Tensor]):
    """R, and `pts` [T, *batch, 3] checked against it"""
    R = rays.numel() // 6
    if pts is not None:
        pts = _f32(pts, "pts")
        assert pts.numel() == T * R * 3, (pts.shape, T, R)
    return R, pts


def _ls_outputs(batch, T: int, device, bg: str, want_weights: bool):
    """(out [*batch, 3], alpha, weights [T, *batch] or None) of a render entry"""
    if bg not in BG:
        raise NotImplementedError(bg)
    out = torch.empty(tuple(batch) + (3,), device=device, dtype=torch.float32)
    alpha = torch.empty((T,) + tuple(batch), device=device, dtype=torch.float32) if want_weights else None
    weights = torch.empty((T,) + tuple(batch), device=device, dtype=torch.float32) if want_weights else None
    return out, alpha, weights


def _ls_workspace(workspace: Optional[torch.Tensor], T: int, R: int, device, head: bool = False) -> torch.Tensor:
    if workspace is not None:
        return workspace
    lib = _lib.load()
    nbytes = lib.na_render_head_ls_workspace_bytes(T, R) if head else lib.na_render_ls_workspace_bytes(T, R)
    return torch.empty(int(nbytes), device=device, dtype=torch.uint8)


def render_ls_pack(precision: str, first_wb, view_wb) -> torch.Tensor:
    """Pack PlainNeRF.first and View.mlp ({init, layers.0..3, out} weights and biases each) into the weight stream of
    the layer-synchronous renderer (na_render_ls_pack)."""
    return _ls_pack("LS renderer", "na_render_ls_pack", precision, [first_wb, view_wb], [_LS_SHAPES["first"], _LS_SHAPES["view"]])


def render_plain_view_ls(rays: torch.Tensor, ts: torch.Tensor, hash_tables: torch.Tensor, packed: torch.Tensor,
                         precision: str, sigmoid_kind: str = "thin", bg: str = "black", want_weights: bool = False,
                         workspace: Optional[torch.Tensor] = None, pts: Optional[torch.Tensor] = None):
    """PlainNeRF(view) forward on the layer-synchronous engine (same contract as render_plain_view)."""
    lib = _lib.load()
    rays, ts, hash_tables = _f32(rays, "rays"), _f32(ts, "ts"), _f32(hash_tables, "hash_tables")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    workspace = _ls_workspace(workspace, T, R, rays.device)
    check(lib.na_render_plain_view_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(hash_tables), _ptr(packed),
                                      PREC[precision], SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights),
                                      _ptr(out), _ptr(workspace), workspace.numel(), _stream()))
    _f16x_guard(precision, out, "na_render_plain_view_ls")
    return out, alpha, weights


TRAIN_LS_MAX_ROWS = (1 << 22) - 1  # na_train_plain_view_ls: 32-bit byte offsets into a [N, 256] fp32 plane


def train_plain_view_ls(rays: torch.Tensor, ts: torch.Tensor, pts: torch.Tensor, hash_tables: torch.Tensor, packed: torch.Tensor,
                        sigmoid_kind: str = "thin"):
    """The training forward of PlainNeRF(view) as one launch (na_train_plain_view_ls): returns (planes [10, N, 256], view_rows [N, 69],
    density [N], rgb_pre [N, 3], out [*batch, 3]) with N = T * R, rows t * R + ray.  `packed`: render_ls_pack("bf16x3", ...) of the
    current weights."""
    lib = _lib.load()
    rays, ts, pts, hash_tables = _f32(rays, "rays"), _f32(ts, "ts"), _f32(pts, "pts"), _f32(hash_tables, "hash_tables")
    R, T = rays.numel() // 6, ts.numel()
    N = T * R
    assert pts.numel() == N * 3, (pts.shape, T, R)
    dev = rays.device
    planes = torch.empty((10, N, 256), device=dev, dtype=torch.float32)
    view_rows = torch.empty((N, 69), device=dev, dtype=torch.float32)
    density = torch.empty((N,), device=dev, dtype=torch.float32)
    rgb_pre = torch.empty((N, 3), device=dev, dtype=torch.float32)
    out = torch.empty(tuple(rays.shape[:-1]) + (3,), device=dev, dtype=torch.float32)
    workspace = _ls_workspace(None, T, R, dev)
    check(lib.na_train_plain_view_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(hash_tables), _ptr(packed), SIGMOID[sigmoid_kind],
                                     _ptr(planes), _ptr(view_rows), _ptr(density), _ptr(rgb_pre), _ptr(out), _ptr(workspace),
                                     workspace.numel(), _stream()))
    return planes, view_rows, density, rgb_pre, out


def resample_ts(ts: torch.Tensor, weights: torch.Tensor, n_fine: int, u: Optional[torch.Tensor] = None, want_fine: bool = False):
    """Inverse-cdf resampling of a coarse pass (na_resample_ts): ts [T], weights [T, *batch] -> merged [*batch, T + n_fine] (the
    coarse and the new positions of every ray in increasing order) and, with want_fine, fine [*batch, n_fine].  u: None
    (linspace(0, 1, n_fine)) or [n_fine, *batch] draws."""
    lib = _lib.load()
    ts, weights = _f32(ts, "ts"), _f32(weights, "weights")
    T = ts.shape[0]
    assert weights.shape[0] == T, (weights.shape, T)
    batch = tuple(weights.shape[1:])
    R = weights.numel() // T
    if u is not None:
        u = _f32(u, "u")
        assert tuple(u.shape) == (n_fine,) + batch, (u.shape, n_fine, batch)
    merged = torch.empty(batch + (T + n_fine,), device=ts.device, dtype=torch.float32)
    fine = torch.empty(batch + (n_fine,), device=ts.device, dtype=torch.float32) if want_fine else None
    check(lib.na_resample_ts(_ptr(ts), _ptr(weights), R, T, _ptr(u), n_fine, _ptr(fine), _ptr(merged), _stream()))
    return (merged, fine) if want_fine else merged


BG_RAYTS = {"black": 0, "white": 1, "random": 2}
RAYTS_BWD_FORM = {"auto": 0, "seq": 1, "seg": 2}


def compute_pts_rayts(rays: torch.Tensor, ts_ray: torch.Tensor) -> torch.Tensor:
    """pts[T, *batch, 3] = r_o + ts_ray[*batch, t] r_d over per-ray steps ts_ray [*batch, T] (na_compute_pts_rayts)."""
    lib = _lib.load()
    rays, ts_ray = _f32(rays, "rays"), _f32(ts_ray, "ts_ray")
    R = rays.numel() // 6
    T = ts_ray.shape[-1]
    assert tuple(ts_ray.shape[:-1]) == tuple(rays.shape[:-1]), (ts_ray.shape, rays.shape)
    pts = torch.empty((T,) + tuple(rays.shape[:-1]) + (3,), device=rays.device, dtype=torch.float32)
    check(lib.na_compute_pts_rayts(_ptr(rays), R, _ptr(ts_ray), T, _ptr(pts), _stream()))
    return pts


def _rayts_args(density, feat, ts_ray, rays, bg, rand):
    density, feat, ts_ray, rays = _f32(density, "density"), _f32(feat, "feat"), _f32(ts_ray, "ts_ray"), _f32(rays, "rays")
    T = ts_ray.shape[-1]
    Cn = feat.shape[-1]
    R = rays.numel() // 6
    assert ts_ray.numel() == R * T and density.numel() == T * R and feat.numel() == T * R * Cn, \
        (density.shape, feat.shape, ts_ray.shape, rays.shape)
    if bg not in BG_RAYTS:
        raise NotImplementedError(bg)
    if bg == "random":
        rand = _f32(rand, "rand")
        assert rand.numel() == R, (rand.shape, rays.shape)
    else:
        rand = None
    return density, feat, ts_ray, rays, rand, T, R, Cn


def composite_rayts(density: torch.Tensor, feat: torch.Tensor, ts_ray: torch.Tensor, rays: torch.Tensor, softplus: bool = True,
                    bg: str = "black", want_weights: bool = True, rand: Optional[torch.Tensor] = None):
    """`composite` over per-ray steps: density [T,...], feat [T,...,C], ts_ray [...,T] (increasing along T), rays [...,6] ->
    (out [...,C], alpha [T,...], weights [T,...]).  bg "random" takes the per-ray draw `rand` [..., 1]."""
    lib = _lib.load()
    density, feat, ts_ray, rays, rand, T, R, Cn = _rayts_args(density, feat, ts_ray, rays, bg, rand)
    out = torch.empty(tuple(rays.shape[:-1]) + (Cn,), device=rays.device, dtype=torch.float32)
    alpha = torch.empty_like(density) if want_weights else None
    weights = torch.empty_like(density) if want_weights else None
    check(lib.na_composite_rayts(_ptr(density), _ptr(feat), _ptr(ts_ray), _ptr(rays), T, R, Cn, 0 if softplus else 1, BG_RAYTS[bg],
                                 _ptr(rand), _ptr(out), _ptr(alpha), _ptr(weights), _stream()))
    return out, alpha, weights


def composite_rayts_backward(density, feat, ts_ray, rays, g_out, softplus: bool = True, bg: str = "black", rand=None, form: str = "auto"):
    """(g_density [T,...], g_feat [T,...,C]) of `composite_rayts` given g_out [...,C]; form: the decomposition over T -- "auto" (by T),
    "seq" (one thread per ray) or "seg" (16-step segments, 17 .. 256 steps)."""
    lib = _lib.load()
    density, feat, ts_ray, rays, rand, T, R, Cn = _rayts_args(density, feat, ts_ray, rays, bg, rand)
    g_out = _f32(g_out, "g_out")
    assert g_out.numel() == R * Cn, (g_out.shape, rays.shape, Cn)
    gd = torch.empty_like(density)
    gf = torch.empty_like(feat)
    check(lib.na_composite_rayts_backward_form(_ptr(density), _ptr(feat), _ptr(ts_ray), _ptr(rays), T, R, Cn, 0 if softplus else 1,
                                               BG_RAYTS[bg], _ptr(rand), _ptr(g_out), _ptr(gd), _ptr(gf), RAYTS_BWD_FORM[form], _stream()))
    return gd, gf


def render_plain_view_ls_rayts(rays: torch.Tensor, ts_ray: torch.Tensor, hash_tables: torch.Tensor, packed: torch.Tensor,
                               precision: str, sigmoid_kind: str = "thin", bg: str = "black", want_weights: bool = False,
                               workspace: Optional[torch.Tensor] = None):
    """render_plain_view_ls with per-ray steps ts_ray [*batch, T] (increasing along T)."""
    lib = _lib.load()
    rays, ts_ray, hash_tables = _f32(rays, "rays"), _f32(ts_ray, "ts_ray"), _f32(hash_tables, "hash_tables")
    R = rays.numel() // 6
    T = ts_ray.shape[-1]
    assert ts_ray.numel() == R * T, (ts_ray.shape, R)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    workspace = _ls_workspace(workspace, T, R, rays.device)
    check(lib.na_render_plain_view_ls_rayts(_ptr(rays), R, _ptr(ts_ray), T, _ptr(hash_tables), _ptr(packed), PREC[precision],
                                            SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _ptr(workspace),
                                            workspace.numel(), _stream()))
    _f16x_guard(precision, out, "na_render_plain_view_ls_rayts")
    return out, alpha, weights


def render_plain_mip_ls_pack(precision: str, first_wb, view_wb) -> torch.Tensor:
    """PlainNeRF.first and View.mlp of a mip model (96 IPE latent columns in both) as one weight stream of the
    layer-synchronous renderer (na_render_plain_mip_ls_pack; f16x only)."""
    return _ls_pack("LS mip renderer", "na_render_plain_mip_ls_pack", precision, [first_wb, view_wb],
                    [_LS_SHAPES["mip_first"], _LS_SHAPES["mip_view"]], bias_required=True)


def render_plain_mip_ls(rays: torch.Tensor, ts: torch.Tensor, hash_tables: torch.Tensor, packed: torch.Tensor, precision: str,
                        kind: str, t_end: float, min_deg: int, max_deg: int, sigmoid_kind: str = "thin", bg: str = "black",
                        want_weights: bool = False, workspace: Optional[torch.Tensor] = None):
    """PlainNeRF(view) + mip forward as one launch (rays [B,H,W,6] of whole crops; same outputs as render_plain_view_ls)."""
    lib = _lib.load()
    rays, ts, hash_tables = _f32(rays, "rays"), _f32(ts, "ts"), _f32(hash_tables, "hash_tables")
    assert rays.dim() == 4 and rays.shape[-1] == 6, rays.shape
    B, H, W = rays.shape[:3]
    R, T = B * H * W, ts.shape[0]
    out, alpha, weights = _ls_outputs((B, H, W), T, rays.device, bg, want_weights)
    workspace = _ls_workspace(workspace, T, R, rays.device)
    check(lib.na_render_plain_mip_ls(_ptr(rays), B, H, W, _ptr(ts), T, _ptr(hash_tables), _ptr(packed), PREC[precision],
                                     MIP_KIND[kind], min_deg, max_deg, float(t_end), SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha),
                                     _ptr(weights), _ptr(out), _ptr(workspace), workspace.numel(), _stream()))
    _f16x_guard(precision, out, "na_render_plain_mip_ls")
    return out, alpha, weights


def render_plain_pos_ls_pack(precision: str, first_wb, pos_wb) -> torch.Tensor:
    """PlainNeRF.first and refl.Positional.mlp ({init, layers.0..4, out}) as one weight stream of the layer-synchronous renderer
    (na_render_plain_pos_ls_pack; f16x only)."""
    return _ls_pack("LS pos renderer", "na_render_plain_pos_ls_pack", precision, [first_wb, pos_wb],
                    [_LS_SHAPES["first"], _LS_SHAPES["pos"]], bias_required=True)


def render_plain_plv_ls_pack(precision: str, first_wb, head_wb, n_rl: int = 0) -> torch.Tensor:
    """PlainNeRF.first and refl.PosLinearView ({pos.init, pos.layers.0..1, pos.out, view.init, view.layers.0..1, view.out}) as one
    weight stream (na_render_plain_plv_ls_pack; f16x only); n_rl = DynamicNeRF's refl_latent columns (0..3)."""
    n = int(n_rl)  # (0..3: the C entry refuses anything else)
    head =[(256, 102 + n), (256, 358 + n), (256, 256), (67, 256), (128, 134 + n), (128, 262 + n), (128, 128), (1, 128)]
    return _ls_pack("LS pos-linear-view renderer", "na_render_plain_plv_ls_pack", precision, [first_wb, head_wb],
                    [_LS_SHAPES["first"], head], n, bias_required=True)


def _render_head_ls(which: str, rays, ts, hash_tables, hash_tables_refl, packed, precision, sigmoid_kind, bg, want_weights, workspace,
                    pts, refl_latent=None):
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    hash_tables, hash_tables_refl = _f32(hash_tables, "hash_tables"), _f32(hash_tables_refl, "hash_tables_refl")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    workspace = _ls_workspace(workspace, T, R, rays.device, head=True)
    if which == "pos":
        assert refl_latent is None
        check(lib.na_render_plain_pos_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(hash_tables), _ptr(hash_tables_refl), _ptr(packed),
                                         PREC[precision], SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights), _ptr(out),
                                         _ptr(workspace), workspace.numel(), _stream()))
    else:
        n_rl, ld = 0, 0
        if refl_latent is not None:
            n_rl = refl_latent.shape[-1]
            refl_latent, ld = _rows(refl_latent, n_rl, "refl_latent")
            assert refl_latent.shape[0] == T * R, (refl_latent.shape, T, R)
        check(lib.na_render_plain_plv_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(hash_tables), _ptr(hash_tables_refl),
                                         _ptr(refl_latent), ld, n_rl, _ptr(packed), PREC[precision], SIGMOID[sigmoid_kind], BG[bg],
                                         _ptr(alpha), _ptr(weights), _ptr(out), _ptr(workspace), workspace.numel(), _stream()))
    _f16x_guard(precision, out, f"na_render_plain_{which}_ls")
    return out, alpha, weights


def render_plain_pos_ls(rays, ts, hash_tables, hash_tables_refl, packed, precision: str, sigmoid_kind: str = "thin", bg: str = "black",
                        want_weights: bool = False, workspace: Optional[torch.Tensor] = None, pts: Optional[torch.Tensor] = None):
    """PlainNeRF + refl.Positional (`--refl-kind pos`) forward as one launch; same contract as render_plain_view_ls."""
    return _render_head_ls("pos", rays, ts, hash_tables, hash_tables_refl, packed, precision, sigmoid_kind, bg, want_weights, workspace, pts)


def render_plain_plv_ls(rays, ts, hash_tables, hash_tables_refl, packed, precision: str, sigmoid_kind: str = "thin", bg: str = "black",
                        want_weights: bool = False, workspace: Optional[torch.Tensor] = None, pts: Optional[torch.Tensor] = None,
                        refl_latent: Optional[torch.Tensor] = None):
    """PlainNeRF + refl.PosLinearView (`--refl-kind pos-linear-view`) forward as one launch; refl_latent [T, ..., n <= 3] =
    DynamicNeRF's per-sample reflectance latent (rows may be a column slice: passed by pitch)."""
    return _render_head_ls("plv", rays, ts, hash_tables, hash_tables_refl, packed, precision, sigmoid_kind, bg, want_weights, workspace, pts,
                           refl_latent)


def mlp_hash_ls_pack(precision: str, weights, biases) -> torch.Tensor:
    """Pack a hash-encoded SkipConnMLP (in 3, HashEncoder, 5 x 256, skip 3: {init, layers.0..4, out}) into the weight stream of the
    layer-synchronous engine (D-NeRF's deformation network): "f16x" (out <= 32) or, round 6, "bf16x3" (the three-product split, out <= 64)."""
    n_out = int(weights[-1].shape[0])  # (f16x: <= 32 rows, bf16x3: <= 64: the C entry refuses anything else)
    shapes = [(256, 38), (256, 294)] + 2 * _H + [(256, 294)] + _H + [(n_out, 256)]
    return _ls_pack("LS hash MLP", "na_mlp_hash_ls_pack", precision, [(weights, biases)], [shapes], n_out)


def mlp_hash_ls(rays: torch.Tensor, ts: torch.Tensor, tables: torch.Tensor, packed: torch.Tensor, precision: str, n_out: int,
                pts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The packed hash-encoded MLP at the samples of rays [..., 6] x ts [T] (or explicit pts [T, ..., 3]) -> [T, ..., n_out]."""
    lib = _lib.load()
    rays, ts, tables = _f32(rays, "rays"), _f32(ts, "ts"), _f32(tables, "tables")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    y = torch.empty((T,) + tuple(rays.shape[:-1]) + (n_out,), device=rays.device, dtype=torch.float32)
    check(lib.na_mlp_hash_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(tables), _ptr(packed), PREC[precision], n_out, _ptr(y),
                             n_out, _stream()))
    _f16x_guard(precision, y, "na_mlp_hash_ls")
    return y


def mlp_fourier_ls_pack(precision: str, weights, biases) -> torch.Tensor:
    """Pack a Fourier-encoded SkipConnMLP (in 3, 128 frequencies, 6 x 256, skip 3, out 65: {init, layers.0..5, out}) into the weight
    stream of the layer-synchronous engine (f16x only; VolSDF's MLP SDF network)."""
    return _ls_pack("LS Fourier MLP", "na_mlp_fourier_ls_pack", precision, [(weights, biases)], [_LS_SHAPES["fourier"]])


def mlp_fourier_ls(rays: torch.Tensor, ts: torch.Tensor, basis: torch.Tensor, packed: torch.Tensor, precision: str,
                   pts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The packed Fourier-encoded MLP at the samples of rays [..., 6] x ts [T] (or explicit pts [T, ..., 3]) -> [T, ..., 65];
    basis [3, 128] (FourierEncoder.basis x extra_scale)."""
    lib = _lib.load()
    rays, ts, basis = _f32(rays, "rays"), _f32(ts, "ts"), _f32(basis, "basis")
    assert tuple(basis.shape) == (3, 128), basis.shape
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    y = torch.empty((T,) + tuple(rays.shape[:-1]) + (65,), device=rays.device, dtype=torch.float32)
    check(lib.na_mlp_fourier_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(basis), _ptr(packed), PREC[precision], _ptr(y), 65,
                                _stream()))
    _f16x_guard(precision, y, "na_mlp_fourier_ls")
    return y


AE_SIZES = ((16, 32, 64), (32, 64))  # (encoding sizes, intermediate sizes) na_ae_front is instantiated for


def ae_front_supported(E: int, I: int) -> bool:
    return E in AE_SIZES[0] and I in AE_SIZES[1]


def ae_front_pack(precision: str, E: int, I: int, enc_wb, den_wb) -> torch.Tensor:
    """Pack NeRFAE's two narrow SkipConnMLPs -- encode (Fourier, 5 x 128, out E) and density_tform (5 x 64, out 1 + I), each
    ({init, layers.0..4, out} weights, biases) -- into the weight stream of na_ae_front."""
    lib = _lib.load()
    (w1, b1), (w2, b2) = enc_wb, den_wb
    assert len(w1) == 7 and len(b1) == 7 and len(w2) == 7 and len(b2) == 7
    w1 = [_f32(w.detach(), "weight") for w in w1]
    w2 = [_f32(w.detach(), "weight") for w in w2]
    b1 = [None if b is None else _f32(b.detach(), "bias") for b in b1]
    b2 = [None if b is None else _f32(b.detach(), "bias") for b in b2]
    shapes = [(128, 259), (128, 387), (128, 128), (128, 128), (128, 387), (128, 128), (E, 128),
              (64, E), (64, 64 + E), (64, 64), (64, 64), (64, 64 + E), (64, 64), (1 + I, 64)]
    for w, shp in zip(w1 + w2, shapes):
        if tuple(w.shape) != shp:
            raise ValueError(f"NeRFAE front: weight shape {tuple(w.shape)} != {shp}")
    nbytes = int(lib.na_ae_front_packed_bytes(PREC[precision], E, I))
    if nbytes == 0:
        raise _lib.NaError(f"NeRFAE front: precision {precision} / E {E} / I {I} not supported")
    ptrs = lambda ts: (C.c_void_p * 7)(*[0 if t is None else t.data_ptr() for t in ts])
    packed = torch.empty(nbytes, device=w1[0].device, dtype=torch.uint8)
    check(lib.na_ae_front_pack(PREC[precision], E, I, ptrs(w1), ptrs(b1), ptrs(w2), ptrs(b2), _ptr(packed), _stream()))
    return packed


def ae_front(rays: torch.Tensor, ts: torch.Tensor, basis: torch.Tensor, packed: torch.Tensor, precision: str, E: int, I: int,
             normalize: bool = False, pts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """NeRFAE's front in one launch at the samples of rays [..., 6] x ts [T] (or explicit pts [T, ..., 3]) -> rows [T, ..., 1 + E + I] =
    [density logit | encoded (normalised if asked) | first_out[1:]]: with E + I = 64 what `render_view_ls(beta=None)` takes as feat.
    basis [3, 128] (FourierEncoder.basis x extra_scale)."""
    lib = _lib.load()
    rays, ts, basis = _f32(rays, "rays"), _f32(ts, "ts"), _f32(basis, "basis")
    assert tuple(basis.shape) == (3, 128), basis.shape
    T = ts.shape[0]
    R = rays.numel() // 6
    if pts is not None:
        pts = _f32(pts, "pts")
        assert pts.numel() == T * R * 3, (pts.shape, T, R)
    ld = 1 + E + I
    y = torch.empty((T,) + tuple(rays.shape[:-1]) + (ld,), device=rays.device, dtype=torch.float32)
    check(lib.na_ae_front(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(basis), _ptr(packed), PREC[precision], E, I, int(bool(normalize)),
                          _ptr(y), ld, _stream()))
    return y


def row_normalize(x: torch.Tensor) -> torch.Tensor:
    """F.normalize(x, dim=-1) for rows of width <= 64 (column slices go down with their pitch)."""
    lib = _lib.load()
    W = x.shape[-1]
    x2, ld = _rows(x, W, "x")
    y = torch.empty(x2.shape, device=x.device, dtype=torch.float32)
    check(lib.na_row_normalize(_ptr(x2), ld, x2.shape[0], W, _ptr(y), W, _stream()))
    return y.reshape(x.shape)


def row_normalize_backward(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    W = x.shape[-1]
    x2, ld = _rows(x, W, "x")
    g2, gld = _rows(g, W, "g")
    gx = torch.empty(x2.shape, device=x.device, dtype=torch.float32)
    check(lib.na_row_normalize_backward(_ptr(x2), ld, _ptr(g2), gld, x2.shape[0], W, _ptr(gx), W, _stream()))
    return gx.reshape(x.shape)


def row_sqnorm_mean(x: torch.Tensor) -> torch.Tensor:
    """torch.linalg.norm(x, dim=-1).square().mean() -> 0-dim tensor (fixed-point reduction in the deterministic mode)."""
    lib = _lib.load()
    W = x.shape[-1]
    x2, ld = _rows(x, W, "x")
    out = torch.zeros(1, device=x.device, dtype=torch.float32)
    check(lib.na_row_sqnorm_mean(_ptr(x2), ld, x2.shape[0], W, _ptr(out), _stream()))
    return out.reshape(())


def row_sqnorm_mean_backward(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    W = x.shape[-1]
    x2, ld = _rows(x, W, "x")
    g = _f32(g.reshape(1), "g")
    gx = torch.empty(x2.shape, device=x.device, dtype=torch.float32)
    check(lib.na_row_sqnorm_mean_backward(_ptr(x2), ld, _ptr(g), x2.shape[0], W, _ptr(gx), W, _stream()))
    return gx.reshape(x.shape)


def render_tiny_ls_pack(precision: str, weights, biases) -> torch.Tensor:
    """Pack TinyNeRF.estim ({init, layers.0..5, out}) into the weight stream of the layer-synchronous renderer."""
    return _ls_pack("LS TinyNeRF renderer", "na_render_tiny_ls_pack", precision, [(weights, biases)], [_LS_SHAPES["tiny"]])


def render_tiny_ls(rays: torch.Tensor, ts: torch.Tensor, packed: torch.Tensor, precision: str, sigmoid_kind: str = "thin",
                   bg: str = "black", want_weights: bool = False, pts: Optional[torch.Tensor] = None):
    """TinyNeRF forward in one kernel (layer-synchronous engine): rays [..., 6], ts [T] -> (rgb [..., 3], alpha, weights)."""
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    check(lib.na_render_tiny_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(packed), PREC[precision], SIGMOID[sigmoid_kind],
                                BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _stream()))
    _f16x_guard(precision, out, "na_render_tiny_ls")
    return out, alpha, weights


def render_view_ls_pack(precision: str, weights, biases) -> torch.Tensor:
    """Pack refl.View's MLP ({init, layers.0..3, out}; 5 + 64 inputs) into the weight stream of na_render_view_ls."""
    return _ls_pack("LS View renderer", "na_render_view_ls_pack", precision, [(weights, biases)], [_LS_SHAPES["view"]])


def render_view_ls(rays: torch.Tensor, ts: torch.Tensor, feat: torch.Tensor, beta: torch.Tensor, packed: torch.Tensor,
                   precision: str, sigmoid_kind: str = "thin", bg: str = "black", want_weights: bool = False,
                   pts: Optional[torch.Tensor] = None):
    """View head + compositing in one kernel.  feat [T, *rays.shape[:-1], >= 65]: column 0 signed distance, 1..64 latent
    (the SDF network's output, rows may be wider); beta: the Laplace scale (0-dim or 1-element device tensor), or None: column 0
    is a density logit, sigma = softplus(column 0 - 1) (NeRFAE's rows from `ae_front`)."""
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    feat, ld = _rows(feat, feat.shape[-1], "feat")
    assert feat.shape[0] == T * R and ld >= 65, (feat.shape, T, R, ld)
    beta = None if beta is None else _f32(beta.reshape(1), "beta")
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    workspace = _ls_workspace(None, T, R, rays.device)
    check(lib.na_render_view_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(feat), ld, _ptr(beta), _ptr(packed), PREC[precision],
                                SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _ptr(workspace),
                                workspace.numel(), _stream()))
    _f16x_guard(precision, out, "na_render_view_ls")
    return out, alpha, weights


def render_volsdf_siren_ls_pack(precision: str, sdf_wb, view_wb) -> torch.Tensor:
    """Pack the SIREN SDF network (7 Linears) and refl.View's MLP (6) into the stream of na_render_volsdf_siren_ls."""
    return _ls_pack("LS SIREN-VolSDF renderer", "na_render_volsdf_siren_ls_pack", precision, [sdf_wb, view_wb],
                    [_LS_SHAPES["siren"], _LS_SHAPES["view"]])


def render_volsdf_siren_ls(rays: torch.Tensor, ts: torch.Tensor, beta: torch.Tensor, packed: torch.Tensor, precision: str,
                           sigmoid_kind: str = "thin", bg: str = "black", want_weights: bool = False,
                           pts: Optional[torch.Tensor] = None):
    """VolSDF (SIREN SDF network + View head) forward in one kernel: rays [..., 6], ts [T] -> (rgb, alpha, weights)."""
    lib = _lib.load()
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    beta = _f32(beta.reshape(1), "beta")
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    workspace = _ls_workspace(None, T, R, rays.device)
    check(lib.na_render_volsdf_siren_ls(_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(beta), _ptr(packed), PREC[precision],
                                        SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _ptr(workspace),
                                        workspace.numel(), _stream()))
    _f16x_guard(precision, out, "na_render_volsdf_siren_ls")
    return out, alpha, weights


# ------------------------------------------------------------------------------------------------- forward-mode tangents
def act_deriv(x: torch.Tensor, act: str, order: int = 1) -> torch.Tensor:
    lib = _lib.load()
    x = _f32(x, "x")
    out = torch.empty_like(x)
    check(lib.na_act_deriv(_ptr(x), x.numel(), ACT[act], order, _ptr(out), _stream()))
    return out


def mul_bcast(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [n...] shared by the J leading rows of b [J, n...]."""
    lib = _lib.load()
    a, b = _f32(a, "a"), _f32(b, "b")
    J = b.shape[0]
    assert b.numel() == J * a.numel(), (a.shape, b.shape)
    out = torch.empty_like(b)
    check(lib.na_mul_bcast(_ptr(a), _ptr(b), a.numel(), J, _ptr(out), _stream()))
    return out


def mul_reduce(g: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    g, b = _f32(g, "g"), _f32(b, "b")
    J = b.shape[0]
    out = torch.empty(b.shape[1:], device=b.device, dtype=torch.float32)
    check(lib.na_mul_reduce(_ptr(g), _ptr(b), out.numel(), J, _ptr(out), _stream()))
    return out


def eikonal_loss(normals: torch.Tensor) -> torch.Tensor:
    """normals [3, N] (tangent-major) -> scalar mean((|n| - 1)^2)."""
    lib = _lib.load()
    normals = _f32(normals, "normals")
    loss = torch.zeros(1, device=normals.device, dtype=torch.float32)
    check(lib.na_eikonal_loss(_ptr(normals), normals.shape[1], _ptr(loss), _stream()))
    return loss.reshape(())


def eikonal_loss_backward(normals: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    normals, g = _f32(normals, "normals"), _f32(g.reshape(1), "g")
    out = torch.empty_like(normals)
    check(lib.na_eikonal_loss_backward(_ptr(normals), normals.shape[1], _ptr(g), _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------- NeRFVoxel (csrc/voxel.hip, voxel_fine.hip)
# One section for the three colour heads of a voxel model: "rgb" (rows of C colour parameters), "plv" (pos-linear-view, rows [raw rgb |
# (order+1)^2 coefficients]) and "sh" (spherical-harmonic colour, rows of 3 (order+1)^2 coefficients).  `_voxel_head` is the one place a
# head is recognised; one implementation per operator takes the head's name, and the public voxel_* / voxel_plv_* / voxel_sh_* functions
# are its three spellings.
PLV_CHANNELS = {3 + (k + 1) ** 2: k for k in range(5)}   # C = 3 + (order + 1)^2 -> order
VOX_HEAD = {"rgb": 0, "plv": 1, "sh": 2, "density": 3}   # include/nerf_atlas_amd.h NA_VOX_HEAD_*
VOXEL_FINE_LANES = (4, 8, 16, 32, 64)                    # lanes per ray na_voxel_fine_lanes is instantiated for
VOXEL_SPARSE_LANES = 16      # lanes per ray of the shipped sparse renderer
VOXEL_DEAD_DENSITY = -1e30   # what a dead sample's density column is masked to: finite, and fast_softplus(-1e30 - 1) is 0


def _voxel_even(S: int):
    """an odd resolution makes the reference's ids `floor + x.5` truncated"""
    if S % 2 != 0 or S < 2:
        raise ValueError(f"voxel resolution {S}: even resolutions only (the reference's ids are floor(.) + S / 2)")


def _aligned16(t: torch.Tensor) -> torch.Tensor:
    """the kernels read and write [density | 3 colours] rows as one 16-byte access: a contiguous view at an odd storage offset is copied"""
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _voxel_head(kind: str, densities: torch.Tensor, rgb: torch.Tensor, order: Optional[int] = None):
    """(densities, rgb, S, C, order) of densities [S,S,S,1] and rgb [S,S,S,C] under the head `kind`.  "rgb": any C (the library refuses a
    count without a kernel), order -1.  "plv": C = 3 + (order+1)^2 names the order.  "sh": C does not identify the head (3 is the RGB
    head's, 12 the pos-linear-view head's at order 2), so the order is explicit and checked against C.  The two view-dependent heads read
    rows 16 bytes at a time where they are aligned: their grid is returned 16-byte aligned."""
    if kind not in ("rgb", "plv", "sh"):
        raise ValueError(f"voxel head {kind!r} (rgb, plv, sh)")
    if kind == "sh":
        _voxel_order(order)
    densities, rgb = _f32(densities, "densities"), _f32(rgb, "rgb")
    S = densities.shape[0]
    if densities.dim() != 4 or tuple(densities.shape) != (S, S, S, 1) or rgb.dim() != 4 or tuple(rgb.shape[:3]) != (S, S, S):
        raise ValueError(f"voxel grids must be densities [S,S,S,1] and rgb [S,S,S,C], got {tuple(densities.shape)} and {tuple(rgb.shape)}")
    _voxel_even(S)
    Cn = rgb.shape[-1]
    if kind == "rgb":
        return densities, rgb, S, Cn, -1
    if kind == "plv":
        if Cn not in PLV_CHANNELS:
            raise ValueError(f"rgb has {Cn} channels: the pos-linear-view voxel head holds 3 + (order + 1)^2 = {sorted(PLV_CHANNELS)}")
        order = PLV_CHANNELS[Cn]
    elif Cn != 3 * (order + 1) ** 2:
        raise ValueError(f"rgb has {Cn} channels: the spherical-harmonic voxel head of order {order} holds 3 (order + 1)^2 = {3 * (order + 1) ** 2}")
    return densities, _aligned16(rgb), S, Cn, order


def _voxel_abi(kind: str, Cn: int, order: int):
    """(the head's entry points by operator, the arguments that name the head behind S in their parameter lists)"""
    lib = _lib.load()
    if kind == "rgb":
        return dict(sample=lib.na_voxel_sample, backward=lib.na_voxel_sample_backward, backward_pts=lib.na_voxel_sample_backward_pts,
                    render=lib.na_voxel_render, render_rayts=lib.na_voxel_render_rayts, dyn_render=lib.na_dyn_voxel_render), (Cn,)
    if kind == "plv":
        return dict(sample=lib.na_voxel_plv_sample, backward=lib.na_voxel_plv_sample_backward,
                    backward_variant=lib.na_voxel_plv_sample_backward_variant, backward_pts=lib.na_voxel_plv_sample_backward_pts,
                    render=lib.na_voxel_plv_render, render_rayts=lib.na_voxel_plv_render_rayts, dyn_render=lib.na_dyn_voxel_plv_render), (order,)
    return dict(sample=lib.na_voxel_sh_sample, backward=lib.na_voxel_sh_sample_backward,
                backward_variant=lib.na_voxel_sh_sample_backward_variant, backward_pts=lib.na_voxel_sh_sample_backward_pts,
                render=lib.na_voxel_sh_render, render_rayts=lib.na_voxel_sh_render_rayts, dyn_render=lib.na_dyn_voxel_sh_render), (Cn, order)


def _voxel_order(order) -> int:
    if isinstance(order, bool) or not isinstance(order, int) or order not in range(5):
        raise ValueError(f"order {order!r} outside 0..4")
    return order


def _voxel_positions(kind: str, pts, rays, ts):
    """(pts or None, rays or None, ts or None, R, T, batch shape of the samples).  The RGB head reads no ray: explicit pts [..., 3] are one
    row of samples (T = 1), else rays [..., 6] x ts [T].  The view-dependent heads always take rays [..., 6], with explicit pts
    [T, *rays.shape[:-1], 3] (any T) or ts [T]; the ray of sample n is n % R."""
    if kind == "rgb" and pts is not None:
        pts = _f32(pts, "pts")
        if pts.shape[-1] != 3:
            raise ValueError(f"pts must be [..., 3], got {tuple(pts.shape)}")
        return pts, None, None, pts.numel() // 3, 1, tuple(pts.shape[:-1])
    if rays is None or (pts is None and ts is None):
        raise ValueError("voxel lookup needs explicit pts, or rays and ts")
    rays = _f32(rays, "rays")
    if rays.shape[-1] != 6:
        raise ValueError(f"rays must be [..., 6], got {tuple(rays.shape)}")
    R = rays.numel() // 6
    if pts is not None:
        pts = _f32(pts, "pts")
        if pts.shape[-1] != 3 or R == 0 or (pts.numel() // 3) % R != 0:
            raise ValueError(f"pts must be [T, ..., 3] over the {R} rays, got {tuple(pts.shape)}")
        return pts, rays, None, R, pts.numel() // 3 // R, tuple(pts.shape[:-1])
    ts = _f32(ts, "ts")
    if ts.dim() != 1:
        raise ValueError(f"rays must be [..., 6] and ts [T], got {tuple(rays.shape)} and {tuple(ts.shape)}")
    return None, rays, ts, R, ts.shape[0], (ts.shape[0],) + tuple(rays.shape[:-1])


def _voxel_g_raw(kind: str, g_raw, g_sh, n: int, Cn: int):
    """the lookup's output gradients, one row per sample: g_raw [..., 1 + C] (RGB head) or [..., 4], 16-byte aligned; g_sh [...] (plv)"""
    g_raw = _f32(g_raw, "g_raw")
    if kind == "rgb":
        if Cn < 1 or g_raw.shape[-1] != 1 + Cn or g_raw.numel() != n * (1 + Cn):
            raise ValueError(f"g_raw must be [..., {1 + Cn}] with one row per sample ({n}), got {tuple(g_raw.shape)}")
    elif kind == "sh":
        if g_raw.numel() != n * 4:
            raise ValueError(f"g_raw must be [..., 4] with one row per sample ({n}), got {tuple(g_raw.shape)}")
    else:
        g_sh = _f32(g_sh, "g_sh")
        if g_raw.numel() != n * 4 or g_sh.numel() != n:
            raise ValueError(f"g_raw must be [..., 4] and g_sh [...] with one row per sample ({n}), got {tuple(g_raw.shape)} and {tuple(g_sh.shape)}")
    return _aligned16(g_raw), g_sh


def _voxel_sample(kind, densities, rgb, grid_radius, pts, rays, ts, order=None):
    densities, rgb, S, Cn, order = _voxel_head(kind, densities, rgb, order)
    pts, rays, ts, R, T, batch = _voxel_positions(kind, pts, rays, ts)
    fn, head = _voxel_abi(kind, Cn, order)
    raw = torch.empty(batch + (1 + Cn if kind == "rgb" else 4,), device=densities.device, dtype=torch.float32)
    sh = torch.empty(batch, device=densities.device, dtype=torch.float32) if kind == "plv" else None
    check(fn["sample"](_ptr(pts), _ptr(rays), R, _ptr(ts), T, _ptr(densities), _ptr(rgb), S, *head, float(grid_radius),
                                                  _ptr(raw), *((_ptr(sh),) if kind == "plv" else ()), _stream()))
    return (raw, sh) if kind == "plv" else raw


def _voxel_sample_backward(kind, g_raw, g_sh, S, order, grid_radius, pts, rays, ts, variant=None):
    g_raw = _f32(g_raw, "g_raw")
    _voxel_even(S)
    Cn = g_raw.shape[-1] - 1 if kind == "rgb" else 3 + (_voxel_order(order) + 1) ** 2 if kind == "plv" else 3 * (_voxel_order(order) + 1) ** 2
    pts, rays, ts, R, T, _ = _voxel_positions(kind, pts, rays, ts)
    g_raw, g_sh = _voxel_g_raw(kind, g_raw, g_sh, T * R, Cn)
    if kind != "rgb":  # (the RGB head's 4 sums per voxel stay inside the default workspace up to S = 80 and it never asked for more)
        config.require_deterministic_workspace(8 * S ** 3 * (1 + Cn))  # (a no-op outside config.set_deterministic's mode)
    g_den = torch.zeros(S, S, S, 1, device=g_raw.device, dtype=torch.float32)
    g_rgb = torch.zeros(S, S, S, Cn, device=g_raw.device, dtype=torch.float32)
    fn, head = _voxel_abi(kind, Cn, order)
    args = (_ptr(pts), _ptr(rays), R, _ptr(ts), T, _ptr(g_raw), *((_ptr(g_sh),) if kind == "plv" else ()), S, *head, float(grid_radius),
            _ptr(g_den), _ptr(g_rgb))
    if variant is None:
        check(fn["backward"](*args, _stream()))
    else:
        check(fn["backward_variant"](*args, int(variant), _stream()))
    return g_den, g_rgb


def _voxel_sample_backward_pts(kind, g_raw, g_sh, pts, rays, densities, rgb, grid_radius, order=None):
    densities, rgb, S, Cn, order = _voxel_head(kind, densities, rgb, order)
    pts, rays, _, R, T, _ = _voxel_positions(kind, pts, rays, None)
    g_raw, g_sh = _voxel_g_raw(kind, g_raw, g_sh, T * R, Cn)
    g_pts = torch.empty(pts.shape, device=pts.device, dtype=torch.float32)
    fn, head = _voxel_abi(kind, Cn, order)
    rays_of = () if kind == "rgb" else (_ptr(rays), R)  # (the RGB head's entry point takes no rays)
    check(fn["backward_pts"](_ptr(pts), *rays_of, T * R, _ptr(densities), _ptr(rgb), _ptr(g_raw), *((_ptr(g_sh),) if kind == "plv" else ()), S,
                             *head, float(grid_radius), _ptr(g_pts), _stream()))
    return g_pts


def _voxel_render(kind, rays, ts, densities, rgb, grid_radius, order, sigmoid_kind, bg, want_weights, pts=None):
    """the one-launch renderer over the shared row ts [T], at o + t d or at explicit pts [T, ..., 3]"""
    densities, rgb, S, Cn, order = _voxel_head(kind, densities, rgb, order)
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    T = ts.shape[0]
    R, pts = _ls_batch(rays, T, pts)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], T, rays.device, bg, want_weights)
    fn, head = _voxel_abi(kind, Cn, order)
    check(fn["render"](_ptr(rays), _ptr(pts), R, _ptr(ts), T, _ptr(densities), _ptr(rgb), S, *head, float(grid_radius), SIGMOID[sigmoid_kind],
                       BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _stream()))
    return out, alpha, weights


def _voxel_render_rayts(kind, rays, ts_ray, densities, rgb, grid_radius, order, sigmoid_kind, bg, want_weights):
    """the one-launch renderer over per-ray rows ts_ray [*batch, M] of rays [*batch, 6]"""
    densities, rgb, S, Cn, order = _voxel_head(kind, densities, rgb, order)
    rays, ts_ray = _f32(rays, "rays"), _f32(ts_ray, "ts_ray")
    assert rays.shape[-1] == 6 and ts_ray.dim() >= 1 and tuple(ts_ray.shape[:-1]) == tuple(rays.shape[:-1]), (ts_ray.shape, rays.shape)
    R, M = rays.numel() // 6, ts_ray.shape[-1]
    out, alpha, weights = _ls_outputs(rays.shape[:-1], M, rays.device, bg, want_weights)
    fn, head = _voxel_abi(kind, Cn, order)
    check(fn["render_rayts"](_ptr(rays), R, _ptr(ts_ray), M, _ptr(densities), _ptr(rgb), S, *head, float(grid_radius), SIGMOID[sigmoid_kind],
                             BG[bg], _ptr(alpha), _ptr(weights), _ptr(out), _stream()))
    return out, alpha, weights


def voxel_sample(densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float, pts: Optional[torch.Tensor] = None,
                 rays: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """raw [..., 1 + C] = [density | C colour parameters] of the reference's 8-neighbour lookup (src/nerf.py:493-524) at explicit
    pts [..., 3], or at o + t d of rays [..., 6] x ts [T] formed in the kernel ([T, ..., 1 + C])."""
    return _voxel_sample("rgb", densities, rgb, grid_radius, pts, rays, ts)


def voxel_sample_backward(g_raw: torch.Tensor, S: int, grid_radius: float, pts: Optional[torch.Tensor] = None,
                          rays: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None):
    """(g_densities [S,S,S,1], g_rgb [S,S,S,C]) of voxel_sample given g_raw [..., 1 + C] and the same positions."""
    return _voxel_sample_backward("rgb", g_raw, None, S, -1, grid_radius, pts, rays, ts)


def voxel_sample_backward_pts(g_raw: torch.Tensor, pts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor,
                              grid_radius: float) -> torch.Tensor:
    """g_pts [..., 3]: the gradient of voxel_sample w.r.t. explicit pts [..., 3] given g_raw [..., 1 + C] (a gather: one launch, no atomics)"""
    return _voxel_sample_backward_pts("rgb", g_raw, None, pts, None, densities, rgb, grid_radius)


def voxel_render(rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float,
                 sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True, pts: Optional[torch.Tensor] = None):
    """NeRFVoxel's eval route as ONE launch: positions (o + t d, or explicit pts [T, ..., 3]) -> lookup -> activation -> compositing.
    (out [..., C], alpha [T, ...], weights [T, ...]); bg black | white (random: composite against black, then sky_random)."""
    return _voxel_render("rgb", rays, ts, densities, rgb, grid_radius, None, sigmoid_kind, bg, want_weights, pts=pts)


def voxel_plv_sample(densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float, rays: torch.Tensor,
                     pts: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None):
    """(raw [..., 4] = [density | 3 colour parameters], sh [...] = sum_k Y_k(normalize(rays[..., 3:])) c_k) of NeRFVoxel's lookup with
    the pos-linear-view head, at explicit pts [T, *rays.shape[:-1], 3] or at o + t d of rays x ts [T]."""
    return _voxel_sample("plv", densities, rgb, grid_radius, pts, rays, ts)


def voxel_plv_sample_backward(g_raw: torch.Tensor, g_sh: torch.Tensor, S: int, order: int, grid_radius: float, rays: torch.Tensor,
                              pts: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None, variant: Optional[int] = None):
    """(g_densities [S,S,S,1], g_rgb [S,S,S, 3 + (order+1)^2]) of voxel_plv_sample given g_raw [..., 4], g_sh [...] and the same
    positions.  variant: scatter variant 1 or 2 (measurements); None runs the shipped one."""
    return _voxel_sample_backward("plv", g_raw, g_sh, S, order, grid_radius, pts, rays, ts, variant)


def voxel_plv_sample_backward_pts(g_raw: torch.Tensor, g_sh: torch.Tensor, pts: torch.Tensor, rays: torch.Tensor, densities: torch.Tensor,
                                  rgb: torch.Tensor, grid_radius: float) -> torch.Tensor:
    """g_pts [..., 3]: the gradient of voxel_plv_sample w.r.t. explicit pts given g_raw [..., 4] and g_sh [...] (a gather, no atomics)"""
    return _voxel_sample_backward_pts("plv", g_raw, g_sh, pts, rays, densities, rgb, grid_radius)


def voxel_plv_render(rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float,
                     sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True, pts: Optional[torch.Tensor] = None):
    """NeRFVoxel's eval route with the pos-linear-view head as ONE launch: basis per ray, positions (o + t d, or explicit pts
    [T, ..., 3]) -> lookup -> activation x linear scale -> compositing.  Outputs and backgrounds of voxel_render."""
    return _voxel_render("plv", rays, ts, densities, rgb, grid_radius, None, sigmoid_kind, bg, want_weights, pts=pts)


def voxel_sh_sample(densities: torch.Tensor, rgb: torch.Tensor, order: int, grid_radius: float, rays: torch.Tensor,
                    pts: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """raw [..., 4] = [density | s_r s_g s_b], s_c = sum_k Y_k(normalize(rays[..., 3:])) c_ck with c_ck the interpolated coefficient k of
    colour channel c (rgb[..., c (order+1)^2 + k]), of NeRFVoxel's lookup with the spherical-harmonic head, at explicit pts
    [T, *rays.shape[:-1], 3] or at o + t d of rays x ts [T].  The RGB head's layout: no coefficient array exists."""
    return _voxel_sample("sh", densities, rgb, grid_radius, pts, rays, ts, order)


def voxel_sh_sample_backward(g_raw: torch.Tensor, S: int, order: int, grid_radius: float, rays: torch.Tensor,
                             pts: Optional[torch.Tensor] = None, ts: Optional[torch.Tensor] = None, variant: Optional[int] = None):
    """(g_densities [S,S,S,1], g_rgb [S,S,S, 3 (order+1)^2]) of voxel_sh_sample given g_raw [..., 4] and the same positions.
    variant: scatter variant 1 or 2 (measurements); None runs the shipped one of the mode."""
    return _voxel_sample_backward("sh", g_raw, None, S, order, grid_radius, pts, rays, ts, variant)


def voxel_sh_sample_backward_pts(g_raw: torch.Tensor, pts: torch.Tensor, rays: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor,
                                 order: int, grid_radius: float) -> torch.Tensor:
    """g_pts [..., 3]: the gradient of voxel_sh_sample w.r.t. explicit pts given g_raw [..., 4] (a gather, no atomics)"""
    return _voxel_sample_backward_pts("sh", g_raw, None, pts, rays, densities, rgb, grid_radius, order)


def voxel_sh_render(rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, order: int, grid_radius: float,
                    sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True, pts: Optional[torch.Tensor] = None):
    """NeRFVoxel's eval route with the spherical-harmonic head as ONE launch: basis per ray, positions (o + t d, or explicit pts
    [T, ..., 3]) -> lookup -> activation -> compositing.  Outputs and backgrounds of voxel_render."""
    return _voxel_render("sh", rays, ts, densities, rgb, grid_radius, order, sigmoid_kind, bg, want_weights, pts=pts)


# ------------------------------------------------------------------------------------------------- NeRFVoxel coarse -> fine (csrc/voxel_fine.hip)
def voxel_proposal(rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, grid_radius: float):
    """The proposal pass of NeRFVoxel's coarse -> fine route as ONE launch: (alpha [T, ...], weights [T, ...]) of rays [..., 6] over the
    shared steps ts [T] from the density grid [S,S,S,1] alone -- bit for bit what voxel_render / voxel_plv_render / voxel_sh_render return
    as alpha and weights for the same rays, steps and density grid."""
    lib = _lib.load()
    densities, rays, ts = _f32(densities, "densities"), _f32(rays, "rays"), _f32(ts, "ts")
    S = densities.shape[0]
    if densities.dim() != 4 or tuple(densities.shape) != (S, S, S, 1):
        raise ValueError(f"the density grid must be [S,S,S,1], got {tuple(densities.shape)}")
    _voxel_even(S)
    if rays.shape[-1] != 6 or ts.dim() != 1:
        raise ValueError(f"rays must be [..., 6] and ts [T], got {tuple(rays.shape)} and {tuple(ts.shape)}")
    T, R = ts.shape[0], rays.numel() // 6
    alpha = torch.empty((T,) + tuple(rays.shape[:-1]), device=rays.device, dtype=torch.float32)
    weights = torch.empty_like(alpha)
    check(lib.na_voxel_proposal(_ptr(rays), R, _ptr(ts), T, _ptr(densities), S, float(grid_radius), _ptr(alpha), _ptr(weights), _stream()))
    return alpha, weights


def voxel_render_rayts(rays: torch.Tensor, ts_ray: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float,
                       sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True):
    """`voxel_render` over per-ray steps ts_ray [..., M] (one increasing row per ray, e.g. `resample_ts`'s): positions o + t d -> lookup ->
    activation -> compositing as ONE launch.  (out [..., 3], alpha [M, ...], weights [M, ...]); bg black | white."""
    return _voxel_render_rayts("rgb", rays, ts_ray, densities, rgb, grid_radius, None, sigmoid_kind, bg, want_weights)


def voxel_plv_render_rayts(rays: torch.Tensor, ts_ray: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, grid_radius: float,
                           sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True):
    """`voxel_plv_render` over per-ray steps ts_ray [..., M]; outputs and backgrounds of voxel_render_rayts."""
    return _voxel_render_rayts("plv", rays, ts_ray, densities, rgb, grid_radius, None, sigmoid_kind, bg, want_weights)


def voxel_sh_render_rayts(rays: torch.Tensor, ts_ray: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, order: int, grid_radius: float,
                          sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True):
    """`voxel_sh_render` over per-ray steps ts_ray [..., M]; outputs and backgrounds of voxel_render_rayts."""
    return _voxel_render_rayts("sh", rays, ts_ray, densities, rgb, grid_radius, order, sigmoid_kind, bg, want_weights)


def voxel_fine_lanes(head: str, lanes: int, rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: Optional[torch.Tensor],
                     grid_radius: float, order: int = -1, sigmoid_kind: str = "upshifted", bg: str = "black"):
    """Measurements (tools/voxel_fine_bench.py): the proposal (head "density", ts [T]) or a per-ray-step render (head "rgb" | "plv" | "sh",
    ts [..., M]) with `lanes` lanes sharing a ray.  (out or None, alpha, weights)."""
    lib = _lib.load()
    densities, rays, ts = _f32(densities, "densities"), _f32(rays, "rays"), _f32(ts, "ts")
    S, R, M = densities.shape[0], rays.numel() // 6, ts.shape[-1]
    shared = head == "density"
    assert ts.numel() == (M if shared else R * M), (ts.shape, rays.shape)
    if not shared:
        rgb = _aligned16(_f32(rgb, "rgb"))
        want = {"rgb": 3, "plv": 3 + (order + 1) ** 2, "sh": 3 * (order + 1) ** 2}[head]
        assert tuple(rgb.shape) == (S, S, S, want), (rgb.shape, head, order)
    out, alpha, weights = _ls_outputs(rays.shape[:-1], M, rays.device, bg, True)
    check(lib.na_voxel_fine_lanes(VOX_HEAD[head], int(order), int(lanes), 1 if shared else 0, _ptr(rays), R, _ptr(ts), M, _ptr(densities),
                                  _ptr(None if shared else rgb), S, float(grid_radius), SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha),
                                  _ptr(weights), _ptr(None if shared else out), _stream()))
    return (None if shared else out), alpha, weights


# ------------------------------------------------------------------------------------------------- NeRFVoxel.sparsify (csrc/voxel_sparse.hip)
def voxel_d_thresh(thresh: float) -> float:
    """The raw density whose softplus(d - 1) equals `thresh`, 1 + log(expm1(thresh)) in Python doubles rounded once to fp32; -inf for
    thresh == 0 (every voxel is kept).  thresh < 0 or not finite raises ValueError."""
    thresh = float(thresh)
    if not math.isfinite(thresh) or thresh < 0:
        raise ValueError(f"sparsify threshold {thresh!r}: a finite density threshold >= 0")
    if thresh == 0:
        return float("-inf")
    try:
        d = 1 + math.log(math.expm1(thresh))
    except OverflowError:  # (expm1 leaves the doubles above 709: log(expm1(x)) is x there to every digit)
        d = 1 + thresh
    return struct.unpack("f", struct.pack("f", d))[0]


def _voxel_live(live: torch.Tensor, S: int, device) -> torch.Tensor:
    if (not isinstance(live, torch.Tensor) or live.dtype != torch.uint8 or tuple(live.shape) != (S, S, S) or not live.is_contiguous()
            or live.device != device):
        raise ValueError(f"the liveness table must be a contiguous uint8 [{S},{S},{S}] tensor on {device}, got "
                         f"{getattr(live, 'dtype', type(live).__name__)} {tuple(getattr(live, 'shape', ()))} on {getattr(live, 'device', None)}")
    return live


def voxel_live_table(densities: torch.Tensor, thresh: float, want_count: bool = True):
    """(live uint8 [S,S,S], count int64 [1] or None) of a density grid [S,S,S,1] (or [S,S,S]): a voxel is kept iff
    !(d < voxel_d_thresh(thresh)) -- a NaN density is kept -- and live[x,y,z] is the OR of the kept voxels in the window x..x+2, y..y+2,
    z..z+2 clamped at S-1 (the corners a sample whose lower ids are x, y, z can read).  One launch; count is the number of live entries."""
    lib = _lib.load()
    densities = _f32(densities, "densities")
    S = densities.shape[0]
    if tuple(densities.shape) not in ((S, S, S, 1), (S, S, S)):
        raise ValueError(f"the density grid must be [S,S,S,1], got {tuple(densities.shape)}")
    _voxel_even(S)
    d = voxel_d_thresh(thresh)
    live = torch.empty((S, S, S), device=densities.device, dtype=torch.uint8)
    count = torch.empty(1, device=densities.device, dtype=torch.int64) if want_count else None
    check(lib.na_voxel_live_table(_ptr(densities), S, d, _ptr(live), _ptr(count), _stream()))
    return live, count


def voxel_live_samples(live: torch.Tensor, grid_radius: float, pts: Optional[torch.Tensor] = None, rays: Optional[torch.Tensor] = None,
                       ts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 flags of the samples of a voxel lookup: explicit pts [..., 3] (flags [...]), or o + t d of rays [*batch, 6] over a shared row
    ts [M] or per-ray rows ts [*batch, M] (flags [M, *batch]).  A sample is live iff the table holds non-zero at the LOWER ids of its
    cell, or one of its coordinates is not finite."""
    lib = _lib.load()
    S = live.shape[0]
    live = _voxel_live(live, S, live.device)
    if not live.is_cuda:
        raise ValueError("live must be a CUDA(HIP) tensor: the hot path has no CPU implementation")
    if pts is not None:
        pts = _f32(pts, "pts")
        if pts.shape[-1] != 3:
            raise ValueError(f"pts must be [..., 3], got {tuple(pts.shape)}")
        flags = torch.empty(tuple(pts.shape[:-1]), device=live.device, dtype=torch.uint8)
        check(lib.na_voxel_live_samples(_ptr(pts), _ptr(None), _ptr(None), 0, 1, pts.numel() // 3, S, float(grid_radius), _ptr(live),
                                        _ptr(flags), _stream()))
        return flags
    if rays is None or ts is None:
        raise ValueError("voxel_live_samples needs explicit pts, or rays and ts")
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    shared = ts.dim() == 1  # (one row for every ray)
    if rays.shape[-1] != 6 or (not shared and tuple(ts.shape[:-1]) != tuple(rays.shape[:-1])):
        raise ValueError(f"rays must be [..., 6] and ts [M] or [..., M], got {tuple(rays.shape)} and {tuple(ts.shape)}")
    M, R = ts.shape[-1], rays.numel() // 6
    flags = torch.empty((M,) + tuple(rays.shape[:-1]), device=live.device, dtype=torch.uint8)
    check(lib.na_voxel_live_samples(_ptr(None), _ptr(rays), _ptr(ts), 0 if shared else M, M, R, S, float(grid_radius), _ptr(live),
                                    _ptr(flags), _stream()))
    return flags


def voxel_mask_rows(x: torch.Tensor, flags: torch.Tensor, fill0: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[n, :] = flags[n] ? x[n, :] : (fill0, 0, ..., 0) over the rows of x [..., C] (flags uint8 [...]); x itself with all flags set,
    bit for bit.  out: None for a new tensor, or x for in place."""
    lib = _lib.load()
    x = _f32(x, "x")
    Cn = x.shape[-1] if x.dim() > flags.dim() else 1
    N = x.numel() // Cn
    if flags.dtype != torch.uint8 or flags.numel() != N or not flags.is_cuda:
        raise ValueError(f"flags must be uint8 on the GPU, one per row of x ({N}), got {flags.dtype} {tuple(flags.shape)}")
    flags = flags.contiguous()
    if out is None:
        out = torch.empty_like(x)
    check(lib.na_voxel_mask_rows(_ptr(x), _ptr(flags), N, Cn, float(fill0), _ptr(out), _stream()))
    return out


def voxel_sparse_render(head: str, rays: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor, live: torch.Tensor,
                        grid_radius: float, order: int = -1, sigmoid_kind: str = "upshifted", bg: str = "black", want_weights: bool = True,
                        lanes: int = VOXEL_SPARSE_LANES):
    """The one-launch renderers of a voxel model (head "rgb" | "plv" | "sh") over a shared row ts [M] or per-ray rows ts [..., M],
    gathering and walking only the samples the table `live` (uint8 [S,S,S], ops.voxel_live_table) marks: a dead sample has alpha =
    weight = 0 exactly and its colour is not read.  With a table of ones: voxel_*_render_rayts bit for bit.  Outputs of voxel_render_rayts."""
    lib = _lib.load()
    if head not in ("rgb", "plv", "sh"):
        raise ValueError(f"voxel_sparse_render: head {head!r} (rgb, plv, sh)")
    densities, rgb, S, Cn, order = _voxel_head(head, densities, rgb, order)
    if head == "rgb" and Cn != 3:
        raise ValueError(f"voxel_sparse_render: the rgb head has 3 colour parameters per voxel, got {Cn}")
    live = _voxel_live(live, S, densities.device)
    rays, ts = _f32(rays, "rays"), _f32(ts, "ts")
    shared = ts.dim() == 1  # (one row for every ray)
    if rays.shape[-1] != 6 or (not shared and tuple(ts.shape[:-1]) != tuple(rays.shape[:-1])):
        raise ValueError(f"rays must be [..., 6] and ts [M] or [..., M], got {tuple(rays.shape)} and {tuple(ts.shape)}")
    M, R = ts.shape[-1], rays.numel() // 6
    out, alpha, weights = _ls_outputs(rays.shape[:-1], M, rays.device, bg, want_weights)
    check(lib.na_voxel_sparse_render(VOX_HEAD[head], int(order), int(lanes), 1 if shared else 0, _ptr(rays), R, _ptr(ts), M, _ptr(densities),
                                     _ptr(rgb), S, float(grid_radius), _ptr(live), SIGMOID[sigmoid_kind], BG[bg], _ptr(alpha), _ptr(weights),
                                     _ptr(out), _stream()))
    return out, alpha, weights


# ------------------------------------------------------------------------------------------------- DynamicNeRFVoxel (csrc/dyn_voxel.hip)
def _dyn_voxel_grids(ctrl_pts_grid: torch.Tensor, rigidity_grid: torch.Tensor, spline: int):
    """S of ctrl_pts_grid [S,S,S,3(spline-1)] and rigidity_grid [S,S,S,1]"""
    ctrl, rig = _f32(ctrl_pts_grid, "ctrl_pts_grid"), _f32(rigidity_grid, "rigidity_grid")
    _dyn_voxel_spline(spline)
    S = rig.shape[0]
    if rig.dim() != 4 or tuple(rig.shape) != (S, S, S, 1) or tuple(ctrl.shape) != (S, S, S, 3 * (spline - 1)):
        raise ValueError(f"dyn voxel grids must be ctrl_pts_grid [S,S,S,{3 * (spline - 1)}] and rigidity_grid [S,S,S,1], got "
                         f"{tuple(ctrl.shape)} and {tuple(rig.shape)}")
    _dyn_voxel_reso(S)
    return ctrl, rig, S


def _dyn_voxel_spline(spline: int):
    if not 2 <= spline <= 11:
        raise ValueError(f"spline {spline}: 2 .. 11 control points have a kernel (3 (spline - 1) <= {GRID_MAX_C} channels per voxel)")


def _dyn_voxel_reso(S: int):
    if S % 2 != 0 or not 2 <= S <= 1024:
        raise ValueError(f"voxel resolution {S}: even resolutions 2 .. 1024 only (the reference's ids are floor(.) + S / 2)")


def _dyn_voxel_samples(pts: torch.Tensor, t: torch.Tensor):
    pts, t = _f32(pts, "pts"), _f32(t, "t")
    if pts.shape[-1] != 3 or tuple(t.shape) != tuple(pts.shape[:-1]):
        raise ValueError(f"pts must be [..., 3] and t [...] (one time per sample, expanded by the caller), got {tuple(pts.shape)} and "
                         f"{tuple(t.shape)}")
    return pts, t, pts.numel() // 3


def dyn_voxel_warp(pts: torch.Tensor, t: torch.Tensor, ctrl_pts_grid: torch.Tensor, rigidity_grid: torch.Tensor, spline: int,
                   grid_radius: float):
    """DynamicNeRFVoxel's deformation (src/nerf.py:1571-1586) as ONE launch: (warped [..., 3], dp [..., 3], rigidity [...]) of pts [..., 3]
    at times t [...]: the two grids interpolated at the unwarped points, the Bezier spline, warped = pts + dp * rigidity."""
    lib = _lib.load()
    ctrl, rig, S = _dyn_voxel_grids(ctrl_pts_grid, rigidity_grid, spline)
    pts, t, N = _dyn_voxel_samples(pts, t)
    warped, dp = torch.empty_like(pts), torch.empty_like(pts)
    rigidity = torch.empty(pts.shape[:-1], device=pts.device, dtype=torch.float32)
    check(lib.na_dyn_voxel_warp(_ptr(pts), _ptr(t), N, _ptr(ctrl), _ptr(rig), S, spline, float(grid_radius), _ptr(warped), _ptr(dp),
                                _ptr(rigidity), _stream()))
    return warped, dp, rigidity


def dyn_voxel_warp_backward(pts: torch.Tensor, t: torch.Tensor, dp: torch.Tensor, rigidity: torch.Tensor, S: int, spline: int,
                            grid_radius: float, g_warped: Optional[torch.Tensor] = None, g_dp: Optional[torch.Tensor] = None,
                            g_rigidity: Optional[torch.Tensor] = None):
    """(g_ctrl_pts_grid [S,S,S,3(spline-1)], g_rigidity_grid [S,S,S,1]) of dyn_voxel_warp given any of g_warped, g_dp [..., 3] and
    g_rigidity [...] (None = zero) and the forward's dp and rigidity"""
    lib = _lib.load()
    _dyn_voxel_spline(spline)
    _dyn_voxel_reso(S)
    pts, t, N = _dyn_voxel_samples(pts, t)
    dp, rigidity = _f32(dp, "dp"), _f32(rigidity, "rigidity")
    if dp.shape != pts.shape or rigidity.numel() != N:
        raise ValueError(f"dp must be {tuple(pts.shape)} and rigidity one value per sample, got {tuple(dp.shape)} and {tuple(rigidity.shape)}")
    grads = []
    for name, g, numel in (("g_warped", g_warped, 3 * N), ("g_dp", g_dp, 3 * N), ("g_rigidity", g_rigidity, N)):
        if g is not None:
            g = _f32(g, name)
            if g.numel() != numel:
                raise ValueError(f"{name} has {g.numel()} elements, {numel} expected")
        grads.append(g)
    config.require_deterministic_workspace(8 * S ** 3 * (3 * spline - 2))  # (a no-op outside config.set_deterministic's mode)
    g_ctrl = torch.zeros(S, S, S, 3 * (spline - 1), device=pts.device, dtype=torch.float32)
    g_rig = torch.zeros(S, S, S, 1, device=pts.device, dtype=torch.float32)
    check(lib.na_dyn_voxel_warp_backward(_ptr(pts), _ptr(t), N, _ptr(dp), _ptr(rigidity), _ptr(grads[0]), _ptr(grads[1]), _ptr(grads[2]),
                                         S, spline, float(grid_radius), _ptr(g_ctrl), _ptr(g_rig), _stream()))
    return g_ctrl, g_rig


def _dyn_voxel_direction(v: Optional[torch.Tensor], pts: torch.Tensor):
    if v is not None:
        v = _f32(v, "v")
        if v.shape != pts.shape:
            raise ValueError(f"v must be {tuple(pts.shape)} (one direction per sample) or None for ones, got {tuple(v.shape)}")
    return v


def dyn_voxel_jac_quad(pts: torch.Tensor, t: torch.Tensor, ctrl_pts_grid: torch.Tensor, rigidity_grid: Optional[torch.Tensor], spline: int,
                       grid_radius: float, v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """v . (J v) per sample [...] of pts [..., 3] at times t [...] as ONE launch (csrc/dyn_voxel_div.hip), J the Jacobian w.r.t. the
    unwarped position of dyn_voxel_warp's dp (rigidity_grid None: utils.divergence with v = None, i.e. ones) or of dp * rigidity
    (rigidity_grid given: utils.div_approx with v the normal draw).  Nothing per sample but the result is written."""
    lib = _lib.load()
    if rigidity_grid is None:
        _dyn_voxel_spline(spline)
        ctrl, rig = _f32(ctrl_pts_grid, "ctrl_pts_grid"), None
        S = ctrl.shape[0]
        if ctrl.dim() != 4 or tuple(ctrl.shape) != (S, S, S, 3 * (spline - 1)):
            raise ValueError(f"ctrl_pts_grid must be [S,S,S,{3 * (spline - 1)}], got {tuple(ctrl.shape)}")
        _dyn_voxel_reso(S)
    else:
        ctrl, rig, S = _dyn_voxel_grids(ctrl_pts_grid, rigidity_grid, spline)
    pts, t, N = _dyn_voxel_samples(pts, t)
    v = _dyn_voxel_direction(v, pts)
    out = torch.empty(pts.shape[:-1], device=pts.device, dtype=torch.float32)
    check(lib.na_dyn_voxel_jac_quad(_ptr(pts), _ptr(t), N, _ptr(ctrl), _ptr(rig), S, spline, float(grid_radius), _ptr(v), _ptr(out), _stream()))
    return out


def dyn_voxel_jac_quad_backward(pts: torch.Tensor, t: torch.Tensor, S: int, spline: int, grid_radius: float, g: torch.Tensor,
                                v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """g_ctrl_pts_grid [S,S,S,3(spline-1)] of dyn_voxel_jac_quad's dp form given g [...] (one value per sample): one scatter-add launch.
    The dp * rigidity form has no gradient (the reference's estimate has no graph); pts, t and v get none."""
    lib = _lib.load()
    _dyn_voxel_spline(spline)
    _dyn_voxel_reso(S)
    pts, t, N = _dyn_voxel_samples(pts, t)
    v = _dyn_voxel_direction(v, pts)
    g = _f32(g, "g")
    if g.numel() != N:
        raise ValueError(f"g has {g.numel()} elements, one per sample ({N}) expected")
    config.require_deterministic_workspace(8 * S ** 3 * 3 * (spline - 1))
    out = torch.zeros(S, S, S, 3 * (spline - 1), device=pts.device, dtype=torch.float32)
    check(lib.na_dyn_voxel_jac_quad_backward(_ptr(pts), _ptr(t), N, S, spline, float(grid_radius), _ptr(v), _ptr(g), _ptr(out), _stream()))
    return out


DYN_VOXEL_MAPS = ("depth", "acc", "flow", "rigidity", "alpha", "weights")


def dyn_voxel_render(rays: torch.Tensor, t: torch.Tensor, ts: torch.Tensor, densities: torch.Tensor, rgb: torch.Tensor,
                     ctrl_pts_grid: torch.Tensor, rigidity_grid: torch.Tensor, spline: int, grid_radius: float,
                     sigmoid_kind: str = "upshifted", bg: str = "black", want=("depth", "flow", "rigidity"), plv: bool = False,
                     sh_order: Optional[int] = None):
    """DynamicNeRFVoxel's test-time render as ONE launch (csrc/dyn_voxel_render.hip): rays [..., 6] at times t [...] (one per ray, expanded
    by the caller) over the steps ts [T] -> dict(rgb [..., 3] + the outputs named in `want`: depth [..., 1], acc [..., 1], flow [..., 3],
    rigidity [..., 1] -- the maps of runner.py:894-916 -- and alpha, weights [T, ...]).  Bit for bit compute_pts -> dyn_voxel_warp ->
    voxel_render(pts=warped) -> integrate x 4, without their per-sample tensors.  bg black | white (random: black, then sky_random).
    plv: the canonical model carries the pos-linear-view head (rgb [S,S,S, 3 + (order+1)^2]; na_dyn_voxel_plv_render, the composition
    then being over voxel_plv_render).  sh_order: it carries the spherical-harmonic colour head of that order (rgb [S,S,S, 3 (order+1)^2];
    na_dyn_voxel_sh_render, the composition over voxel_sh_render)."""
    if sh_order is not None and plv:
        raise ValueError("dyn_voxel_render: plv and sh_order name two different heads")
    kind = "sh" if sh_order is not None else "plv" if plv else "rgb"
    densities, rgb, S, Cn, order = _voxel_head(kind, densities, rgb, sh_order)
    ctrl, rig, S2 = _dyn_voxel_grids(ctrl_pts_grid, rigidity_grid, spline)
    if S2 != S:
        raise ValueError(f"the canonical grids are {S}^3 and the deformation grids {S2}^3")
    rays, t, ts = _f32(rays, "rays"), _f32(t, "t"), _f32(ts, "ts")
    if rays.shape[-1] != 6 or ts.dim() != 1 or tuple(t.shape) != tuple(rays.shape[:-1]):
        raise ValueError(f"rays must be [..., 6], t [...] (one time per ray, expanded by the caller) and ts [T], got {tuple(rays.shape)}, "
                         f"{tuple(t.shape)} and {tuple(ts.shape)}")
    unknown = set(want) - set(DYN_VOXEL_MAPS)
    if unknown:
        raise ValueError(f"want {sorted(unknown)}: the optional outputs are {DYN_VOXEL_MAPS}")
    if bg not in BG:
        raise NotImplementedError(bg)
    batch, T, R = tuple(rays.shape[:-1]), ts.shape[0], rays.numel() // 6
    new = lambda *shape: torch.empty(shape, device=rays.device, dtype=torch.float32)
    res = {"rgb": new(*batch, 3)}
    for name, shape in (("depth", batch + (1,)), ("acc", batch + (1,)), ("flow", batch + (3,)), ("rigidity", batch + (1,)),
                        ("alpha", (T,) + batch), ("weights", (T,) + batch)):
        if name in want:
            res[name] = new(*shape)
    fn, head = _voxel_abi(kind, Cn, order)
    check(fn["dyn_render"](_ptr(rays), _ptr(t), R, _ptr(ts), T, _ptr(densities), _ptr(rgb), _ptr(ctrl), _ptr(rig), S, *head, spline, float(grid_radius),
                SIGMOID[sigmoid_kind], BG[bg], _ptr(res["rgb"]), *(_ptr(res.get(name)) for name in DYN_VOXEL_MAPS), _stream()))
    return res


# ------------------------------------------------------------------------------------------------- grid operators (csrc/grid_ops.hip)
GRID_MAX_C = 32


def _grid4(grid: torch.Tensor, name: str = "grid") -> torch.Tensor:
    """a channel-last grid [s0,s1,s2,C] as the kernels read it: device, fp32, contiguous (nothing is converted or copied silently)"""
    if not grid.is_cuda:
        raise ValueError(f"{name} must be a CUDA(HIP) tensor: the hot path has no CPU implementation")
    if grid.dim() != 4 or grid.dtype != torch.float32 or not grid.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 [s0,s1,s2,C], got {grid.dtype} {tuple(grid.shape)} "
                         f"{'contiguous' if grid.is_contiguous() else 'strided'}")
    if not 1 <= grid.shape[-1] <= GRID_MAX_C:
        raise ValueError(f"{name} has {grid.shape[-1]} channels: 1 .. {GRID_MAX_C} have a kernel")
    if min(grid.shape[:3]) < 2 or max(grid.shape[:3]) > 1024:
        raise ValueError(f"{name} {tuple(grid.shape[:3])}: 2 .. 1024 voxels per axis (a voxel's neighbour is v + 1, or v - 1 on the last plane)")
    return grid


def _grid_idxs(grid: torch.Tensor, idxs: torch.Tensor, trusted: bool) -> torch.Tensor:
    if not idxs.is_cuda or idxs.device != grid.device:
        raise ValueError("idxs must live on the grid's device")
    if idxs.dtype != torch.int64:
        raise ValueError(f"idxs must be int64 (what torch.randint draws), got {idxs.dtype}")
    idxs = idxs.reshape(-1).contiguous()
    if idxs.numel() < 1:
        raise ValueError("idxs is empty: the mean over no samples")
    n_elem = grid.shape[0] * grid.shape[1] * grid.shape[2]
    if not trusted and bool(((idxs < 0) | (idxs >= n_elem)).any()):  # (ONE host check; the kernels clamp whatever they are given)
        raise ValueError(f"idxs outside the grid: flat indices 0 .. {n_elem - 1}")
    return idxs


def grid_tv(grid: torch.Tensor, idxs: torch.Tensor, trusted: bool = False) -> torch.Tensor:
    """0-dim total_variation (src/nerf.py:381-399) of grid [s0,s1,s2,C] at the flat indices idxs [n] int64 (x = idx % s0 ...): one launch.
    trusted: the indices were drawn inside the grid (nerf.random_sample_grid) -- the host range check, a synchronisation, is skipped."""
    lib = _lib.load()
    grid = _grid4(grid)
    idxs = _grid_idxs(grid, idxs, trusted)
    out = torch.zeros(2, device=grid.device, dtype=torch.float32)  # [value | arrival counter]
    s0, s1, s2, Cn = grid.shape
    check(lib.na_grid_tv(_ptr(grid), s0, s1, s2, Cn, _ptr(idxs), idxs.numel(), _ptr(out), _stream()))
    return out[0]


def grid_tv_backward(grid: torch.Tensor, idxs: torch.Tensor, g: torch.Tensor, trusted: bool = False) -> torch.Tensor:
    """gradient of grid_tv w.r.t. grid times the device scalar g (read by the kernel: no host synchronisation)"""
    lib = _lib.load()
    grid = _grid4(grid)
    idxs = _grid_idxs(grid, idxs, trusted)
    g = _f32(g.reshape(1), "g")
    config.require_deterministic_workspace(8 * grid.numel())  # (ctrl_pts_grid at S = 64 is larger than config's default workspace)
    out = torch.zeros_like(grid)
    s0, s1, s2, Cn = grid.shape
    check(lib.na_grid_tv_backward(_ptr(grid), s0, s1, s2, Cn, _ptr(idxs), idxs.numel(), _ptr(g), _ptr(out), _stream()))
    return out


def grid_upsample(grid: torch.Tensor, reso: int) -> torch.Tensor:
    """[R,R,R,C] = F.interpolate(mode="trilinear", align_corners=False) of the cubic grid [S,S,S,C] (src/nerf.py:377-379): one launch"""
    lib = _lib.load()
    grid = _grid4(grid)
    S, reso = grid.shape[0], int(reso)
    if tuple(grid.shape[:3]) != (S, S, S):
        raise ValueError(f"grid_upsample takes a cubic grid, got {tuple(grid.shape)}")
    if S % 2 != 0 or reso % 2 != 0 or not 2 <= reso <= 1024:
        raise ValueError(f"grid_upsample {S} -> {reso}: even resolutions 2 .. 1024 only")
    out = torch.empty(reso, reso, reso, grid.shape[-1], device=grid.device, dtype=torch.float32)
    check(lib.na_grid_upsample(_ptr(grid), S, _ptr(out), reso, grid.shape[-1], _stream()))
    return out


# ------------------------------------------------------------------------------------------------- spline lengths (csrc/spline_len.hip)
SPLINE_LEN_SAMPLES = 16  # arc_len's samples=16 (src/nerf.py:1509): the only value the Python side uses


_spline_len_tables = {}


def _spline_len_table(device_str: str) -> torch.Tensor:
    """torch.linspace(0, 1, 16)'s own fp32 values, formed on the CPU as the reference's operators see them and copied to the device
    once: the kernels read the table and never form j / 15 themselves"""
    if device_str not in _spline_len_tables:
        _spline_len_tables[device_str] = torch.linspace(0, 1, SPLINE_LEN_SAMPLES, dtype=torch.float32).to(device_str)
    return _spline_len_tables[device_str]


def _spline_len_grid(grid: torch.Tensor):
    """a grid [..., 3 m] of m = 1 .. 10 control points per row as the kernels read it -> (grid, rows, m)"""
    grid = _f32(grid, "grid")
    C = grid.shape[-1]
    if grid.dim() < 2 or C % 3 != 0 or not 1 <= C // 3 <= 10:
        raise ValueError(f"grid must be [..., 3 m] with m = 1 .. 10 control points per row (spline 2 .. 11), got {tuple(grid.shape)}")
    return grid, grid.numel() // C, C // 3


def _spline_len_idxs(rows: int, idxs: torch.Tensor, device, trusted: bool) -> torch.Tensor:
    if not idxs.is_cuda or idxs.device != device:
        raise ValueError("idxs must live on the grid's device")
    if idxs.dtype != torch.int64:
        raise ValueError(f"idxs must be int64 (what torch.randint draws), got {idxs.dtype}")
    idxs = idxs.reshape(-1).contiguous()
    if idxs.numel() < 1:
        raise ValueError("idxs is empty: the mean over no rows")
    if not trusted and bool(((idxs < 0) | (idxs >= rows)).any()):  # (ONE host check; the kernels clamp whatever they are given)
        raise ValueError(f"idxs outside the grid: flat rows 0 .. {rows - 1}")
    return idxs


def grid_spline_len(grid: torch.Tensor, idxs: torch.Tensor, trusted: bool = False, want_lens: bool = False):
    """0-dim mean arc length (arc_len, src/nerf.py:1509-1520) of the splines whose m control points are the rows idxs [K] int64 of
    grid [..., 3 m] (control point 0 is not prepended: runner.py:793-796): one launch.  want_lens: (value, lens [K])."""
    lib = _lib.load()
    grid, rows, m = _spline_len_grid(grid)
    idxs = _spline_len_idxs(rows, idxs, grid.device, trusted)
    out = torch.zeros(2, device=grid.device, dtype=torch.float32)  # [value | arrival counter]
    lens = torch.empty(idxs.numel(), device=grid.device, dtype=torch.float32) if want_lens else None
    check(lib.na_grid_spline_len(_ptr(grid), rows, m, _ptr(idxs), idxs.numel(), _ptr(_spline_len_table(str(grid.device))),
                                 SPLINE_LEN_SAMPLES, _ptr(lens), _ptr(out), _stream()))
    return (out[0], lens) if want_lens else out[0]


def grid_spline_len_backward(grid: torch.Tensor, idxs: torch.Tensor, g: torch.Tensor, trusted: bool = False) -> torch.Tensor:
    """gradient of grid_spline_len w.r.t. grid times the device scalar g (read by the kernel: no host synchronisation)"""
    lib = _lib.load()
    grid, rows, m = _spline_len_grid(grid)
    idxs = _spline_len_idxs(rows, idxs, grid.device, trusted)
    g = _f32(g.reshape(1), "g")
    config.require_deterministic_workspace(8 * grid.numel())
    out = torch.zeros_like(grid)
    check(lib.na_grid_spline_len_backward(_ptr(grid), rows, m, _ptr(idxs), idxs.numel(), _ptr(_spline_len_table(str(grid.device))),
                                          SPLINE_LEN_SAMPLES, _ptr(g), _ptr(out), _stream()))
    return out


def _spline_len_samples(pts: torch.Tensor, ctrl_pts_grid: torch.Tensor, spline: int, w: Optional[torch.Tensor]):
    _dyn_voxel_spline(spline)
    ctrl, pts = _f32(ctrl_pts_grid, "ctrl_pts_grid"), _f32(pts, "pts")
    S = ctrl.shape[0]
    if ctrl.dim() != 4 or tuple(ctrl.shape) != (S, S, S, 3 * (spline - 1)):
        raise ValueError(f"ctrl_pts_grid must be [S,S,S,{3 * (spline - 1)}], got {tuple(ctrl.shape)}")
    _dyn_voxel_reso(S)
    if pts.shape[-1] != 3 or pts.numel() < 3:
        raise ValueError(f"pts must be a non-empty [..., 3], got {tuple(pts.shape)}")
    N = pts.numel() // 3
    if w is not None:
        w = _f32(w, "w")
        if w.numel() != N:
            raise ValueError(f"w has {w.numel()} elements, one per sample ({N}) expected")
    return pts, ctrl, S, N, w


def dyn_voxel_spline_len(pts: torch.Tensor, ctrl_pts_grid: torch.Tensor, spline: int, grid_radius: float,
                         w: Optional[torch.Tensor] = None, want_lens: bool = False):
    """0-dim mean over the samples pts [..., 3] of w * arc_len(control points of the sample) (runner.py:784-787; w None = 1): the
    control points 1 .. spline-1 are interpolated from ctrl_pts_grid as dyn_voxel_warp does, behind the zero control point 0, and
    never leave the registers.  One launch.  want_lens: (value, lens [...])."""
    lib = _lib.load()
    pts, ctrl, S, N, w = _spline_len_samples(pts, ctrl_pts_grid, spline, w)
    out = torch.zeros(2, device=pts.device, dtype=torch.float32)  # [value | arrival counter]
    lens = torch.empty(pts.shape[:-1], device=pts.device, dtype=torch.float32) if want_lens else None
    check(lib.na_dyn_voxel_spline_len(_ptr(pts), N, _ptr(ctrl), S, spline, float(grid_radius), _ptr(w), _ptr(_spline_len_table(str(pts.device))),
                                      SPLINE_LEN_SAMPLES, _ptr(lens), _ptr(out), _stream()))
    return (out[0], lens) if want_lens else out[0]


def dyn_voxel_spline_len_backward(pts: torch.Tensor, ctrl_pts_grid: torch.Tensor, spline: int, grid_radius: float, g: torch.Tensor,
                                  w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gradient of dyn_voxel_spline_len w.r.t. ctrl_pts_grid times the device scalar g: one scatter-add launch (pts and w get none)"""
    lib = _lib.load()
    pts, ctrl, S, N, w = _spline_len_samples(pts, ctrl_pts_grid, spline, w)
    g = _f32(g.reshape(1), "g")
    config.require_deterministic_workspace(8 * ctrl.numel())
    out = torch.zeros_like(ctrl)
    check(lib.na_dyn_voxel_spline_len_backward(_ptr(pts), N, _ptr(ctrl), S, spline, float(grid_radius), _ptr(w),
                                               _ptr(_spline_len_table(str(pts.device))), SPLINE_LEN_SAMPLES, _ptr(g), _ptr(out), _stream()))
    return out


# ------------------------------------------------------------------------------------------------- SSIM / MS-SSIM (csrc/ssim.hip)
SSIM_WINDOW = 11
MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # pytorch_msssim's default scale weights
MS_SSIM_MIN_SIDE = (SSIM_WINDOW - 1) * 2 ** (len(MS_SSIM_WEIGHTS) - 1)  # 160: both sides must be LARGER (the library's assertion)


def _ssim_images(x: torch.Tensor, y: torch.Tensor, flag: str):
    """the image pair [N,H,W,C] as the kernels read it: device, fp32, channel-last, contiguous, C = 1 .. 4 -> (x, y, N, H, W, C).
    flag: the caller's command-line flag, named where a CPU tensor arrives (there is no CPU implementation)"""
    if not x.is_cuda or not y.is_cuda:
        raise NotImplementedError(f"{flag} runs on the GPU only: SSIM is a HIP kernel (DESIGN.md 3r) and the images are on "
                                  f"{x.device} / {y.device}")
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"{flag}: two channel-last images [N,H,W,C] of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    x, y = _f32(x, "x"), _f32(y, "y")
    N, H, W, Cn = x.shape
    if not 1 <= Cn <= 4:
        raise ValueError(f"{flag}: {Cn} channels, 1 .. 4 have a kernel")
    if min(H, W) < SSIM_WINDOW:
        raise ValueError(f"{flag}: a {H} x {W} image is smaller than the {SSIM_WINDOW}-tap window")
    return x, y, N, H, W, Cn


def ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, flag: str = "ops.ssim"):
    """(ssim [N,C], cs [N,C]): the means of SSIM and of its contrast-structure factor over the valid (H-10) x (W-10) map of the
    channel-last pair x, y [N,H,W,C] (11-tap Gaussian window, sigma 1.5).  Two launches, no atomics: bit-identical from run to run."""
    lib = _lib.load()
    x, y, N, H, W, Cn = _ssim_images(x, y, flag)
    out = torch.empty(N, Cn, 2, device=x.device, dtype=torch.float32)
    nbytes = int(lib.na_ssim_workspace_bytes(N, H, W, Cn))
    ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
    check(lib.na_ssim(_ptr(x), _ptr(y), N, H, W, Cn, float(data_range), _ptr(out), _ptr(ws), nbytes, _stream()))
    return out[..., 0], out[..., 1]


def ssim_backward(x: torch.Tensor, y: torch.Tensor, g: torch.Tensor, data_range: float = 1.0, flag: str = "ops.ssim") -> torch.Tensor:
    """g_x [N,H,W,C]: the gradient of sum g[n,c] ssim[n,c] w.r.t. x (y takes none); one launch, every element written once"""
    lib = _lib.load()
    x, y, N, H, W, Cn = _ssim_images(x, y, flag)
    g = _f32(g, "g")
    if tuple(g.shape) != (N, Cn):
        raise ValueError(f"g must be [N,C] = {(N, Cn)}, got {tuple(g.shape)}")
    out = torch.empty_like(x)
    check(lib.na_ssim_backward(_ptr(x), _ptr(y), _ptr(g), N, H, W, Cn, float(data_range), _ptr(out), _stream()))
    return out


def image_halve(x: torch.Tensor, y: Optional[torch.Tensor] = None, flag: str = "ops.image_halve"):
    """F.avg_pool2d(kernel 2, padding (H % 2, W % 2)) of channel-last images [N,H,W,C] -> [N, H // 2 + H % 2, W // 2 + W % 2, C]; with y
    both images in ONE launch -> (x', y')"""
    lib = _lib.load()
    if not x.is_cuda or (y is not None and not y.is_cuda):
        raise NotImplementedError(f"{flag} runs on the GPU only: the 2 x 2 pooling between MS-SSIM's scales is a HIP kernel (DESIGN.md 3r)")
    if x.dim() != 4 or (y is not None and y.shape != x.shape):
        raise ValueError(f"{flag}: channel-last images [N,H,W,C] of one shape, got {tuple(x.shape)}" + ("" if y is None else f" and {tuple(y.shape)}"))
    x = _f32(x, "x")
    y = None if y is None else _f32(y, "y")
    N, H, W, Cn = x.shape
    if not 1 <= Cn <= 4:
        raise ValueError(f"{flag}: {Cn} channels, 1 .. 4 have a kernel")
    ox = torch.empty(N, H // 2 + H % 2, W // 2 + W % 2, Cn, device=x.device, dtype=torch.float32)
    oy = None if y is None else torch.empty_like(ox)
    check(lib.na_image_halve(_ptr(x), _ptr(y), N, H, W, Cn, _ptr(ox), _ptr(oy), _stream()))
    return ox if y is None else (ox, oy)


def ms_ssim_combine(vals: torch.Tensor, weights=MS_SSIM_WEIGHTS) -> torch.Tensor:
    """[N,C] = prod_i relu(vals[i]) ** weights[i] of the per-scale values vals [5,N,C] (cs of scales 0 .. 3, ssim of scale 4): plain torch
    on whatever device and dtype vals has, so a host test can feed it reference sums"""
    if vals.dim() != 3 or vals.shape[0] != len(weights):
        raise ValueError(f"vals must be [{len(weights)},N,C], got {tuple(vals.shape)}")
    w = torch.tensor(weights, dtype=vals.dtype, device=vals.device)
    return torch.prod(torch.relu(vals) ** w[:, None, None], dim=0)


def ms_ssim_check_size(H: int, W: int, flag: str = "ops.ms_ssim"):
    if min(H, W) <= MS_SSIM_MIN_SIDE:
        raise ValueError(f"{flag}: image size should be larger than {MS_SSIM_MIN_SIDE} due to the {len(MS_SSIM_WEIGHTS) - 1} downsamplings "
                         f"in ms-ssim, got {H} x {W}")


def ms_ssim(x: torch.Tensor, y: torch.Tensor, data_range: float = 1.0, flag: str = "ops.ms_ssim") -> torch.Tensor:
    """[N,C] MS-SSIM of the channel-last pair x, y [N,H,W,C], min(H, W) > 160: five scales, image_halve between them, cs of scales
    0 .. 3 and ssim of scale 4 through relu, weighted geometric mean.  A metric: no backward."""
    if x.dim() == 4:
        ms_ssim_check_size(x.shape[1], x.shape[2], flag)
    vals = []
    with torch.no_grad():
        for i in range(len(MS_SSIM_WEIGHTS)):
            s, cs = ssim(x, y, data_range, flag)
            if i < len(MS_SSIM_WEIGHTS) - 1:
                vals.append(cs)
                x, y = image_halve(x, y, flag)
            else:
                vals.append(s)
        return ms_ssim_combine(torch.stack(vals, dim=0))


# ------------------------------------------------------------------------------------------------- the loss wrapper (csrc/image_loss.hip)
IMAGE_SPACES = {"rgb": 1, "hsv": 2, "luminance": 4, "xyz": 8}   # NA_SPACE_*
IMAGE_LOSS_FNS = {"l2": 1, "l1": 2, "rmse": 4}                   # NA_LOSS_*
_image_loss_ws = {}  # (device index, stream) -> the zeroed workspace na_image_loss leaves zeroed (its arrival counter)


def image_loss_masks(loss_fns, color_spaces, gamma, flag: str = "ops.image_loss"):
    """(mask of spaces, mask of functions, gamma) of the names of --color-spaces / --loss-fns and of --gamma-correct-loss; anything the
    kernel has no form for raises a ValueError that names it"""
    masks = []
    for names, table, what in ((color_spaces, IMAGE_SPACES, "--color-spaces"), (loss_fns, IMAGE_LOSS_FNS, "--loss-fns")):
        names = list(names)
        if not names:
            raise ValueError(f"{flag}: {what} is empty, must provide at least 1")
        bad = [n for n in names if n not in table]
        if bad:
            raise ValueError(f"{flag}: {what} {bad[0]!r} is not one of {sorted(table)}")
        if len(set(names)) != len(names):
            raise ValueError(f"{flag}: {what} {names} names an entry twice")
        masks.append(sum(table[n] for n in names))
    gamma = float(gamma)
    if not (gamma > 0 and gamma != float("inf")):
        raise ValueError(f"{flag}: --gamma-correct-loss {gamma} must be finite and > 0")
    return masks[0], masks[1], gamma


def _image_pair(got: torch.Tensor, ref: torch.Tensor, flag: str):
    if got.shape != ref.shape or got.dim() < 1 or got.shape[-1] != 3 or got.numel() == 0:
        raise ValueError(f"{flag}: two images [..., 3] of one shape with at least one pixel, got {tuple(got.shape)} and {tuple(ref.shape)}")
    return _f32(got, "got"), _f32(ref, "ref"), got.numel() // 3


def image_loss(got: torch.Tensor, ref: torch.Tensor, loss_fns=("l2",), color_spaces=("rgb",), tone_map: bool = False, gamma: float = 1.0,
               flag: str = "ops.image_loss"):
    """(loss, stats[8]) of got, ref [..., 3]: the mean over color_spaces of the mean over loss_fns, after the gamma step and the tone
    map (the reference's loss wrapper).  ONE launch, no host synchronisation, bit-identical from run to run; stats feeds the backward."""
    lib = _lib.load()
    spaces, fns, gamma = image_loss_masks(loss_fns, color_spaces, gamma, flag)
    got, ref, P = _image_pair(got, ref, flag)
    nbytes = int(lib.na_image_loss_workspace_bytes(P))
    key = (got.device.index, torch.cuda.current_stream().cuda_stream)
    ws = _image_loss_ws.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = _image_loss_ws[key] = torch.zeros(max(nbytes // 4, 1024), device=got.device, dtype=torch.float32)
    out = torch.empty((), device=got.device, dtype=torch.float32)
    stats = torch.empty(8, device=got.device, dtype=torch.float32)
    check(lib.na_image_loss(_ptr(got), _ptr(ref), P, spaces, fns, gamma, int(bool(tone_map)), _ptr(out), _ptr(stats), _ptr(ws), ws.numel() * 4,
                            _stream()))
    return out, stats


def image_loss_backward(got: torch.Tensor, ref: torch.Tensor, stats: torch.Tensor, g_up: torch.Tensor, loss_fns=("l2",), color_spaces=("rgb",),
                        tone_map: bool = False, gamma: float = 1.0, flag: str = "ops.image_loss") -> torch.Tensor:
    """g_got (shaped like got) = g_up d loss / d got from the forward's stats; g_up is a device scalar the kernel reads.  ONE launch,
    every element written once"""
    lib = _lib.load()
    spaces, fns, gamma = image_loss_masks(loss_fns, color_spaces, gamma, flag)
    shape = got.shape
    got, ref, P = _image_pair(got, ref, flag)
    stats, g_up = _f32(stats, "stats"), _f32(g_up, "g_up")
    if stats.numel() != 8 or g_up.numel() != 1:
        raise ValueError(f"{flag}: stats of 8 floats and a scalar g_up, got {tuple(stats.shape)} and {tuple(g_up.shape)}")
    out = torch.empty(P, 3, device=got.device, dtype=torch.float32)
    check(lib.na_image_loss_backward(_ptr(got), _ptr(ref), P, spaces, fns, gamma, int(bool(tone_map)), _ptr(stats), _ptr(g_up), _ptr(out), _stream()))
    return out.view(shape)
