"""Plain fp64 restatement of DynamicNeRFVoxel's one-launch test render (csrc/dyn_voxel_render.hip, na_dyn_voxel_render): rays x times
-> rgb and the depth / accumulation / flow / rigidity maps of runner.py:894-916, with the error bounds the kernel is held to.  Imported
by tests/test_dyn_voxel_maps_ref.py (CPU) and tests/test_gpu_dyn_voxel_render.py.

Cell membership is fp32 and part of the operator's definition, as in voxel_ref / dyn_voxel_ref: the deformation grids are read at the
cells of the fp32 positions o + t d (voxel_ref.pts_of, voxel_ref.cells), the canonical grids at the cells of the fp32 image of the
restated warped point.  Everything behind the cells is fp64: dyn_voxel_ref.warp_ref, voxel_ref.sample_ref, composite_ref.composite_ref.

THE BOUNDS (derived, not tuned; first order in u = 2^-24).  Three stages, each one's bound the next one's input error:

  deformation   dyn_voxel_ref.warp_ref's b_warped, b_dp, b_rigidity as they stand; rigid_dp = dp r, one product:
                    |d(dp r)| <= |r| b_dp + |dp| b_r + u |dp r|
  lookup        raw_c = sum_u w_u v_uc at the warped point: voxel_ref's gather bound SAMPLE_C u mag_c, plus the warped point's own error.
                The lookup is a continuous function of the position, inside a cell the polynomial whose slope along axis a is
                (1 / voxel_len) sum_u s_ua d_ua v_uc (d_ua the product of the other two axes' factors; dyn_voxel_ref's position
                gradient), so a displacement delta moves raw_c by at most sum_a delta_a slope_ca, slope_ca = (1 / voxel_len) sum_u
                |d_ua| |v_uc|.  delta = b_warped + u |warped| (the kernel's fp32 point against the fp64 one, and the rounding of the
                fp64 point to the fp32 one whose cells this file reads):
                    |d raw_c| <= SAMPLE_C u mag_c + sum_a (b_warped_a + u |warped_a|) slope_ca
  compositing   composite_ref.forward_bounds with its inputs' errors filled in:
                    density  the logit v = raw_0 - 1 carries |d raw_0| (+ u |v| where the fp32 difference is inexact: forward_bounds'
                             own term); an absolute error of the logit is sigmoid(v) / softplus(v) of it relative on sigma, so
                             eps_sigma = EPS_SOFTPLUS + (|d raw_0| + u |v|) sigmoid(v) / softplus(v)
                    colour   act(raw_c), act = sigmoid (+ the kind's affine map): slope <= SLOPE[kind] passes |d raw_c| on; the libm
                             sigmoid EPS_SIGMOID_LIBM relative, the affine map of `thin` / `upshifted` at most 4 roundings of values
                             <= 1.02:  err_c = SLOPE |d raw_c| + (EPS_SIGMOID_LIBM + 4 u) (|c| + 0.02)
                    rgb      forward_bounds(feat = colour, err_c), with the kernel's sky
                    depth    forward_bounds(feat = ts, err_c = 0): the steps are inputs
                    acc      forward_bounds(feat = [1 .. 1 0], err_c = 0)
                    flow     forward_bounds(feat = dp r, err_c = |d(dp r)|)
                    rigidity forward_bounds(feat = r, err_c = b_r)
                every map is `out = sum_t w_t feat_t` against a black sky; forward_bounds' (T + 2) u sum covers the sequential sum.
An entry with bound 0 must be exact.  A ray with a non-finite coordinate is NaN in every output (voxel_ref.worst_ratio counts NaN in
both as equal)."""
import torch

import oracle as O
import composite_ref as CR
import dyn_voxel_ref as D
import voxel_ref as V

U = V.U
MAPS = ("depth", "acc", "flow", "rigidity")
OUTPUTS = ("rgb",) + MAPS + ("alpha", "weights")
PER_SAMPLE = ("alpha", "weights", "dp", "rig")   # [T, R, ...]; every other output is [R, ...]
# act -> the largest slope of the oracle's fp64 activation (oracle.sigmoid): the kinds the g25 fixtures and the tests use; leaky_relu is
# one product by 0.01f, itself 2^-25 off 0.01, inside EPS_COLOUR
SLOPE = {"normal": 0.25, "upshifted": 0.25, "thin": 0.25, "leaky_relu": 1.0}
EPS_COLOUR = CR.EPS_SIGMOID_LIBM + 4.0 * U


def lookup_ref(pts64, d_pts, densities, rgb, grid_radius=V.GRID_RADIUS):
    """raw [N, 4] fp64 at the fp32 image of pts64 [N, 3] and its bound given the positions' own bound d_pts [N, 3] (module docstring)"""
    S = densities.shape[0]
    p32 = pts64.float()
    ids, xyz = V.cells(p32, S, grid_radius)
    rows, w = V.rows_of(ids, S), V.weights_of(xyz)
    grid = torch.cat([densities, rgb], dim=-1).double().reshape(S ** 3, -1)[rows]       # [N,8,4]
    raw = (w[..., None] * grid).sum(dim=1)
    mag = (w[..., None] * grid).abs().sum(dim=1)
    x = xyz.double()
    x = torch.where(torch.isfinite(x).all(dim=-1, keepdim=True), x, torch.full_like(x, float("nan")))
    vl = float(torch.tensor(grid_radius * 2 / S, dtype=torch.float32))
    delta = d_pts + U * pts64.abs()
    move = torch.zeros_like(raw)
    for a in range(3):
        o1, o2 = [i for i in range(3) if i != a]
        slope = torch.zeros_like(raw)
        for u in range(8):
            f = lambda i: x[:, i] if V.bit_i(u, i) else 1 - x[:, i]
            slope = slope + (f(o1) * f(o2)).abs()[:, None] * grid[:, u].abs()
        move = move + delta[:, a, None] * slope / vl
    return raw, V.SAMPLE_C * U * mag + move


def render_ref(rays, t_ray, ts, densities, rgb, ctrl, rig, spline, grid_radius=V.GRID_RADIUS, act="upshifted", bg="black"):
    """rays [R,6], t_ray [R], ts [T] fp32 and the four grids -> dict of fp64 tensors rgb [R,3], depth [R,1], acc [R,1], flow [R,3],
    rigidity [R,1], alpha, weights [T,R] and their bounds under "b_" + name; dp [T,R,3] and rig [T,R] (the per-sample deformation) ride
    along for the tests that form the reference's maps themselves"""
    assert rays.dim() == 2 and t_ray.shape == rays.shape[:1] and bg in ("black", "white")
    R, T = rays.shape[0], ts.shape[0]
    pts = V.pts_of(rays, ts)                                                          # [T,R,3] fp32
    tt = t_ray[None, :].expand(T, R)
    w = D.warp_ref(pts.reshape(-1, 3), tt.reshape(-1), ctrl, rig, spline, grid_radius)
    raw, b_raw = lookup_ref(w["warped"], w["b_warped"], densities, rgb, grid_radius)
    raw, b_raw = raw.reshape(T, R, 4), b_raw.reshape(T, R, 4)
    dp, r = w["dp"].reshape(T, R, 3), w["rigidity"].reshape(T, R)
    b_dp, b_r = w["b_dp"].reshape(T, R, 3), w["b_rigidity"].reshape(T, R)
    slope = SLOPE[act]
    colour = O.sigmoid(act)(raw[..., 1:])
    err_c = slope * b_raw[..., 1:] + EPS_COLOUR * (colour.abs() + 0.02)
    dirs = rays[:, 3:].double()
    zero = torch.zeros(T, R, 1, dtype=torch.float64)
    ref = CR.composite_ref(raw[..., 0], colour, ts.double(), dirs, "softplus", bg)
    v = raw[..., 0] - 1
    amp = torch.sigmoid(v) / torch.nn.functional.softplus(v).clamp(min=1e-300)
    eps_sigma = CR.EPS_SOFTPLUS + (b_raw[..., 0] + U * v.abs()) * amp
    fb = CR.forward_bounds(ref, eps_sigma, colour, err_c, bg)
    out = dict(rgb=ref["out"], b_rgb=fb["out"], alpha=ref["alpha"], b_alpha=fb["alpha"], weights=ref["weights"], b_weights=fb["weights"],
               dp=dp, rig=r)
    wgt = ref["weights"]
    rdp = dp * r[..., None]
    ones = torch.ones(T, R, 1, dtype=torch.float64)
    ones[-1] = 0
    feats = dict(depth=(ts.double()[:, None, None].expand(T, R, 1), zero), acc=(ones, zero),
                 flow=(rdp, r.abs()[..., None] * b_dp + dp.abs() * b_r[..., None] + U * rdp.abs()), rigidity=(r[..., None], b_r[..., None]))
    for name, (feat, err) in feats.items():
        black = dict(ref, out=(wgt[..., None] * feat).sum(dim=0))
        out[name] = black["out"]
        out["b_" + name] = CR.forward_bounds(black, eps_sigma, feat, err, "black")["out"]
    bad = ~torch.isfinite(pts.double()).all(dim=-1).all(dim=0)                         # a non-finite coordinate: the whole ray is NaN
    if bool(bad.any()):
        for k in OUTPUTS:
            out[k] = out[k].clone()
            if k in PER_SAMPLE:
                out[k][:, bad] = float("nan")
            else:
                out[k][bad] = float("nan")
    return out


def reference_maps(weights, ts, dp, rigidity):
    """the reference's own maps (runner.py:894-916) from a forward's arrays in THEIR dtype: volumetric_integrate(weights, other) =
    sum(weights[..., None] * other, dim=0) with other = ts, dp * rigidity, rigidity, and acc = weights[:-1].sum(0)"""
    shape = (-1,) + (1,) * weights.dim()
    vi = lambda other: (weights[..., None] * other).sum(dim=0)
    return dict(depth=vi(ts.to(weights.dtype).reshape(shape)), flow=vi(dp * rigidity), rigidity=vi(rigidity),
                acc=weights[:-1].sum(dim=0).unsqueeze(-1))


def fixture_ref(g):
    """render_ref of a g25 fixture's case, reshaped to the model's [B,H,W,.] (alpha / weights [T,B,H,W])"""
    from conftest import golden_params
    p = golden_params(g)
    rays = g["rays"]
    batch = tuple(rays.shape[:-1])
    t_ray = g["times"][:, None, None].expand(batch)
    ref = render_ref(rays.reshape(-1, 6), t_ray.reshape(-1), g["ts"], p["canonical.densities"], p["canonical.rgb"], p["ctrl_pts_grid"],
                     p["rigidity_grid"], int(g["spline"]), float(g["grid_radius"]), str(g["act"]), str(g["bg"]))
    out = {}
    for k, v in ref.items():
        lead = 2 if k.replace("b_", "") in PER_SAMPLE else 1        # [T, R, ...] or [R, ...]
        out[k] = v.reshape(tuple(v.shape[:lead - 1]) + batch + tuple(v.shape[lead:]))
    return out
