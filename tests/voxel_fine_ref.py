"""fp64 restatement of NeRFVoxel's coarse -> fine passes (csrc/voxel_fine.hip; `--voxel-steps-fine`) AT GIVEN STEPS, and the
bounds the GPU tests hold the kernels to.  The feature has no counterpart in the reference: the pins are the operators' own references,
composed -- the lookup of tests/voxel_ref.py (`cells`: membership fixed in fp32, `sample_ref`; the heads' forms in voxel_plv_ref /
voxel_sh_ref, both built on it) and tests/composite_ref.py's `composite_ref` over per-ray steps.  The resampled rows are INPUTS (taken from
na_resample_ts, which its own tests pin): the fp32 bin decisions stay out of the comparison, and no gradient flows through a position.

  proposal   positions o + ts[t] d in fp32 (a multiply, then an add), density lookup, composite_ref over the shared row (black background)
  fine pass  positions o + ts_ray[r, t] d in fp32, lookup of both grids, the head, the activation, composite_ref over the rays' own rows

THE BOUNDS are the two modules' own, chained to first order (u = 2^-24):
  density    |dd| <= voxel_ref.sample_bound(mag).  sigma = softplus(d - 1) then carries the relative error
                 eps_sigma = EPS_SOFTPLUS + (u |d - 1| + |dd|) sigmoid(d - 1) / softplus(d - 1)
             (composite_ref.eps_sigma_of with the lookup's absolute error next to the one of the fp32 difference, taken as always inexact)
  colours    a colour parameter p carries |dp| <= the head's sample bound; every activation of ops.SIGMOID is 1-Lipschitz and is evaluated
             with libm (expf, tanhf, sinf: 2 ulp) and at most four more roundings and two additive constants of 1e-2:
                 err_c = |dp| + EPS_ACT (|c| + 0.03),  EPS_ACT = 10 u
             pos-linear-view: c = act(p) scale(s), scale = sigmoid(s) / 2 + 0.5 in [0.5, 1], |scale'| <= 1/8, |ds| <= sh_bound:
                 err_c = scale (|dp| + EPS_ACT (|act| + 0.03)) + |act| (|ds| / 8 + EPS_ACT scale) + u |c|
  image      composite_ref.forward_bounds(ref, eps_sigma, colours, err_c): alpha, weights, out
  gradients  the grids' gradients are the lookup's scatter of g_raw = dL/d[density | colour parameters] per sample.  With g_raw exact the
             scatter is inside <module>.scatter_bound(ref, mag, cnt, det); the kernels' g_raw is composite_rayts_backward's and the
             activation's backward, whose errors b_raw (composite_ref.backward_bounds on the eps_sigma above, plus the colours' own error
             carried through G and V, plus the activation's chain factor: |act''| <= 1, EPS_CHAIN = 16 u) reach an entry as
             sum |w_u| b_raw: the scatter of b_raw's magnitudes, which <module>.scatter_ref returns as `mag` of the bound rows.
"""
import torch

import composite_ref as CR
import oracle as O
import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

U = V.U
EPS_ACT = 10.0 * U
EPS_CHAIN = 16.0 * U
HEADS = ("rgb", "plv", "sh")


def channels(head, order):
    return 3 if head == "rgb" else P.channels(order) if head == "plv" else H.channels(order)


def pts_rayts(rays, ts_ray):
    """o + t d over per-ray steps as na_compute_pts_rayts and the render kernels form it in fp32: rays [R,6], ts_ray [R,M] -> [M,R,3]"""
    assert rays.dtype == torch.float32 and ts_ray.dtype == torch.float32
    return rays[None, :, :3] + ts_ray.t().contiguous()[..., None] * rays[None, :, 3:]


def lookup(head, order, pts, dirs, den, rgb, grid_radius=V.GRID_RADIUS):
    """pts [N,3] fp32 (sample n belongs to ray n % R) -> raw [N,4] = [density | 3 colour parameters], mag [N,4], s [N] or None, mag_s"""
    if head == "rgb":
        raw, mag = V.sample_ref(pts, den, rgb, grid_radius)
        return raw, mag, None, None
    if head == "plv":
        return P.sample_ref(pts, dirs, den, rgb, grid_radius)
    raw, mag = H.sample_ref(pts, dirs, den, rgb, order, grid_radius)
    return raw, mag, None, None


def raw_bound(head, order, mag):
    return V.sample_bound(mag) if head != "sh" else H.sample_bound(mag, order)


def colours(head, raw, s, act):
    c = O.sigmoid(act)(raw[..., 1:])
    return c * (torch.sigmoid(s)[..., None] / 2 + 0.5) if head == "plv" else c


def colour_err(head, order, raw, mag, s, mag_s, act):
    a = O.sigmoid(act)(raw[..., 1:]).abs()
    dp = raw_bound(head, order, mag)[..., 1:]
    if head != "plv":
        return dp + EPS_ACT * (a + 0.03)
    scale = (torch.sigmoid(s) / 2 + 0.5)[..., None]
    ds = P.sh_bound(mag_s, order)[..., None]
    return scale * (dp + EPS_ACT * (a + 0.03)) + a * (ds / 8 + EPS_ACT * scale) + U * a * scale


def eps_sigma(density, b_density, libm=False):
    v = density - 1
    amp = torch.sigmoid(v) / torch.nn.functional.softplus(v).clamp(min=1e-300)
    return (CR.EPS_SOFTPLUS_LIBM if libm else CR.EPS_SOFTPLUS) + (U * v.abs() + b_density) * amp


def proposal_ref(rays, ts, den, grid_radius=V.GRID_RADIUS):
    """rays [R,6], ts [T] fp32, den [S,S,S,1] -> (composite_ref dict over the shared row: alpha, weights [T,R]; bounds dict)"""
    R, T = rays.shape[0], ts.shape[0]
    pts = V.pts_of(rays, ts)
    zero = torch.zeros(den.shape[:3] + (3,), dtype=den.dtype)
    raw, mag = V.sample_ref(pts.reshape(-1, 3), den, zero, grid_radius)
    d = raw[:, 0].reshape(T, R)
    feat = torch.zeros(T, R, 3, dtype=torch.float64)
    ref = CR.composite_ref(d, feat, ts.double(), rays[:, 3:].double(), "softplus", "black")
    return ref, CR.forward_bounds(ref, eps_sigma(d.detach(), V.sample_bound(mag[:, 0]).reshape(T, R)), feat)


def fine_ref(rays, ts_ray, den, rgb, head="rgb", order=-1, act="upshifted", bg="black", rand=None, grid_radius=V.GRID_RADIUS):
    """rays [R,6], ts_ray [R,M] fp32, the two grids (fp32, or fp64 leaves for autograd) -> dict: comp (composite_ref's dict: out [R,3],
    alpha, weights [M,R], ...), density [M,R], feat [M,R,3], raw [N,4], s, and the lookup's magnitudes"""
    R, M = ts_ray.shape
    pts = pts_rayts(rays, ts_ray)
    raw, mag, s, mag_s = lookup(head, order, pts.reshape(-1, 3), rays[:, 3:].contiguous(), den, rgb, grid_radius)
    if raw.requires_grad:
        raw.retain_grad()
        if s is not None:
            s.retain_grad()
    feat = colours(head, raw, s, act).reshape(M, R, 3)
    if feat.requires_grad:
        feat.retain_grad()
    d = raw[:, 0].reshape(M, R)
    comp = CR.composite_ref(d, feat, ts_ray.double(), rays[:, 3:].double(), "softplus", bg, None if rand is None else rand.double())
    return dict(comp=comp, density=d, feat=feat, raw=raw, s=s, mag=mag, mag_s=mag_s, pts=pts, head=head, order=order, act=act, bg=bg, rand=rand)


def fine_bounds(f):
    """per-element bounds of alpha, weights [M,R] and out [R,3] of a fine_ref dict (module docstring)"""
    M, R = f["density"].shape
    raw, mag = f["raw"].detach(), f["mag"].detach()
    s, mag_s = (None, None) if f["s"] is None else (f["s"].detach(), f["mag_s"].detach())
    eps = eps_sigma(f["density"].detach(), raw_bound(f["head"], f["order"], mag)[:, 0].reshape(M, R))
    err_c = colour_err(f["head"], f["order"], raw, mag, s, mag_s, f["act"]).reshape(M, R, 3)
    comp = {k: v.detach() for k, v in f["comp"].items()}
    return CR.forward_bounds(comp, eps, f["feat"].detach(), err_c=err_c, bg=f["bg"], rand=f["rand"])


def _act_derivs(raw_p, act):
    """|act'| and a bound of |act''| (<= 1 for every kind of ops.SIGMOID) at the colour parameters, fp64"""
    p = raw_p.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(O.sigmoid(act)(p).sum(), p)
    return g.abs(), torch.ones_like(g)


def fine_grads(rays, ts_ray, den, rgb, head, order, act, bg, det, rand=None, grid_radius=V.GRID_RADIUS):
    """loss = sum(out^2) of the fine pass at the given rows: (g_densities [S^3], g_rgb [S^3, C]) by fp64 autograd and their per-entry bounds
    (module docstring).  The proposal contributes nothing: its weights are constants."""
    S = den.shape[0]
    dl, rl = den.double().clone().requires_grad_(True), rgb.double().clone().requires_grad_(True)
    f = fine_ref(rays, ts_ray, dl, rl, head, order, act, bg, rand, grid_radius)
    out = f["comp"]["out"]
    (out ** 2).sum().backward()
    g_den, g_rgb = dl.grad.reshape(S ** 3), rl.grad.reshape(S ** 3, -1)
    M, R = f["density"].shape
    raw, mag = f["raw"].detach(), f["mag"].detach()
    g_raw = f["raw"].grad.detach()                                  # [N,4]
    g_out = (2 * out).detach()
    comp = {k: v.detach() for k, v in f["comp"].items()}
    density, feat = f["density"].detach(), f["feat"].detach()
    s, mag_s = (None, None) if f["s"] is None else (f["s"].detach(), f["mag_s"].detach())
    b_dn = raw_bound(head, order, mag)
    eps = eps_sigma(density, b_dn[:, 0].reshape(M, R), libm=True)
    # g_out is the forward's own output: its error is forward_bounds' (fast transcendentals there), doubled
    fb = CR.forward_bounds(comp, eps_sigma(density, b_dn[:, 0].reshape(M, R)), feat,
                           err_c=colour_err(head, order, raw, mag, s, mag_s, act).reshape(M, R, 3), bg=bg, rand=rand)
    d_go = 2 * fb["out"] + U * g_out.abs()
    b_d, b_f = CR.backward_bounds(comp, eps, density.float(), feat, g_out, "softplus", bg, rand)
    # ... the colours' and g_out's own errors through G_t = sum_c g_c c_tc (- the sky's share) and V (composite_ref's recurrence)
    err_c = colour_err(head, order, raw, mag, s, mag_s, act).reshape(M, R, 3)
    x, e, a, fq, Pq = comp["x"], comp["e"], comp["alpha"], comp["f"], comp["P"]
    dG = (err_c * g_out.abs()[None]).sum(-1) + ((feat.abs() + 1) * d_go[None]).sum(-1)
    dV = torch.zeros_like(x)
    for t in range(M - 1, 0, -1):
        dV[t - 1] = dG[t] * a[t] + fq[t] * dV[t]
    v = density - 1
    K = comp["dist"] * e * torch.sigmoid(v)
    b_d = b_d + Pq * (dG + dV) * K * (1 + 64 * U)
    b_f = b_f + comp["weights"][..., None] * d_go[None]
    # ... and the head's backward: g_p = g_feat act'(p) (times the linear scale), g_s = sum_c g_feat_c act(p_c) scale'(s)
    g_feat = f["feat"].grad.detach()
    d1, d2 = _act_derivs(raw[:, 1:], act)
    d1, d2 = d1.reshape(M, R, 3), d2.reshape(M, R, 3)
    dp = b_dn[:, 1:].reshape(M, R, 3)
    if head == "plv":
        sc = (torch.sigmoid(s) / 2 + 0.5).reshape(M, R, 1)
        dsc = (torch.sigmoid(s) * (1 - torch.sigmoid(s)) / 2).reshape(M, R, 1)
        ds = P.sh_bound(mag_s, order).reshape(M, R, 1)
        act_v = O.sigmoid(act)(raw[:, 1:]).reshape(M, R, 3)
        b_p = b_f * d1 * sc + g_feat.abs() * (d2 * dp * sc + d1 * dsc * ds + EPS_CHAIN * d1 * sc)
        b_s = (b_f * act_v.abs() * dsc + g_feat.abs() * (d1 * dp * dsc + act_v.abs() * ds / 8 + EPS_CHAIN * act_v.abs() * dsc)).sum(-1)
    else:
        b_p = b_f * d1 + g_feat.abs() * (d2 * dp + EPS_CHAIN * d1)
        b_s = None
    b_raw = torch.cat([b_d[..., None], b_p], dim=-1).reshape(-1, 4)
    pts, dirs = f["pts"].reshape(-1, 3), rays[:, 3:].contiguous()
    if head == "rgb":
        ref, mg, cnt = V.scatter_ref(pts, g_raw, S, grid_radius)
        bound = V.scatter_bound(ref, mg, cnt, det) + V.scatter_ref(pts, b_raw, S, grid_radius)[1]
    elif head == "plv":
        g_s = f["s"].grad.detach()
        ref, mg, cnt = P.scatter_ref(pts, dirs, g_raw, g_s, S, order, grid_radius)
        bound = P.scatter_bound(ref, mg, cnt, det) + P.scatter_ref(pts, dirs, b_raw, b_s.reshape(-1), S, order, grid_radius)[1]
    else:
        ref, mg, cnt = H.scatter_ref(pts, dirs, g_raw, S, order, grid_radius)
        bound = H.scatter_bound(ref, mg, cnt, det) + H.scatter_ref(pts, dirs, b_raw, S, order, grid_radius)[1]
    # the scatter references restate the autograd result entry by entry
    assert torch.allclose(ref[:, 0], g_den, rtol=1e-9, atol=1e-12) and torch.allclose(ref[:, 1:], g_rgb, rtol=1e-9, atol=1e-12)
    return ref, bound
