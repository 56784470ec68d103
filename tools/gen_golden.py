#!/usr/bin/env python3
"""Generate tests/golden/*.npz by running the REAL reference (/root/reference) on CPU.

Runs only in the build container (the reference never travels to the GPU box).  What is
committed are small fixtures: inputs + expected outputs (+ parameter name/shape lists so the
tests can regenerate the procedural weights with oracle/procedural.py).  No reference source
is copied; the reference modules are imported in-process with the shims of SURVEY.md App. A.

    python tools/gen_golden.py            # rewrites every fixture
"""
import os
import sys
import types
import math

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.procedural import proc_param, proc_uniform  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden")
REF = "/root/reference"


# ------------------------------------------------------------------ shims
def _stub(name, subs=()):
    m = types.ModuleType(name)
    m.__path__ = []
    sys.modules[name] = m
    for s in subs:
        sm = types.ModuleType(f"{name}.{s}")
        sm.__path__ = []
        sys.modules[f"{name}.{s}"] = sm
        setattr(m, s, sm)


_stub("torchvision", ["models", "transforms", "io"])
_tf = types.ModuleType("torchvision.transforms.functional")
sys.modules["torchvision.transforms.functional"] = _tf
sys.modules["torchvision.transforms"].functional = _tf
_stub("imageio")
sys.path.insert(0, REF)
import src.nerf as rnerf  # noqa: E402
import src.utils as rutils  # noqa: E402
import src.cameras as rcam  # noqa: E402
import src.neural_blocks as rnb  # noqa: E402
import src.refl as rrefl  # noqa: E402
import src.sdf as rsdf  # noqa: E402

nn.Module.cuda = lambda self, *a, **k: self
rnerf.with_transmission = False
rutils.git_hash = lambda: "nogit"
torch.set_grad_enabled(False)
torch.set_num_threads(8)


def save(name, **kw):
    out = {}
    for k, v in kw.items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.1f} KiB")


def fill_procedural(module: nn.Module, sigma_by_suffix=None):
    """Overwrite every parameter/buffer with oracle.procedural.proc_param(name, shape).
    Returns (names, shapes) in state_dict order."""
    names, shapes = [], []
    sd = module.state_dict()
    for name, t in sd.items():
        if name.endswith("primes") or t.numel() == 0:
            continue
        if name == "scale" or name.endswith(".scale"):
            continue  # VolSDF beta stays at its init (0.1)
        v = torch.from_numpy(proc_param(name, tuple(t.shape)))
        if name.endswith("basis"):
            sigma = 16.0 if "sdf" in name or "underlying" in name else 32.0
            if sigma_by_suffix is not None:
                sigma = sigma_by_suffix
            v = v * sigma
        t.copy_(v.to(t.dtype))
        names.append(name)
        shapes.append(list(t.shape))
    return names, shapes


def spec(names, shapes):
    flat = []
    for s in shapes:
        flat.append(",".join(str(d) for d in s))
    return dict(param_names=np.array(names), param_shapes=np.array(flat))


POSES = torch.tensor([
    [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]],
    [[0.8, -0.36, 0.48, 1.9], [0.0, 0.8, 0.6, 2.4], [-0.6, -0.48, 0.64, 2.6]],
    [[-0.28, 0.0, -0.96, -3.8], [0.576, 0.8, -0.168, -0.7], [0.768, -0.6, -0.224, -0.9]],
], dtype=torch.float)


def cam(poses=POSES[:1], size=16, fov=0.6911):
    focal = 0.5 * size / math.tan(0.5 * fov)
    return rcam.NeRFCamera(cam_to_world=poses.clone(), focal=focal), focal


def ref_pixel_grid(size, crop):
    ii, jj = torch.meshgrid(torch.arange(size, dtype=torch.float), torch.arange(size, dtype=torch.float),
                            indexing="ij")
    positions = torch.stack([ii.transpose(-1, -2), jj.transpose(-1, -2)], dim=-1)
    t, l, h, w = crop
    return positions[t:t + h, l:l + w, :]


# ------------------------------------------------------------------ G1 cameras
def g1():
    size = 16
    c, focal = cam(POSES, size)
    crops = [(0, 0, 16, 16), (3, 5, 6, 7), (12, 12, 8, 8)]  # full, interior, ragged edge (slice clips)
    kw = dict(c2w=POSES, focal=np.float64(focal), size=size, crops=np.array(crops))
    for i, crop in enumerate(crops):
        pos = ref_pixel_grid(size, crop)
        kw[f"pos{i}"] = pos
        kw[f"rays{i}"] = c.sample_positions(pos, size=size, with_noise=False)
    # jittered rays: pin the global RNG draw order (u first, then v)
    torch.manual_seed(11)
    pos = ref_pixel_grid(size, crops[1])
    ru = torch.rand_like(pos[..., :1])
    rv = torch.rand_like(pos[..., :1])
    torch.manual_seed(11)
    kw["noise"] = torch.cat([ru, rv], dim=-1)
    kw["rays_noise"] = c.sample_positions(pos, size=size, with_noise=0.1)
    save("g1_nerf_camera", **kw)

    # DTU camera with synthetic pose/intrinsics
    size = 12
    pose = torch.eye(4).repeat(2, 1, 1)
    pose[0, :3, :4] = torch.tensor([[0.9, 0.1, -0.42, 0.5], [-0.05, 0.99, 0.12, -0.2], [0.43, -0.09, 0.9, -1.1]])
    pose[1, :3, :4] = torch.tensor([[0.6, -0.3, 0.74, -0.8], [0.2, 0.95, 0.22, 0.1], [-0.77, 0.02, 0.63, -0.9]])
    intr = torch.eye(4).repeat(2, 1, 1)
    intr[:, 0, 0] = 2892.0
    intr[:, 1, 1] = 2883.0
    intr[:, 0, 2] = 800.0
    intr[:, 1, 2] = 600.0
    intr[1, 0, 1] = 1.5
    d = rcam.DTUCamera(pose=pose.clone(), intrinsic=intr.clone())
    pos = ref_pixel_grid(size, (2, 1, 7, 9))
    save("g1_dtu_camera", pose=pose, intrinsic=intr, size=size, pos=pos,
         rays=d.sample_positions(pos, size=size))


# ------------------------------------------------------------------ G2 sampling
def g2():
    rays = torch.zeros(1, 2, 2, 6)
    kw = {}
    for tag, (near, far, T, lindisp) in {"lin": (2.0, 6.0, 16, False), "disp": (0.3, 1.8, 16, True),
                                         "lin128": (2.0, 6.0, 128, False)}.items():
        _, _, ts, _ = rnerf.compute_ts(rays, near, far, T, lindisp=lindisp)
        kw[f"ts_{tag}"] = ts
        kw[f"cfg_{tag}"] = np.array([near, far, T, int(lindisp)], dtype=np.float64)
    torch.manual_seed(5)
    rand = torch.rand(16)
    torch.manual_seed(5)
    _, _, ts, mids = rnerf.compute_ts(rays, 2.0, 6.0, 16, perturb=1.0)
    kw.update(rand=rand, ts_perturb=ts, mids=mids)
    c, focal = cam(POSES[1:2], 8)
    r = c.sample_positions(ref_pixel_grid(8, (0, 0, 8, 8)), size=8)
    pts, ts, r_o, r_d, _ = rnerf.compute_pts_ts(r, 2.0, 6.0, 16)
    kw.update(rays=r, pts=pts)
    save("g2_sampling", **kw)


# ------------------------------------------------------------------ G3 compositing
def g3():
    T, B, H, W = 16, 2, 3, 4
    density = torch.from_numpy(proc_uniform((T, B, H, W), 101, 4.0))
    density[3, 0, 0, 0] = 60.0  # saturating: alpha == 1
    density[5, 1, 2, 3] = 1e4
    density[7, 0, 1, 1] = -50.0
    rgb = torch.from_numpy(proc_uniform((T, B, H, W, 3), 102, 0.5)) + 0.5
    r_d = torch.from_numpy(proc_uniform((B, H, W, 3), 103, 1.0))
    ts = torch.linspace(2, 6, T)
    ts_zero = ts.clone()
    ts_zero[5] = ts_zero[4]  # zero-length interval -> clamp 1e-5
    kw = dict(density=density, rgb=rgb, r_d=r_d, ts=ts, ts_zero=ts_zero)
    for tag, (t, sp) in {"softplus": (ts, True), "relu": (ts, False), "zero": (ts_zero, True)}.items():
        alpha, weights = rnerf.alpha_from_density(density, t, r_d, softplus=sp)
        out = rnerf.volumetric_integrate(weights, rgb)
        kw[f"alpha_{tag}"] = alpha
        kw[f"weights_{tag}"] = weights
        kw[f"out_{tag}"] = out
        kw[f"white_{tag}"] = out + rnerf.white(None, weights)
    # KAT from SURVEY 8(c)
    a, w = rnerf.alpha_from_density(torch.tensor([0.5, 1, 2, -1.0]).reshape(4, 1, 1, 1), torch.linspace(2, 6, 4),
                                    torch.tensor([0, 0, -1.0]).reshape(1, 1, 1, 3))
    kw.update(kat_alpha=a.reshape(-1), kat_weights=w.reshape(-1))
    save("g3_composite", **kw)


# ------------------------------------------------------------------ G4 hash
def hash_inputs():
    x = torch.from_numpy(proc_uniform((61, 3), 201, 3.0))
    special = torch.tensor([[0.3, -1.7, 2.2], [0.0, 0.0, 0.0], [1.0, -1.0, 2.0], [-3.0, 3.0, -0.5],
                            [0.0625, -0.0625, 0.125], [5.99, -5.99, 4.0], [-40.0, 37.5, 55.25]])
    return torch.cat([special, x], dim=0)


def g4():
    enc = rnb.HashEncoder()
    names, shapes = fill_procedural(enc)
    x = hash_inputs()
    idx = []
    for i in range(enc.levels):
        N_l = enc.low_reso * (enc.scale ** i)
        l = (x * N_l).floor().long()
        lx, ly, lz = l.split([1, 1, 1], dim=-1)
        h = l + 1
        hx, hy, hz = h.split([1, 1, 1], dim=-1)
        cat = lambda a, b, c: torch.cat([a, b, c], dim=-1)
        vs = [l, cat(lx, ly, hz), cat(lx, hy, lz), cat(lx, hy, hz), cat(hx, ly, lz), cat(hx, ly, hz),
              cat(hx, hy, lz), h]
        idx.append(torch.stack([(enc.hash_fn(v) % enc.emb_size).squeeze(-1) for v in vs], dim=0))
    save("g4_hash", x=x, idx=torch.stack(idx, 0), feats=enc(x),
         resolutions=np.array([enc.low_reso * (enc.scale ** i) for i in range(enc.levels)], dtype=np.float64),
         **spec(names, shapes))


# ------------------------------------------------------------------ G5 fourier / positional
def g5():
    kw = {}
    for sigma in (16, 32):
        enc = rnb.FourierEncoder(input_dims=3, sigma=sigma)
        basis = torch.from_numpy(proc_param("basis", (3, 128))) * sigma
        enc.basis.copy_(basis)
        x = torch.from_numpy(proc_uniform((48, 3), 300 + sigma, 3.0))
        kw[f"x_{sigma}"] = x
        kw[f"out_{sigma}"] = enc(x)
        kw[f"out64_{sigma}"] = rutils.fourier(x.double(), basis.double())
    pe = rnb.PositionalEncoder(input_dims=3, max_freq=6.0, N=8)
    x = torch.from_numpy(proc_uniform((20, 3), 333, 2.0))
    kw.update(pe_x=x, pe_bands=pe.bands, pe_out=pe(x))
    save("g5_fourier", **kw)


# ------------------------------------------------------------------ G6 SkipConnMLP
MLP_CASES = {
    # tag: (in, enc, latent, layers, out, act, init)
    "tiny": (3, None, 0, 6, 4, "leaky_relu", "xavier"),
    "first": (3, "hash", 0, 4, 65, "leaky_relu", None),
    "view": (5, None, 64, 4, 3, "sin", "siren"),
    "posrefl": (3, "hash", 64, 5, 3, "leaky_relu", None),
    "delta6": (3, "hash", 0, 5, 19, "leaky_relu", "xavier"),
    "sdfmlp": (3, "fourier16", 0, 6, 65, "leaky_relu", "xavier"),
    "siren": (3, None, 0, 5, 65, "sin", "siren"),
    "mipfirst": (3, "hash", 96, 4, 65, "leaky_relu", None),
    "plv_view": (6, None, 128, 2, 1, "sin", "siren"),  # hidden 128
    "plv_pos": (3, "hash", 0, 2, 67, "leaky_relu", None),
}


def make_mlp(case):
    in_size, enc, latent, layers, out, act, init = MLP_CASES[case]
    e = None
    if enc == "hash":
        e = rnb.HashEncoder()
    elif enc == "fourier16":
        e = rnb.FourierEncoder(input_dims=in_size, sigma=16)
    hidden = 128 if case == "plv_view" else 256
    kwargs = dict(num_layers=layers, hidden_size=hidden, in_size=in_size, out=out, latent_size=latent, enc=e, init=init)
    if act == "sin":
        kwargs["activation"] = torch.sin
    return rnb.SkipConnMLP(**kwargs)


def g6():
    for case in MLP_CASES:
        in_size, enc, latent, layers, out, act, init = MLP_CASES[case]
        m = make_mlp(case)
        names, shapes = fill_procedural(m, sigma_by_suffix=16.0 if enc == "fourier16" else None)
        N = 40
        p = torch.from_numpy(proc_uniform((N, in_size), 400, 2.5))
        lat = torch.from_numpy(proc_uniform((N, latent), 401, 1.0)) if latent else None
        inter = []
        hooks = [m.init.register_forward_hook(lambda mod, i, o: inter.append(o.clone()))]
        for l in m.layers:
            hooks.append(l.register_forward_hook(lambda mod, i, o: inter.append(o.clone())))
        y = m(p, lat)
        for h in hooks:
            h.remove()
        kw = dict(p=p, y=y, act=act, enc=str(enc), layers=layers, out=out, latent_size=latent, **spec(names, shapes))
        if lat is not None:
            kw["latent"] = lat
        for i, t in enumerate(inter):
            kw[f"inter{i}"] = t
        save(f"g6_mlp_{case}", **kw)


# ------------------------------------------------------------------ G7 elaz + heads
def g7():
    d = torch.from_numpy(proc_uniform((29, 3), 500, 1.0))
    d = torch.cat([d, torch.tensor([[0, 0, 1.0], [0, 0, -1.0], [0, 0, -5.0], [1e-4, -1e-4, 3.0], [-0.08, 0.08, -1.0],
                                    [2.0, 0, 0], [0, -3.0, 0]])], dim=0)
    kw = dict(dirs=d, elaz=rutils.dir_to_elev_azim(d))
    v = torch.from_numpy(proc_uniform((33,), 501, 6.0))
    for k in ["normal", "thin", "fat", "tanh", "upshifted", "relu", "sin", "leaky_relu", "upshifted_softplus",
              "upshifted_relu", "cyclic"]:
        kw[f"sig_{k}"] = rutils.load_sigmoid(k)(v)
    kw["sig_in"] = v
    save("g7_elaz_sigmoid", **kw)
    N = 24
    x = torch.from_numpy(proc_uniform((N, 3), 510, 2.5))
    view = torch.from_numpy(proc_uniform((N, 3), 511, 1.0))
    lat = torch.from_numpy(proc_uniform((N, 64), 512, 1.0))
    for kind, cons in {"view": rrefl.View, "pos": rrefl.Positional, "pos-linear-view": rrefl.PosLinearView}.items():
        for act in (["thin", "upshifted"] if kind == "view" else ["thin"]):
            r = cons(latent_size=64, act=act, out_features=3)
            names, shapes = fill_procedural(r)
            save(f"g7_refl_{kind}_{act}", x=x, view=view, latent=lat, rgb=r(x=x, view=view, latent=lat), act=act,
                 **spec(names, shapes))


# ------------------------------------------------------------------ G8 mip primitives
def g8():
    x = torch.from_numpy(proc_uniform((10, 3), 600, 3.0))
    var = torch.from_numpy(proc_uniform((10, 3), 601, 0.5)).abs()
    y, yv = rutils.expected_sin(x, var)
    kw = dict(x=x, var=var, es_y=y, es_var=yv, ipe=rutils.integrated_pos_enc_diag(x, var, 0, 16))
    c, focal = cam(POSES[:2], 16)
    for i, crop in enumerate([(0, 0, 16, 16), (3, 5, 6, 7), (10, 2, 6, 9)]):
        rays = c.sample_positions(ref_pixel_grid(16, crop), size=16)
        kw[f"rd{i}"] = rays[..., 3:]
        kw[f"radii{i}"] = rutils.radii_x(rays[..., 3:])
    t0 = torch.linspace(2, 5.75, 16)
    t1 = t0 + 0.25
    rad = torch.tensor(0.003)
    # scalar moments, taken from the reference by probing lift_gaussian with a unit z direction:
    # mean_z = t_mean, cov_zz = t_var, cov_xx = r_var
    rd = torch.tensor([[0.0, 0.0, 1.0]])
    mean, cov = rutils.cylinder_to_gaussian(rd, t0, t1, rad)
    kw.update(t0=t0, t1=t1, rad=rad, cyl_tmean=mean[:, 0, 2], cyl_cov=cov)
    mean, cov = rutils.conical_frustrum_to_gaussian(rd, t0, t1, float(rad))
    kw.update(cone_tmean=mean[:, 0, 2], cone_cov=cov)
    save("g8_mip", **kw)


# ------------------------------------------------------------------ G9 bezier + D-NeRF
def g9():
    kw = {}
    t = torch.from_numpy(proc_uniform((7, 1), 700, 0.5)) + 0.5
    for n in range(2, 7):
        co = torch.from_numpy(proc_uniform((n, 7, 3), 701 + n, 1.0))
        kw[f"coeffs{n}"] = co
        kw[f"dc{n}"] = rnerf.de_casteljau(co, t, n)
    kw["cubic"] = rnerf.cubic_bezier(kw["coeffs4"], t, 4)
    kw["t"] = t
    save("g9_bezier", **kw)
    for spline in (6, 4):
        size, T = 6, 8
        canon = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
        m = rnerf.DynamicNeRF(canonical=canon, spline=spline)
        m.eval()
        names, shapes = fill_procedural(m)
        c, focal = cam(POSES[:2], size)
        rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
        times = torch.tensor([0.25, 0.8])
        out = m((rays, times))
        save(f"g9_dnerf_spline{spline}", rays=rays, times=times, out=out, steps=T, near=2.0, far=6.0,
             rigidity=m.rigidity, dp=m.dp, weights=canon.weights, **spec(names, shapes))
    # `make dnerf` as shipped (makefile:106-114): --spline 6 --dyn-refl-latent 3 --refl-kind pos-linear-view; + the View head and
    # the cubic spline with the same latent (runner.py:1169-1211 builds the head with latent_size = model.intermediate_size)
    for spline, kind, rl in ((6, "pos-linear-view", 3), (6, "view", 3), (4, "pos-linear-view", 2)):
        size, T = 6, 8
        canon = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
        m = rnerf.DynamicNeRF(canonical=canon, spline=spline, refl_latent=rl)
        m.set_refl(rrefl.refl_kinds[kind](latent_size=m.intermediate_size, act="upshifted", out_features=3))
        m.eval()
        names, shapes = fill_procedural(m)
        c, focal = cam(POSES[:2], size)
        rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
        times = torch.tensor([0.25, 0.8])
        captured = {}
        orig = canon.from_pts
        canon.from_pts = lambda pts, ts, r_o, r_d, enc=None: (captured.update(enc=enc), orig(pts, ts, r_o, r_d, enc))[1]
        out = m((rays, times))
        tag = {"pos-linear-view": "plv", "view": "view"}[kind]
        save(f"g9_dnerf_spline{spline}_rl{rl}_{tag}", rays=rays, times=times, out=out, steps=T, near=2.0, far=6.0,
             rigidity=m.rigidity, dp=m.dp, weights=canon.weights, refl_latent=captured["enc"], refl_kind=kind, n_rl=rl,
             **spec(names, shapes))


# ------------------------------------------------------------------ G10 laplace + VolSDF
def g10():
    s = torch.from_numpy(proc_uniform((40,), 800, 0.6))
    s[0] = 0.0
    kw = dict(sdf=s)
    for sc in (0.1, 0.02, 1.5):
        kw[f"cdf_{sc}"] = rutils.laplace_cdf(s, torch.tensor(sc))
    save("g10_laplace", **kw)
    for kind in ("mlp", "siren"):
        size, T = 6, 8
        under = rsdf.sdf_kinds[kind](intermediate_size=64)
        refl = rrefl.View(latent_size=64, act="upshifted", out_features=3)
        sdf = rsdf.SDF(under, refl, isect=None, t_near=0.3, t_far=1.8)
        m = rnerf.VolSDF(sdf=sdf, steps=T, t_near=0.3, t_far=1.8, sigmoid_kind="upshifted")
        m.eval()
        names, shapes = fill_procedural(m)
        c, focal = cam(POSES[:2], size)
        rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
        rays = torch.cat([rays[..., :3] * 0.2, torch.nn.functional.normalize(rays[..., 3:], dim=-1)], dim=-1)
        out = m(rays)
        save(f"g10_volsdf_{kind}", rays=rays, out=out, steps=T, near=0.3, far=1.8, scale=m.scale,
             weights=m.weights, alpha=m.alpha, **spec(names, shapes))


# ------------------------------------------------------------------ G11 PlainNeRF
def g11():
    for kind in ("view", "pos", "pos-linear-view"):
        for B in (1, 2):
            size, T = 6, 16
            m = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted",
                                bg="white" if B == 2 else "black")
            if kind != "view":
                r = rrefl.refl_kinds[kind](latent_size=64, act="upshifted", out_features=3)
                m.set_refl(r)
            m.eval()
            names, shapes = fill_procedural(m)
            c, focal = cam(POSES[:B], size)
            rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
            out = m(rays)
            save(f"g11_plain_{kind}_b{B}", rays=rays, out=out, steps=T, near=2.0, far=6.0,
                 bg="white" if B == 2 else "black", ts=m.ts, alpha=m.alpha, weights=m.weights, **spec(names, shapes))
    # fp64 tie-breaker for the headline model
    import copy
    m = rnerf.PlainNeRF(steps=16, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
    m.eval()
    names, shapes = fill_procedural(m)
    c, focal = cam(POSES[:1], 6)
    rays = c.sample_positions(ref_pixel_grid(6, (0, 0, 6, 6)), size=6)
    m64 = copy.deepcopy(m).double()
    save("g11_plain_view_fp64", rays=rays, out32=m(rays), out64=m64(rays.double()), **spec(names, shapes))


# ------------------------------------------------------------------ G12 tiled frame (runner.render + test()-style tiling)
def g12():
    import runner  # the reference's own render()
    runner.device = "cpu"
    size, T, cs = 20, 8, 8  # ragged: 20 = 8+8+4
    m = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
    m.eval()
    names, shapes = fill_procedural(m)
    c, focal = cam(POSES[1:2], size)
    args = types.SimpleNamespace(data_kind="original")
    got = torch.zeros(size, size, 3)
    n = math.ceil(size / cs)
    for x in range(n):
        c0 = x * cs
        for y in range(n):
            c1 = y * cs
            out, rays = runner.render(m, c, (c0, c1, cs, cs), size=size, with_noise=False, times=None, args=args)
            got[c0:c0 + cs, c1:c1 + cs, :] = out.squeeze(0)
    exp = torch.from_numpy(proc_uniform((size, size, 3), 1200, 0.5)) + 0.5
    mse = torch.nn.functional.mse_loss(got, exp)
    save("g12_tiled_frame", c2w=POSES[1:2], focal=np.float64(focal), size=size, steps=T, crop_size=cs, near=2.0, far=6.0,
         frame=got, exp=exp, psnr=rutils.mse2psnr(mse), **spec(names, shapes))


# ------------------------------------------------------------------ tiny (reference primitives composed)
def g13():
    size, T = 8, 8
    mlp = rnb.SkipConnMLP(in_size=3, out=4, num_layers=6, hidden_size=256, init="xavier")
    sd_names, sd_shapes = [], []
    for name, t in mlp.state_dict().items():
        full = "estim." + name
        t.copy_(torch.from_numpy(proc_param(full, tuple(t.shape))))
        sd_names.append(full)
        sd_shapes.append(list(t.shape))
    c, focal = cam(POSES[:1], size)
    rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
    pts, ts, r_o, r_d, _ = rnerf.compute_pts_ts(rays, 2.0, 6.0, T)
    o = mlp(pts)
    alpha, w = rnerf.alpha_from_density(o[..., 0], ts, r_d)
    out = rnerf.volumetric_integrate(w, rutils.upshifted_sigmoid(o[..., 1:]))
    save("g13_tiny", rays=rays, out=out, steps=T, near=2.0, far=6.0, weights=w, **spec(sd_names, sd_shapes))


# ------------------------------------------------------------------ G14 loaders (N2)
def g14():
    """Reference loaders (src/loaders.py:74-150) on the analytic scene of tools/make_scene.py, at the file size and
    through PIL's resize; labels stored as uint16 fixed point of the exact k/255 grid where possible."""
    import tempfile
    import src.loaders as rload
    from tools.make_scene import make_scene
    kw = {}
    with tempfile.TemporaryDirectory() as td:
        d = make_scene(os.path.join(td, "static"), size=24, n_train=4, n_test=2) + "/"
        for training in (True, False):
            for size in (24, 16):
                for white in (False, True):
                    labels, c, _ = rload.original(d, normalize=False, training=training, size=size, white_bg=white)
                    key = f"orig_{'train' if training else 'test'}_{size}_{'w' if white else 'b'}"
                    kw[key + "_labels"] = labels
                    kw[key + "_c2w"] = c.cam_to_world
                    kw[key + "_focal"] = np.float64(c.focal)
        labels, c, _ = rload.original(d, normalize=True, training=True, size=24, with_mask=True)
        kw["orig_norm_mask_labels"], kw["orig_norm_mask_c2w"] = labels, c.cam_to_world
        dd = make_scene(os.path.join(td, "dyn"), size=24, n_train=5, n_test=2, dynamic=True) + "/"
        # shuffle the frame order and stretch the times so that sorting and normalisation are exercised
        import json
        tf = json.load(open(dd + "transforms_train.json"))
        tf["frames"] = [tf["frames"][i] for i in (3, 0, 4, 1, 2)]
        for fr in tf["frames"]:
            fr["time"] = fr["time"] * 3.0 - 0.5
        json.dump(tf, open(dd + "transforms_train.json", "w"))
        for gamma in (False, True):
            (labels, times), c, _ = rload.dnerf(dd, training=True, size=24, time_gamma=gamma, white_bg=False)
            kw[f"dnerf_g{int(gamma)}_labels"], kw[f"dnerf_g{int(gamma)}_times"] = labels, times
            kw[f"dnerf_g{int(gamma)}_c2w"] = c.cam_to_world
        (labels, times), c, _ = rload.dnerf(dd, training=False, size=16, time_gamma=False, white_bg=True)
        kw["dnerf_test_labels"], kw["dnerf_test_times"], kw["dnerf_test_focal"] = labels, times, np.float64(c.focal)
    save("g14_loaders", **kw)


# ------------------------------------------------------------------ G15 SDF marching (N4)
def g15():
    """Reference src/march.py on (a) an analytic two-sphere SDF (pins the marching logic exactly) and (b) the reference
    SIREN SDF model with procedural weights (pins it through a network)."""
    import random
    import src.march as rmarch
    c2w = POSES[1:2]
    camr, _ = cam(c2w, 12)
    rays = camr.sample_positions(ref_pixel_grid(12, (0, 0, 12, 12)), size=12, with_noise=False)[0]
    r_o, r_d = rays[..., :3].contiguous(), torch.nn.functional.normalize(rays[..., 3:], dim=-1)

    def analytic(p):
        a = torch.linalg.norm(p - torch.tensor([0.1, -0.2, 0.0]), dim=-1) - 1.1
        b = torch.linalg.norm(p - torch.tensor([0.9, 0.6, 0.3]), dim=-1) - 0.5
        return torch.minimum(a, b).unsqueeze(-1)
    siren = rsdf.SIREN(intermediate_size=0)
    names, shapes = fill_procedural(siren)
    kw = dict(r_o=r_o, r_d=r_d, **spec(names, shapes))
    for tag, fn, near, far in (("an", analytic, 1.0, 6.0), ("nn", siren, 0.5, 5.0)):
        pts, hits, dist, _ = rmarch.sphere_march(fn, r_o, r_d, iters=24, eps=1e-3, near=near, far=far)
        kw.update({f"{tag}_sm_pts": pts, f"{tag}_sm_hits": hits, f"{tag}_sm_dist": dist})
        random.seed(7)
        jit = random.random()
        random.seed(7)
        tput, best, lastp, firstn = rmarch.throughput_with_sign_change(fn, r_o, r_d, near, far, batch_size=40)
        kw.update({f"{tag}_tp": tput, f"{tag}_best": best, f"{tag}_last": lastp, f"{tag}_first": firstn})
        random.seed(7)
        pts, hits, best2, tput2 = rmarch.bisect(fn, r_o, r_d, iters=40, near=near, far=far)
        kw.update({f"{tag}_bi_pts": pts, f"{tag}_bi_hits": hits, f"{tag}_bi_tput": tput2})
        kw[f"{tag}_near"], kw[f"{tag}_far"] = np.float64(near), np.float64(far)
    kw["jitter"] = np.float64(jit)
    save("g15_march", **kw)


# ------------------------------------------------------------------ G16 occlusion models (N4)
def g16():
    """Reference src/renderers.py:29-163 occlusion kinds over a src/lights.py Point light and the reference SIREN SDF's
    intersect_mask (src/sdf.py:123-135), all with procedural weights; points on a [2,6,8] grid, some masked out."""
    import random
    import src.renderers as rrend
    import src.lights as rlights
    siren = rsdf.SIREN(intermediate_size=0)
    names, shapes = fill_procedural(siren)
    sdf = rsdf.SDF(siren, rrefl.View(latent_size=0), None, t_near=0.5, t_far=5.0)
    sdf.eval()
    # the procedural SIREN is negative somewhere along every ray: lift its output bias so about half the points see the light
    shift = 0.9
    siren.siren.out.bias.data += shift
    light0 = rlights.Point(center=[1.5, 2.0, -1.0], intensity=[30.0])
    light = next(iter(light0.iter()))  # how src/renderers.py:198 hands lights to the occlusion model
    gen = torch.Generator().manual_seed(16)
    pts = torch.rand(2, 6, 8, 3, generator=gen) * 2.4 - 1.2
    mask = torch.rand(2, 6, 8, generator=gen) > 0.25
    kw = dict(pts=pts, mask=mask, sdf_out_bias_shift=np.float64(shift), center=light.center.detach(), intensity=light.intensity.detach(),
              sdf_param_names=np.array(names), sdf_param_shapes=np.array([",".join(map(str, sh)) for sh in shapes]))
    seen = {}

    def isect(r_o, r_d, near=None, far=None, eps=1e-3):
        vis, tput, _ = sdf.intersect_mask(r_o, r_d, near=near, far=far, eps=eps)
        seen["tput"], seen["far"] = tput, far
        return vis, tput, None
    cases = [("hard", True, {}), ("learned", True, {}), ("learned-const", False, {}),
             ("all-learned", True, {"all_learned_occ_kind": "pos-elaz"}), ("all-learned-pos", False, {"all_learned_occ_kind": "pos"}),
             ("joint-all-const", False, {})]
    for tag, use_mask, extra in cases:
        kind = "all-learned" if tag.startswith("all-learned") else tag
        args = types.SimpleNamespace(occ_kind=kind, **extra)
        occ = rrend.load_occlusion_kind(args, kind, 0)
        occ.eval()
        onames, oshapes = fill_procedural(occ, sigma_by_suffix=4.0)
        for n_, p_ in occ.named_parameters():
            if n_.endswith("alpha"):
                p_.data.fill_(0.3)
        seen.clear()
        random.seed(16)
        d, s = occ(pts, light, isect, mask=mask if use_mask else None, latent=None)
        t = tag.replace("-", "_")
        kw.update({f"{t}_dir": d, f"{t}_spectrum": s, f"{t}_param_names": np.array(onames),
                   f"{t}_param_shapes": np.array([",".join(map(str, sh)) for sh in oshapes])})
        if "tput" in seen:
            kw[f"{t}_tput"], kw[f"{t}_far"] = seen["tput"], np.float64(seen["far"])
        if hasattr(occ, "all_learned_occ"):
            kw[f"{t}_raw_att"] = occ.all_learned_occ.raw_att
    random.seed(16)
    kw["jitter"] = np.float64(random.random())
    # no-shadow lighting (src/renderers.py:29-31)
    d, s = rrend.lighting_wo_isect(pts, light, None, mask=mask)
    kw["none_dir"], kw["none_spectrum"] = d, s
    save("g16_occlusion", **kw)


# ------------------------------------------------------------------ G17 FFJORD divergence estimate (N1)
def g17():
    """Reference utils.div_approx (src/utils.py:467-478) on DynamicNeRF.rigid_dp exactly as runner.py:697-700 calls it:
    training-mode forward (perturbed samples, pts.requires_grad_()), e = randn_like(rigid_dp).  The estimate carries no
    graph (torch.autograd.grad without create_graph): `term_requires_grad` records that the loss term is a constant."""
    size, T, spline = 6, 8, 6
    canon = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
    m = rnerf.DynamicNeRF(canonical=canon, spline=spline)
    m.train()
    names, shapes = fill_procedural(m)
    c, focal = cam(POSES[:2], size)
    rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
    times = torch.tensor([0.25, 0.8])
    with torch.enable_grad():
        torch.manual_seed(17)
        out = m((rays, times))
        torch.manual_seed(18)
        div = rutils.div_approx(m.pts, m.rigid_dp)
        torch.manual_seed(18)
        e = torch.randn_like(m.rigid_dp)
        term = (m.canonical.alpha.detach() * div.abs().square()).mean()
    save("g17_ffjord", rays=rays, times=times, pts=m.pts, e=e, div=div, rigid_dp=m.rigid_dp, alpha=m.canonical.alpha,
         term=term, term_requires_grad=np.bool_(term.requires_grad), steps=T, near=2.0, far=6.0, **spec(names, shapes))


# ------------------------------------------------------------------ G18 auxiliary maps (N3: runner.py:511-538, 894-913)
def g18():
    """The reference's OWN visualisation functions on the last forward of DynamicNeRF(spline 6): runner.depth_vis / flow_vis /
    rigidity_vis (runner.py:511-538) and the raw maps of the test() loop (runner.py:894-913), utils.depth_to_normals
    (src/utils.py:421-427).  `depth_vis` as written divides by `(args.far - args.near).clamp(min=0, max=1)` -- the clamp binds
    to the denominator and only exists for tensors -- so it is called with tensor near / far chosen such that far - near = 1,
    where the written expression and the evident intent ((raw - near) / (far - near), clamped to [0, 1]) coincide wherever
    the result lies in [0, 1]; the fixture keeps the raw map too."""
    import argparse
    import runner as rrunner
    size, T, spline = 6, 8, 6
    canon = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted")
    m = rnerf.DynamicNeRF(canonical=canon, spline=spline)
    m.eval()
    names, shapes = fill_procedural(m)
    c, focal = cam(POSES[:2], size)
    rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
    times = torch.tensor([0.25, 0.8])
    out = m((rays, times))
    w = canon.weights
    raw_depth = rnerf.volumetric_integrate(w, canon.ts[:, None, None, None, None])
    args = argparse.Namespace(near=torch.tensor(2.5), far=torch.tensor(3.5), normals_from_depth=True)
    dvis = rrunner.depth_vis(m, args)
    fvis = rrunner.flow_vis(m, args)
    rvis = rrunner.rigidity_vis(m, args)
    save("g18_aux_maps", rays=rays, times=times, out=out, steps=T, near=2.0, far=6.0, vis_near=2.5, vis_far=3.5,
         weights=w, raw_depth=raw_depth, depth_vis=dvis[0], depth_normal_vis=dvis[1],
         depth_normals=rutils.depth_to_normals(raw_depth[0]),
         flow_raw=rnerf.volumetric_integrate(w, m.rigid_dp), flow_vis=fvis[0],
         rigidity_raw=rnerf.volumetric_integrate(w, m.rigidity), rigidity_vis=rvis[0],
         acc=w[:-1].sum(dim=0), **spec(names, shapes))


# ------------------------------------------------------------------ G19 --bg random (src/nerf.py:99-103)
def g19():
    """PlainNeRF(view) with bg = "random": one uniform draw PER RAY (rand_like of the [..., 1] remainder), broadcast over the
    colour channels, times 1 - sum(weights[:-1]).  The draw is replayed from the same seed and stored (the Q13 convention:
    stochastic inputs are explicit tensors on the build's side)."""
    size, T = 6, 8
    m = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind="upshifted", bg="random")
    m.eval()
    names, shapes = fill_procedural(m)
    c, focal = cam(POSES[:2], size)
    rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
    torch.manual_seed(19)
    out = m(rays)
    summed = 1 - m.weights[:-1].sum(dim=0).unsqueeze(-1)
    torch.manual_seed(19)
    rand = torch.rand_like(summed)
    m.set_bg("black")
    out_black = m(rays)
    assert torch.allclose(out, out_black + rand * summed, atol=1e-6)
    # the bare function on synthetic weights (g3's)
    g3w = rnerf.alpha_from_density(torch.from_numpy(proc_uniform((16, 2, 3, 4), 101, 4.0)), torch.linspace(2, 6, 16),
                                   torch.from_numpy(proc_uniform((2, 3, 4, 3), 103, 1.0)))[1]
    torch.manual_seed(20)
    sky = rnerf.random_color(None, g3w)
    torch.manual_seed(20)
    rand3 = torch.rand_like(sky)
    save("g19_bg_random", rays=rays, out=out, out_black=out_black, rand=rand, steps=T, near=2.0, far=6.0,
         fn_weights=g3w, fn_rand=rand3, fn_sky=sky, **spec(names, shapes))


# ------------------------------------------------------------------ G20 spherical-harmonic colour head (src/refl.py:696-731)
SH_KINDS = ["normal", "thin", "fat", "tanh", "upshifted", "relu", "sin", "leaky_relu", "upshifted_softplus", "upshifted_relu",
            "cyclic", "identity"]  # nerf_atlas_amd.ops.SIGMOID; "identity" = eval_sh itself (the reference has no such key)
SH_GRAD_ROWS = 8   # the gradient is recorded for the first rows only (the special directions + 4 random): file size


def g20():
    """g20_sh_eval: act(eval_sh(deg, coeffs, normalize(dirs))) of the reference in fp32 and fp64 for degrees 0..4 and every activation
    kind, + the gradient of sum(out * probe) w.r.t. the coefficients in fp32 and fp64 (first SH_GRAD_ROWS directions).  Coefficients
    [257, 3 K] and probe [257, 3] are proc_uniform(shape, seed, 1.0) of the stored seeds.
    g20_plain_sph-har_o{0..4}: the g11 recipe with the sph-har head, fp32 and fp64.  g20_plain_sph-har_grads: order 2, fp64 gradients."""
    import copy
    import src.spherical_harmonics as rsh
    F = torch.nn.functional
    act_of = lambda k: (lambda v: v) if k == "identity" else rutils.load_sigmoid(k)
    n = 257
    dirs = torch.from_numpy(proc_uniform((n, 3), 2001, 1.5)).float()
    dirs[0] = torch.tensor([0.0, 0.0, 2.0])      # both poles
    dirs[1] = torch.tensor([0.0, 0.0, -0.5])
    dirs[2] = torch.tensor([1.5, 0.0, 0.0])      # axis-aligned
    dirs[3] = torch.tensor([0.0, 0.7, -0.3])     # zero x
    kw = dict(dirs=dirs, kinds=np.array(SH_KINDS), grad_rows=SH_GRAD_ROWS)
    for deg in range(5):
        K = (deg + 1) ** 2
        co = torch.from_numpy(proc_uniform((n, 3 * K), 2010 + deg, 1.0)).float()
        probe = torch.from_numpy(proc_uniform((n, 3), 2020 + deg, 1.0)).float()
        # (not stored: the test regenerates both with oracle.procedural.proc_uniform from these seeds)
        kw[f"coeffs_seed{deg}"], kw[f"probe_seed{deg}"] = 2010 + deg, 2020 + deg
        for dt, tag in ((torch.float32, "32"), (torch.float64, "64")):
            outs, grads = [], []
            for kind in SH_KINDS:
                with torch.enable_grad():
                    c = co.detach().to(dt).clone().requires_grad_()
                    o = act_of(kind)(rsh.eval_sh(deg, c.reshape(n, 3, K), F.normalize(dirs.to(dt), dim=-1)))
                    (o * probe.to(dt)).sum().backward()
                outs.append(o.detach())
                grads.append(c.grad[:SH_GRAD_ROWS].clone())
            kw[f"out{tag}_{deg}"] = torch.stack(outs)
            kw[f"grad{tag}_{deg}"] = torch.stack(grads)
    save("g20_sh_eval", **kw)

    size, T = 6, 16
    recipe = [("upshifted", "black"), ("normal", "black"), ("leaky_relu", "white"), ("thin", "black"), ("upshifted", "black")]
    c, focal = cam(POSES[:2], size)
    rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
    for order, (act, bg) in enumerate(recipe):
        m = rnerf.PlainNeRF(steps=T, t_near=2.0, t_far=6.0, intermediate_size=64, sigmoid_kind=act, bg=bg)
        m.set_refl(rrefl.refl_kinds["sph-har"](latent_size=64, act=act, out_features=3, order=order))
        m.eval()
        names, shapes = fill_procedural(m)
        out = m(rays)
        ts, alpha, weights = m.ts, m.alpha, m.weights
        m64 = copy.deepcopy(m).double()
        out64 = m64(rays.double())
        dev, devw = float((out.double() - out64).abs().max()), float((weights.double() - m64.weights).abs().max())
        print(f"g20 order {order} ({act}/{bg}): |out - out64| {dev:.2e}, |weights - weights64| {devw:.2e}")
        assert dev <= 5e-5, dev  # a fixture whose fp32 value is itself noisy is never written
        save(f"g20_plain_sph-har_o{order}", rays=rays, out=out, out64=out64, steps=T, near=2.0, far=6.0, bg=bg, act=act, order=order,
             ts=ts, alpha=alpha, alpha64=m64.alpha, weights=weights, weights64=m64.weights, **spec(names, shapes))
        if order == 2:
            keys = ["refl.mlp.out.weight", "refl.mlp.out.bias", "refl.mlp.layers.3.weight", "refl.mlp.init.weight", "first.out.weight"]
            # a weighted MEAN (|loss| < 1): a sum over 216 entries could not be compared to 1e-6 absolute in fp32
            probe = torch.from_numpy(proc_uniform(tuple(out.shape), 2030, 1.0)).double() / out.numel()
            with torch.enable_grad():
                for p_ in m64.parameters():
                    p_.requires_grad_(p_.is_floating_point())
                loss = (m64(rays.double()) * probe).sum()
                loss.backward()
            named = dict(m64.named_parameters())
            save("g20_plain_sph-har_grads", rays=rays, probe=probe, loss=loss.detach(), steps=T, near=2.0, far=6.0, bg=bg, act=act,
                 order=order, grad_names=np.array(keys), **{"grad_" + k: named[k].grad.float() for k in keys},
                 **spec(names, shapes))


AE_CASES = {  # name: (E, I, B, crop (t, l, h, w) of the 6 x 6 frame, bg, act, normalize_latent)
    "e32_i32_black": (32, 32, 1, (0, 0, 6, 6), "black", "thin", False),
    "e32_i32_white": (32, 32, 1, (0, 0, 6, 6), "white", "upshifted", False),
    "e32_i32_norm": (32, 32, 1, (0, 0, 6, 6), "black", "thin", True),
    "e16_i32": (16, 32, 1, (0, 0, 6, 6), "black", "thin", False),
    "e32_i64": (32, 64, 2, (2, 0, 3, 5), "black", "thin", False),                # B = 2; the CLI default width, head latent 96
    "e32_i32_ragged": (32, 32, 1, (0, 1, 5, 5), "white", "thin", False),   # 25 rays: not a multiple of 32
    "e64_i32_ragged": (64, 32, 1, (1, 0, 5, 6), "black", "normal", True),  # 30 rays
}
AE_GRAD_CAP = 6000  # entries kept per gradient tensor (whole rows, evenly spaced): keeps the fixture inside the committed-file limit


def _ae_build(E, I, bg, act, norm, T=16):
    m = rnerf.NeRFAE(steps=T, t_near=2.0, t_far=6.0, intermediate_size=I, encoding_size=E, normalize_latent=norm, sigmoid_kind=act, bg=bg)
    m.eval()
    names, shapes = fill_procedural(m)
    return m, names, shapes


def _ae_parts(m, rays):
    """(out, encoded as the head sees it, first_out, alpha, weights) of the reference class, through its own methods"""
    out = m(rays)
    pts, ts, r_o, r_d, _ = rnerf.compute_pts_ts(rays, m.t_near, m.t_far, m.steps)
    enc = m.compute_encoded(pts, ts, r_o, r_d).reshape(pts.shape[:-1] + (-1,))
    if m.normalize_latent: enc = torch.nn.functional.normalize(enc, dim=-1)
    return out, enc, m.density_tform(enc), m.alpha, m.weights, ts


def g21():
    """g21_ae_{case}: the reference's NeRFAE (src/nerf.py:766-840) constructed directly, procedural weights (Fourier basis at sigma 32),
    eval mode, steps 16, near 2 / far 6, in fp32 AND fp64: encoded (after normalisation where on), first_out, out, alpha, weights.
    g21_ae_grad: training mode, density noise off, the stratified steps `ts` of one seeded draw stored; loss = mse(out, target) + 0.1 *
    latent_l2_loss and its fp64 gradient w.r.t. EVERY parameter -- per tensor the L2 norm of the whole gradient and evenly spaced whole
    rows of it (at most AE_GRAD_CAP entries: two full sets would be 4 MB)."""
    import copy
    size = 6
    for name, (E, I, B, crop, bg, act, norm) in AE_CASES.items():
        c, focal = cam(POSES[:B], size)
        rays = c.sample_positions(ref_pixel_grid(size, crop), size=size)
        m, names, shapes = _ae_build(E, I, bg, act, norm)
        out, enc, fo, alpha, weights, ts = _ae_parts(m, rays)
        m64 = copy.deepcopy(m).double()
        out64, enc64, fo64, alpha64, weights64, _ = _ae_parts(m64, rays.double())
        opac = weights64[:-1].sum(0)
        frac = float(((opac > 0.05) & (opac < 0.95)).float().mean())
        print(f"g21 {name}: opacity before the last sample {float(opac.min()):.2f}..{float(opac.max()):.2f} ({frac:.0%} of rays in 0.05..0.95); "
              f"fp32 vs fp64: out {float((out.double() - out64).abs().max()):.2e} weights {float((weights.double() - weights64).abs().max()):.2e} "
              f"encoded {float((enc.double() - enc64).abs().max()):.2e} first_out {float((fo.double() - fo64).abs().max()):.2e}")
        assert frac >= 0.5, f"{name}: degenerate case (the 1e-4 bar would test nothing)"
        save(f"g21_ae_{name}", rays=rays, E=E, I=I, steps=16, near=2.0, far=6.0, bg=bg, act=act, normalize=int(norm), ts=ts,
             encoded=enc, encoded64=enc64, first_out=fo, first_out64=fo64, out=out, out64=out64, alpha=alpha, alpha64=alpha64,
             weights=weights, weights64=weights64, **spec(names, shapes))
    kw = {}
    for name in ("e32_i32_black", "e32_i32_norm"):
        E, I, B, crop, bg, act, norm = AE_CASES[name]
        c, focal = cam(POSES[:B], size)
        rays = c.sample_positions(ref_pixel_grid(size, crop), size=size)
        m, names, shapes = _ae_build(E, I, bg, act, norm)
        m.train()
        m.noise_std = 0
        m.set_regularize_latent()
        target = torch.from_numpy(proc_uniform(tuple(rays.shape[:-1]) + (3,), 2101, 0.5)).double() + 0.5

        def step(mm, dt, pts, ts, r_o, r_d):
            with torch.enable_grad():
                for p_ in mm.parameters():
                    p_.requires_grad_(p_.is_floating_point() and p_ is not mm.encode.enc.basis)
                out = mm.from_pts(pts.to(dt), ts.to(dt), r_o.to(dt), r_d.to(dt))
                mse = torch.nn.functional.mse_loss(out, target.to(dt))
                loss = mse + 0.1 * mm.latent_l2_loss
                loss.backward()
            return out.detach(), mse.detach(), loss.detach()
        # The stratified draw decides which pre-activations sit within fp32 rounding of a LeakyReLU kink; one such sample moves a
        # gradient summed over 576 samples by ~1/576 whatever computes it in fp32 (seed 2100: the reference's OWN fp32 autograd is
        # 2.2e-3 of the largest entry off its fp64 run on encode.init.weight).  Such a draw measures the kink, not an implementation:
        # the first seed from 2100 on is taken at which the reference's fp32 gradients are within 1.25e-4 (a quarter of the fp32 bar
        # of tests/test_gpu_backward.py) of its fp64 gradients on every tensor.
        for seed in range(2100, 2110):
            torch.manual_seed(seed)
            pts, ts, r_o, r_d, _ = rnerf.compute_pts_ts(rays, m.t_near, m.t_far, m.steps, perturb=1)
            m32, m64 = copy.deepcopy(m), copy.deepcopy(m).double()
            _, _, loss32 = step(m32, torch.float32, pts, ts, r_o, r_d)
            out, mse, loss = step(m64, torch.float64, pts, ts, r_o, r_d)
            g32 = dict(m32.named_parameters())
            own = max(float((g32[k].grad.double() - p_.grad).abs().max() / p_.grad.abs().max()) for k, p_ in m64.named_parameters() if p_.grad is not None)
            print(f"g21 grad {name}: seed {seed}: the reference's fp32 gradients are {own:.2e} of the largest entry off its fp64 gradients")
            if own <= 1.25e-4:
                break
        else:
            raise AssertionError("no usable stratified draw in ten seeds")
        gnames = [k for k, p_ in m64.named_parameters() if p_.grad is not None]
        missing = [k for k, p_ in m64.named_parameters() if p_.grad is None]
        assert missing == ["empty_latent", "encode.enc.basis"], f"every parameter but the zero-size latent and the fixed Fourier basis has a gradient: {missing}"
        kw.update({f"{name}.rays": rays, f"{name}.ts": ts, f"{name}.ts_seed": seed, f"{name}.target_seed": 2101, f"{name}.loss": loss.detach(), f"{name}.loss32": loss32.detach(), f"{name}.mse": mse.detach(),
                   f"{name}.latent_l2": m64.latent_l2_loss.detach(), f"{name}.out64": out.detach(), f"{name}.grad_names": np.array(gnames)})
        named = dict(m64.named_parameters())
        for k in gnames:
            g = named[k].grad
            g2 = g.reshape(g.shape[0], -1)
            stride = max(1, -(-g2.numel() // AE_GRAD_CAP))
            kw[f"{name}.grad.{k}"] = g2[::stride].float()
            kw[f"{name}.stride.{k}"] = stride
            kw[f"{name}.norm.{k}"] = g.norm()
        for k, v in spec(names, shapes).items():
            kw[f"{name}.{k}"] = v
        print(f"g21 grad {name}: loss {float(loss):.6f} (mse {float(mse):.6f}, latent l2 {float(m64.latent_l2_loss):.6f}; the fp32 run: {float(loss32):.7f}, {abs(float(loss32) - float(loss)):.2e} off), {len(gnames)} gradients")
    save("g21_ae_grad", **kw)


# ------------------------------------------------------------------ G22 Fourier position gradient + D-NeRF over VolSDF(mlp)
FG_N = 257        # rows per encoder case (the GPU test takes the leading N of them: 1 .. 257)
DVS_GRAD_CAP = 1000  # entries kept per gradient tensor and precision (evenly spaced over the flattened tensor; hash tables: over the touched entries)
DVS_BETA = 0.7
# (no `--dyn-refl-latent` case: the reference cannot run one over VolSDF -- VolSDF.from_pts drops `refl_latent` (src/nerf.py:995-1013) while
# runner.py:1182-1183 builds the head for intermediate_size + refl_latent columns: "shape '[-1, 67]' is invalid" in the first forward)
DVS_CASES = {"view_s4": ("view", 4, 0), "plv_s6": ("pos-linear-view", 6, 0)}


def _dvs_build(kind, spline, rl, T):
    under = rsdf.sdf_kinds["mlp"](intermediate_size=64)
    sdf = rsdf.SDF(under, rrefl.View(latent_size=64, act="upshifted", out_features=3), isect=None, t_near=0.3, t_far=1.8)
    canon = rnerf.VolSDF(sdf=sdf, steps=T, t_near=0.3, t_far=1.8, sigmoid_kind="upshifted")
    m = rnerf.DynamicNeRF(canonical=canon, spline=spline, refl_latent=rl)
    # runner.py:1182-1183: the head's latent is model.intermediate_size wide (the canonical model's + --dyn-refl-latent)
    m.set_refl(rrefl.refl_kinds[kind](latent_size=m.intermediate_size, act="upshifted", out_features=3))
    m.eval()
    names, shapes = fill_procedural(m)  # (delta_estim.out included: the warp is live)
    # beta = 0.7 instead of the initial 0.1: the procedural SDF is -2.3 .. -0.3 on these samples, which saturates the Laplace CDF at
    # beta = 0.1 (d density / d sdf = 0: the position gradient would reach the deformation through the colour alone)
    canon.scale.fill_(DVS_BETA)
    return m, names, shapes


def g22():
    """g22_fourier_grad: the reference's FourierEncoder (src/neural_blocks.py:36-55, src/utils.py:14-17) under torch autograd, fp64 AND
    fp32: gx = d(sum(enc(x) * g))/dx for F in {128, 4, 6} x D in {1, 2, 3} x extra_scale in {1, 1.5} x sigma in {16, 32}, |x| <= 6.  Inputs
    are shared between the cases (x{D}, g{F}, basis_{sigma}_{D}_{F}); gx64.<case> / gx32.<case> per case.
    g22_dnerf_volsdf_<case>: DynamicNeRF(VolSDF(sdf.MLP)) (`make dnerf_volsdf`, makefile:127-133) constructed directly, procedural weights
    (delta_estim.out non-zero), eval mode, 2 views x 4 x 4 rays x 8 steps, fp64 AND fp32: out, alpha, weights, dp, rigidity, the l2 loss
    against a procedural target and its gradient w.r.t. every parameter (at most DVS_GRAD_CAP entries per tensor, their flat indices,
    the whole tensor's norm / largest entry and the fp32 run's own deviation from the fp64 run)."""
    import copy
    kw = dict(scales=np.array([1.0, 1.5]), sigmas=np.array([16, 32]), Fs=np.array([128, 4, 6]), Ds=np.array([1, 2, 3]))
    for D in (1, 2, 3):
        kw[f"x{D}"] = torch.from_numpy(proc_uniform((FG_N, D), 2200 + D, 6.0))
    for F_ in (128, 4, 6):
        kw[f"g{F_}"] = torch.from_numpy(proc_uniform((FG_N, 2 * F_), 2210 + F_, 1.0))
    worst = 0.0
    for F_ in (128, 4, 6):
        for D in (1, 2, 3):
            for sigma in (16, 32):
                basis = torch.from_numpy(proc_param("basis", (D, F_))) * sigma
                kw[f"basis_{sigma}_{D}_{F_}"] = basis
                for scale in (1.0, 1.5):
                    res = {}
                    for dt in (torch.float64, torch.float32):
                        enc = rnb.FourierEncoder(input_dims=D, freqs=F_, sigma=sigma)
                        enc.basis.copy_(basis)
                        enc = enc.to(dt)
                        enc.extra_scale = scale
                        with torch.enable_grad():
                            x = kw[f"x{D}"].to(dt).clone().requires_grad_()
                            (gx,) = torch.autograd.grad(enc(x), x, kw[f"g{F_}"].to(dt))
                        res[dt] = gx
                    tag = f"F{F_}_D{D}_s{scale}_sig{sigma}"
                    kw[f"gx64.{tag}"], kw[f"gx32.{tag}"] = res[torch.float64], res[torch.float32]
                    worst = max(worst, float((res[torch.float32].double() - res[torch.float64]).abs().max() / res[torch.float64].abs().max()))
    print(f"g22 fourier_grad: the reference's fp32 gx is at most {worst:.2e} of the largest entry off its fp64 gx")
    save("g22_fourier_grad", **kw)

    size, T = 4, 8
    for name, (kind, spline, rl) in DVS_CASES.items():
        m, names, shapes = _dvs_build(kind, spline, rl, T)
        c, focal = cam(POSES[:2], size)
        rays = c.sample_positions(ref_pixel_grid(size, (0, 0, size, size)), size=size)
        rays = torch.cat([rays[..., :3] * 0.2, torch.nn.functional.normalize(rays[..., 3:], dim=-1)], dim=-1)
        target = torch.from_numpy(proc_uniform(tuple(rays.shape[:-1]) + (3,), 2201, 0.5)).double() + 0.5

        def run(dt, times):
            mm = copy.deepcopy(m).to(dt)
            with torch.enable_grad():
                for k, p_ in mm.named_parameters():
                    p_.requires_grad_(p_.is_floating_point() and not k.endswith("basis"))
                out = mm((rays.to(dt), times.to(dt)))
                loss = torch.nn.functional.mse_loss(out, target.to(dt))
                loss.backward()
            return dict(out=out.detach(), loss=loss.detach(), alpha=mm.canonical.alpha.detach(), weights=mm.canonical.weights.detach(),
                        dp=mm.dp.detach(), rigidity=mm.rigidity.detach(), grads={k: p_.grad for k, p_ in mm.named_parameters()})
        # Frame times 0.25 / 0.8, the ones of the g9 D-NeRF fixtures, for every case: no draw is picked.  Where the warped samples land
        # decides which LeakyReLU pre-activations of the SDF network sit within fp32 rounding of the kink (its later layers hold ~70 of
        # 65 536 within 2e-5 each in the fp64 run) and which samples sit on a hash-cell face, and one flip moves a gradient summed over
        # 256 samples by 1 / 256 and more, whatever computes it in fp32.  The reference's OWN fp32 autograd against its fp64 run, the
        # worst tensor in units of its largest entry, goes into the fixture as `own_linf` (view_s4: 3.2e-5; plv_s6: 5.2e-2, it flips):
        # the ruler tests/test_gpu_fourier_grad.py derives its fp32 bar from, on exactly the inputs it runs.
        times = torch.tensor([0.25, 0.8])
        r64, r32 = run(torch.float64, times), run(torch.float32, times)
        opac = r64["weights"][:-1].sum(0)
        frac = float(((opac > 0.05) & (opac < 0.95)).float().mean())
        print(f"g22 {name}: opacity before the last sample {float(opac.min()):.2f}..{float(opac.max()):.2f} ({frac:.0%} of rays in 0.05..0.95), "
              f"|dp| up to {float(r64['dp'].abs().max()):.3f}; fp32 vs fp64: out {float((r32['out'].double() - r64['out']).abs().max()):.2e} "
              f"loss {abs(float(r32['loss']) - float(r64['loss'])):.2e}")
        assert frac >= 0.5, f"{name}: degenerate case"
        gnames = [k for k, g in r64["grads"].items() if g is not None]
        missing = [k for k, g in r64["grads"].items() if g is None]
        kw = dict(rays=rays, times=times, steps=T, near=0.3, far=1.8, spline=spline, n_rl=rl, refl_kind=kind, target_seed=2201,
                  scale=DVS_BETA, grad_names=np.array(gnames), no_grad_names=np.array(missing), **spec(names, shapes))
        for k in ("out", "alpha", "weights", "dp", "rigidity", "loss"):
            kw[k], kw[k + "64"] = r32[k], r64[k]
        own_linf = own_l2 = 0.0
        for k in gnames:
            g64, g32 = r64["grads"][k].reshape(-1), r32["grads"][k].reshape(-1)
            pool = torch.nonzero(g64).reshape(-1).numpy() if "embs" in k else np.arange(g64.numel())
            idx = pool[::max(1, -(-len(pool) // DVS_GRAD_CAP))].astype(np.int64)
            kw[f"idx.{k}"] = idx.astype(np.int32)
            kw[f"grad64.{k}"] = g64[idx]
            kw[f"grad32.{k}"] = g32[idx]
            kw[f"norm64.{k}"] = g64.norm()
            kw[f"max64.{k}"] = g64.abs().max()
            linf = float((g32.double() - g64).abs().max() / g64.abs().max().clamp_min(1e-300))
            l2 = float((g32.double() - g64).norm() / g64.norm().clamp_min(1e-300))
            kw[f"own_linf.{k}"], kw[f"own_l2.{k}"] = linf, l2
            if float(g64.abs().max()) > 0:
                own_linf, own_l2 = max(own_linf, linf), max(own_l2, l2)
        kw["own_linf"], kw["own_l2"] = own_linf, own_l2
        print(f"g22 {name}: loss {float(r64['loss']):.6f}, {len(gnames)} gradients (none: {missing}); the reference's fp32 gradients are at most "
              f"{own_linf:.2e} (of the largest entry) / {own_l2:.2e} (relative L2) per tensor off its fp64 gradients")
        save(f"g22_dnerf_volsdf_{name}", **kw)


VOXEL_CASES = {  # name: (S, T, ray batch shape, act, bg)
    "s64_black": (64, 64, (2, 4, 4), "upshifted", "black"),
    "s64_white": (64, 64, (2, 4, 4), "thin", "white"),
    "s16_ragged": (16, 24, (1, 5, 7), "leaky_relu", "black"),
    "s4": (4, 16, (2, 4, 4), "upshifted", "white"),
    "s2": (2, 7, (2, 4, 4), "thin", "black"),
}


def _voxel_build(S, T, act, bg, head=None):
    """the reference's NeRFVoxel + Positional (or the head class given) constructed directly (its runner wiring is dead: DESIGN.md 7),
    procedural grids"""
    m = rnerf.NeRFVoxel(resolution=S, t_near=2.0, t_far=6.0, steps=T)
    m.set_refl((head or rrefl.Positional)(act=act, latent_size=0, out_features=3))
    m.set_bg(bg)
    m.eval()
    names, shapes = fill_procedural(m)
    return m, names, shapes


def g23(prefix="g23_voxel_", head=None, cases=None):
    """g23_voxel_<case>: the reference's NeRFVoxel (src/nerf.py:401-524) with the per-voxel Positional head, eval mode, near 2 / far 6,
    generic rays (tests/voxel_ref.py generic_rays: origins on the radius-4 sphere, so the first samples of every ray are extrapolated),
    in fp32 AND fp64: out, alpha, weights and the reference's own fp32 - fp64 deviation.  A case whose two precisions disagree by more
    than 1e-5 pins nothing (a sample on a cell-membership plane): the next seed is taken.  S <= 16 also stores the fp64 gradients of
    densities and rgb for loss = sum(out^2) (and how far the reference's own fp32 gradients are from them, `g_dev`), and the reference's fp32 neighbor_ids and xyz (the argument of its trilinear_weights) on
    the lattice point set (voxel_ref.lattice_points), which the fixture carries."""
    import copy
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import voxel_ref as V
    tag = prefix.split("_")[0]
    for name, (S, T, shape, act, bg) in VOXEL_CASES.items():
        if cases is not None and name not in cases:
            continue
        m, names, shapes = _voxel_build(S, T, act, bg, head)
        m64 = copy.deepcopy(m).double()
        for seed in range(4500, 4600, 2):
            rays = V.generic_rays(shape, seed)
            out, alpha, weights, ts = m(rays), m.alpha, m.weights, m.ts
            out64, alpha64, weights64 = m64(rays.double()), m64.alpha, m64.weights
            dev = {k: float((a.double() - b).abs().max()) for k, a, b in (("out", out, out64), ("alpha", alpha, alpha64), ("weights", weights, weights64))}
            if max(dev.values()) <= 1e-5:
                break
            print(f"{tag} {name}: seed {seed} skipped, the reference's fp32 and fp64 disagree by {max(dev.values()):.2e}")
        else:
            raise AssertionError(f"{tag} {name}: no seed on which the reference agrees with itself")
        opac = weights64[:-1].sum(0)
        print(f"{tag} {name}: seed {seed}, opacity before the last sample {float(opac.min()):.2f}..{float(opac.max()):.2f}; fp32 vs fp64: "
              + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        kw = dict(rays=rays, S=S, steps=T, near=2.0, far=6.0, act=act, bg=bg, grid_radius=m.grid_radius, seed=seed, ts=ts,
                  out=out, out64=out64, alpha=alpha, alpha64=alpha64, weights=weights, weights64=weights64,
                  dev=np.array([dev["out"], dev["alpha"], dev["weights"]]), **spec(names, shapes))
        if S <= 16:
            with torch.enable_grad():
                for p_ in m64.parameters(): p_.requires_grad_(True)
                m64(rays.double()).square().sum().backward()
            with torch.enable_grad():
                for p_ in m.parameters(): p_.requires_grad_(True)
                m(rays).square().sum().backward()
            g_dev = [float((a.grad.double() - b.grad).abs().max() / b.grad.abs().max()) for a, b in ((m.densities, m64.densities), (m.rgb, m64.rgb))]
            print(f"{tag} {name}: the reference's fp32 gradients are {g_dev[0]:.2e} (densities) / {g_dev[1]:.2e} (rgb) of the largest entry off its fp64 ones")
            kw.update(g_densities64=m64.densities.grad, g_rgb64=m64.rgb.grad, g_dev=np.array(g_dev))
            lat = V.lattice_points(S, m.grid_radius)
            seen, orig = [], rnerf.trilinear_weights
            rnerf.trilinear_weights = lambda xyzs: (seen.append(xyzs), orig(xyzs))[1]
            try:
                ids, _ = m.grid_coords_trilin_weights(lat)
            finally:
                rnerf.trilinear_weights = orig
            assert ids.dtype == torch.int64 and seen[0].dtype == torch.float32
            kw.update(lat_pts=lat, lat_ids=ids, lat_xyz=seen[0])
        save(f"{prefix}{name}", **kw)


GRID_TV_CASES = {
    # name: (grid shape, samples, seed of the grid's proc_uniform values, torch seed of the draw)
    "462x5": ((4, 6, 2, 5), 257, 5501, 11),    # non-cubic: pins x = idx % s0 against the memory order
    "6x3": ((6, 6, 6, 3), 1000, 5502, 12),     # more samples than voxels: duplicates
    "8x1": ((8, 8, 8, 1), 64, 5503, 13),
}


def g24():
    """g24_grid_tv_<case>: the reference's total_variation (src/nerf.py:381-399) on a grid of proc_uniform values in +-1 (regenerated by
    the tests from `grid_seed`): the indices it drew (the seed replayed through the same torch.randint call, checked against its
    random_sample_grid), its fp32 value, and its value and gradient on the `.double()` grid.  Data only."""
    for name, (shape, n, grid_seed, seed) in GRID_TV_CASES.items():
        grid = torch.from_numpy(proc_uniform(shape, grid_seed, 1.0))
        n_elem = shape[0] * shape[1] * shape[2]
        torch.manual_seed(seed)
        value = rnerf.total_variation(grid, n)
        torch.manual_seed(seed)
        idxs = torch.randint(0, n_elem, (n,))
        torch.manual_seed(seed)
        x, y, z = rnerf.random_sample_grid(grid, n)
        assert torch.equal(x, idxs % shape[0]) and torch.equal(z, idxs // (shape[0] * shape[1]) % shape[2]) and idxs.dtype == torch.int64
        with torch.enable_grad():
            g64 = grid.double().requires_grad_(True)
            torch.manual_seed(seed)
            value64 = rnerf.total_variation(g64, n)
            value64.backward()
        assert value.dtype == torch.float32 and value64.dtype == torch.float64
        print(f"g24 {name}: value {float(value):.7f} (fp32) {float(value64):.12f} (fp64), {len(set(idxs.tolist()))} distinct of {n} indices")
        save(f"g24_grid_tv_{name}", shape=np.array(shape), samples=n, grid_seed=grid_seed, seed=seed, idxs=idxs, value=value,
             value64=value64, grad64=g64.grad)


DYN_VOXEL_CASES = {  # name: (S, spline, T, ray batch shape [B, H, W], times [B], act, bg)
    "s2_n2": (2, 2, 7, (2, 4, 4), (0.0, 1.0), "thin", "black"),
    "s4_n4": (4, 4, 16, (3, 4, 4), (0.0, 0.6, 1.0), "upshifted", "white"),
    "s16_n5_ragged": (16, 5, 24, (2, 5, 7), (0.25, 0.8), "leaky_relu", "black"),
    "s16_n11": (16, 11, 24, (2, 4, 4), (0.3, 0.9), "upshifted", "black"),
    "s64_n4": (64, 4, 64, (2, 4, 4), (0.25, 0.8), "upshifted", "black"),  # forward only
}
DYN_VOXEL_GRADS = ("canonical.densities", "canonical.rgb", "ctrl_pts_grid", "rigidity_grid")


def g25(prefix="g25_dyn_voxel_", head=None, cases=None):
    """g25_dyn_voxel_<case>: the reference's DynamicNeRFVoxel (src/nerf.py:1526-1586) over its NeRFVoxel + Positional, all three built
    directly (load_dyn's own call is a TypeError: DESIGN.md 7), eval mode, near 2 / far 6, procedural grids (stored as specs; proc_param
    fills rigidity_grid too, so the rigidity is not the constant 1/2 of the zero init), voxel_ref.generic_rays and 2-3 times per batch,
    in fp32 AND fp64: out, alpha, weights, dp, rigidity and the reference's own fp32 - fp64 deviation.  g23's rule: a seed on which
    the two precisions disagree by more than 1e-5 pins nothing and is skipped; no agreeing seed is an error.  S <= 16 also stores the
    fp64 gradients of the four grids for loss = sum(out^2) and how far the reference's own fp32 gradients are from them (`g_dev`, in units
    of the largest fp64 entry, in DYN_VOXEL_GRADS' order)."""
    import copy
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import voxel_ref as V
    tag = prefix.split("_")[0]
    for name, (S, spline, T, shape, times, act, bg) in (cases or DYN_VOXEL_CASES).items():
        canon, _, _ = _voxel_build(S, T, act, bg, head)
        m = rnerf.DynamicNeRFVoxel(canon, spline=spline)
        m.eval()
        names, shapes = fill_procedural(m)
        m64 = copy.deepcopy(m).double()
        t = torch.tensor(times, dtype=torch.float32)
        keys = ("out", "alpha", "weights", "dp", "rigidity")

        def run(model, dt, rays):
            out = model((rays.to(dt), t.to(dt)))
            return dict(out=out, alpha=model.canonical.alpha, weights=model.canonical.weights, dp=model.dp, rigidity=model.rigidity)
        for seed in range(4500, 4600, 2):
            rays = V.generic_rays(shape, seed)
            r32, r64 = run(m, torch.float32, rays), run(m64, torch.float64, rays)
            dev = {k: float((r32[k].double() - r64[k]).abs().max()) for k in keys}
            if max(dev.values()) <= 1e-5:
                break
            print(f"{tag} {name}: seed {seed} skipped, the reference's fp32 and fp64 disagree by {max(dev.values()):.2e}")
        else:
            raise AssertionError(f"{tag} {name}: no seed on which the reference agrees with itself")
        opac = r64["weights"][:-1].sum(0)
        print(f"{tag} {name}: seed {seed}, opacity before the last sample {float(opac.min()):.2f}..{float(opac.max()):.2f}, |dp| up to "
              f"{float(r64['dp'].abs().max()):.2f}, rigidity {float(r64['rigidity'].min()):.2f}..{float(r64['rigidity'].max()):.2f}; "
              "fp32 vs fp64: " + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        kw = dict(rays=rays, times=t, S=S, spline=spline, steps=T, near=2.0, far=6.0, act=act, bg=bg, grid_radius=canon.grid_radius, seed=seed,
                  ts=m.ts, dev=np.array([dev[k] for k in keys]), **spec(names, shapes))
        for k in keys:
            kw[k], kw[k + "64"] = r32[k], r64[k]
        if S <= 16:
            for model, dt in ((m64, torch.float64), (m, torch.float32)):
                with torch.enable_grad():
                    for p_ in model.parameters(): p_.requires_grad_(True)
                    model((rays.to(dt), t.to(dt))).square().sum().backward()
            g32, g64 = dict(m.named_parameters()), dict(m64.named_parameters())
            g_dev = [float((g32[k].grad.double() - g64[k].grad).abs().max() / g64[k].grad.abs().max()) for k in DYN_VOXEL_GRADS]
            print(f"{tag} {name}: the reference's fp32 gradients are " + " / ".join(f"{v:.2e}" for v in g_dev)
                  + " of the largest entry off its fp64 ones (densities, rgb, ctrl_pts_grid, rigidity_grid)")
            kw.update(g_dev=np.array(g_dev), **{"grad64." + k: g64[k].grad for k in DYN_VOXEL_GRADS})
        save(f"{prefix}{name}", **kw)


SPLINE_LEN_CASES = {  # name: (S, spline, T, ray batch shape [1, H, W], time, indices of the grid term, act, bg)
    "s2_n2": (2, 2, 7, (1, 4, 4), 0.0, 63, "thin", "black"),               # grid term: one control point per voxel, every length 0
    "s4_n4": (4, 4, 16, (1, 4, 4), 0.6, 257, "upshifted", "white"),        # more indices than voxels: duplicates
    "s16_n5_ragged": (16, 5, 24, (1, 5, 7), 0.25, 1000, "leaky_relu", "black"),
    "s16_n11": (16, 11, 24, (1, 4, 4), 0.9, 257, "upshifted", "black"),
}


def g26():
    """g26_spline_len_<case>: the reference's two spline-length terms (runner.py:784-796 over arc_len, src/nerf.py:1509-1520), in fp32
    AND on `.double()` copies.  Data only.
      grid term    `g_data` built as runner.py:793-795 from the carried indices `g_idxs` (a seeded torch.randint draw decoded as
                   random_sample_grid decodes it, checked against that function) on the model's procedural ctrl_pts_grid: arc_len per
                   voxel `g_lens`, their mean `g_value`, autograd's gradient w.r.t. the grid `g_grad`.  Control point 0 is not
                   prepended there, so spline 2 is a one-point spline: every length and the gradient are 0.
      sample term  the reference's DynamicNeRFVoxel over its NeRFVoxel + Positional built as g25 builds them, eval mode, ONE view
                   (arc_len's .squeeze(dim=1) is a shape error at more), voxel_ref.generic_rays: model.ctrl_pts `s_ctrl_pts`,
                   arc_len of them `s_lens`, the canonical's weights `s_weights`, (w * arc_lens).mean() `s_value` and the gradient
                   w.r.t. ctrl_pts_grid `s_grad`.  g23's rule: a seed on which the reference's fp32 and fp64 lengths disagree by more
                   than 1e-5 (a sample on a cell-membership plane) pins nothing and is skipped."""
    import copy
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import voxel_ref as V
    for name, (S, spline, T, shape, time, K, act, bg) in SPLINE_LEN_CASES.items():
        canon, _, _ = _voxel_build(S, T, act, bg)
        m = rnerf.DynamicNeRFVoxel(canon, spline=spline)
        m.eval()
        names, shapes = fill_procedural(m)
        m64 = copy.deepcopy(m).double()
        t = torch.tensor([time], dtype=torch.float32)

        def sample_term(model, dt, rays):
            with torch.enable_grad():
                model.ctrl_pts_grid.requires_grad_(True)
                model.ctrl_pts_grid.grad = None
                model((rays.to(dt), t.to(dt)))
                lens = rnerf.arc_len(model.ctrl_pts)
                w = model.canonical.weights.detach().squeeze(1)
                value = (w * lens).mean()
                value.backward()
            return dict(ctrl_pts=model.ctrl_pts.detach(), lens=lens.detach(), weights=w, value=value.detach(), grad=model.ctrl_pts_grid.grad.clone())
        for seed in range(4500, 4600, 2):
            rays = V.generic_rays(shape, seed)
            r32, r64 = sample_term(m, torch.float32, rays), sample_term(m64, torch.float64, rays)
            dev = float((r32["lens"].double() - r64["lens"]).abs().max())
            if dev <= 1e-5:
                break
            print(f"g26 {name}: seed {seed} skipped, the reference's fp32 and fp64 lengths disagree by {dev:.2e}")
        else:
            raise AssertionError(f"g26 {name}: no seed on which the reference agrees with itself")
        assert r32["lens"].shape == (T,) + tuple(shape[1:]) and r32["lens"].dtype == torch.float32 and r64["value"].dtype == torch.float64
        kw = dict(rays=rays, time=t, S=S, spline=spline, steps=T, near=2.0, far=6.0, act=act, bg=bg, grid_radius=canon.grid_radius, seed=seed,
                  ts=m.ts, **spec(names, shapes))
        for k in r32:
            kw["s_" + k], kw["s_" + k + "64"] = r32[k], r64[k]
        torch.manual_seed(2600 + S + spline)
        idxs = torch.randint(0, S ** 3, (K,))
        torch.manual_seed(2600 + S + spline)
        x, y, z = rnerf.random_sample_grid(m.ctrl_pts_grid, K)
        assert torch.equal(x, idxs % S) and torch.equal(y, idxs // S % S) and torch.equal(z, idxs // (S * S) % S)

        def grid_term(model):
            with torch.enable_grad():
                model.ctrl_pts_grid.grad = None
                data = torch.stack(model.ctrl_pts_grid[x, y, z].split(3, dim=-1), dim=0)[:, :, None, None, None, :]
                lens = rnerf.arc_len(data)
                value = lens.mean()
                value.backward()
            return dict(lens=lens.detach().reshape(K), value=value.detach(), grad=model.ctrl_pts_grid.grad.clone())
        q32, q64 = grid_term(m), grid_term(m64)
        for k in q32:
            kw["g_" + k], kw["g_" + k + "64"] = q32[k], q64[k]
        print(f"g26 {name}: seed {seed}; sample term {float(r64['value']):.9f} (lengths up to {float(r64['lens'].max()):.3f}, fp32 off by {dev:.2e}), "
              f"grid term {float(q64['value']):.9f} over {len(set(idxs.tolist()))} distinct of {K} indices")
        save(f"g26_spline_len_{name}", g_idxs=idxs, **kw)


def g27():
    """g27_voxel_plv_<case>: g23 with the reference's PosLinearView head in its voxel form (src/refl.py:265-280: rgb [S,S,S, 3 + 25],
    order 4) -- same cases, same seed rule, same outputs and fp64 gradients; the lattice ids and xyz are g23's and are carried again."""
    g23("g27_voxel_plv_", rrefl.PosLinearView, ("s2", "s4", "s16_ragged", "s64_black"))


DYN_VOXEL_PLV_CASES = {  # (the layout of DYN_VOXEL_CASES)
    "s4_n4": (4, 4, 16, (3, 4, 4), (0.0, 0.6, 1.0), "upshifted", "white"),
    "s16_n2": (16, 2, 24, (2, 5, 7), (0.25, 0.8), "leaky_relu", "black"),
}


def g28():
    """g28_dyn_voxel_plv_<case>: g25's builder over the canonical model of g27 (NeRFVoxel + PosLinearView, order 4)"""
    g25("g28_dyn_voxel_plv_", rrefl.PosLinearView, DYN_VOXEL_PLV_CASES)


DYN_VOXEL_DIV_CASES = {  # name: (S, spline, T, ray batch shape [B, H, W], times [B])
    "s2_n2": (2, 2, 6, (1, 3, 3), (0.7,)),
    "s4_n4": (4, 4, 6, (2, 2, 3), (0.35, 1.0)),
    "s4_n5": (4, 5, 6, (1, 3, 3), (0.6,)),
    "s16_n11_ragged": (16, 11, 7, (1, 3, 5), (0.45,)),   # 105 samples
}


def g29():
    """g29_dyn_voxel_div_<case>: the reference's two divergence regularisers over its DynamicNeRFVoxel (runner.py:694-700:
    utils.div_approx(model.pts, model.rigid_dp) and utils.divergence(model.pts, model.dp)), TRAINING mode (perturbed samples,
    pts.requires_grad_()), evaluated in fp64.  Data only.
      positions   the fp32 training-mode forward under the carried torch seed gives `pts` (fp32); the fp64 model is then run AT those
                  positions (compute_pts_ts wrapped to hand back their double images), so every input of the fp64 run is an fp32 number.
      membership  g24 / g28's convention, made strict: every coordinate of every sample is at least 1e-3 voxel lengths from a plane on which
                  the cell pair changes (asserted; the next seed is taken otherwise), and the ids of the fp64 run equal those of the
                  fp32 chain (tests/voxel_ref.cells) -- no sample ever has to be excluded from a comparison.
      coverage    at least a third of the samples inside the grid and a third outside (asserted).
      e           captured as g17 captures it (the seed replayed); the draw is made in fp32 and widened (randn_like wrapped for the
                  call), so the kernels can be fed the very same numbers.
      contents    pts, t (one per sample), both grids (procedural values, stored), e, div_approx, divergence,
                  g_ctrl = d(mean divergence)/d ctrl_pts_grid, and the reference's own fp32 - fp64 deviations `dev`."""
    import copy
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import voxel_ref as V
    import dyn_voxel_div_ref as R
    for name, (S, spline, T, shape, times) in DYN_VOXEL_DIV_CASES.items():
        canon, _, _ = _voxel_build(S, T, "upshifted", "black")
        m = rnerf.DynamicNeRFVoxel(canon, spline=spline)
        fill_procedural(m)
        m.train()
        canon.train()
        m64 = copy.deepcopy(m).double()
        t = torch.tensor(times, dtype=torch.float32)
        gr = canon.grid_radius
        for seed in range(4500, 4700, 2):
            rays = V.generic_rays(shape, seed)
            torch.manual_seed(seed)
            with torch.enable_grad():
                m((rays, t))
            pts = m.pts.detach().clone()
            flat = pts.reshape(-1, 3)
            inside = (flat.abs() <= gr).all(dim=-1).float().mean()
            if float(R.face_distance(flat, S, gr).min()) >= 1e-3 and 1 / 3 <= float(inside) <= 2 / 3:
                break
        else:
            raise AssertionError(f"g29 {name}: no seed keeps every sample 1e-3 voxel lengths off the cell faces with a third inside / outside")
        orig_pts, orig_randn = rnerf.compute_pts_ts, torch.randn_like

        def run(model, dt):
            def at_pts(*a, **k):
                _, ts, r_o, r_d, mids = orig_pts(*a, **k)
                return pts.to(dt), ts, r_o, r_d, mids
            rnerf.compute_pts_ts = at_pts
            torch.randn_like = lambda x, **k: orig_randn(x.float(), **k).to(x.dtype)
            try:
                with torch.enable_grad():
                    model.ctrl_pts_grid.requires_grad_(True)
                    model.ctrl_pts_grid.grad = None
                    torch.manual_seed(seed)
                    model((rays.to(dt), t.to(dt)))
                    assert torch.equal(model.pts.detach(), pts.to(dt)) and model.pts.requires_grad
                    torch.manual_seed(seed + 1)
                    div_approx = rutils.div_approx(model.pts, model.rigid_dp)
                    torch.manual_seed(seed + 1)
                    e = torch.randn_like(model.rigid_dp)
                    divergence = rutils.divergence(model.pts, model.dp)
                    divergence.mean().backward()
                    ids, _ = model.canonical.grid_coords_trilin_weights(model.pts)
            finally:
                rnerf.compute_pts_ts, torch.randn_like = orig_pts, orig_randn
            assert not div_approx.requires_grad and divergence.requires_grad
            return dict(e=e.detach(), div_approx=div_approx.detach(), divergence=divergence.detach(), dp=model.dp.detach(),
                        g_ctrl=model.ctrl_pts_grid.grad.clone(), ids=ids)
        r32, r64 = run(m, torch.float32), run(m64, torch.float64)
        assert r64["div_approx"].dtype == torch.float64 and torch.equal(r32["e"].double(), r64["e"]) and float(r64["g_ctrl"].abs().max()) > 0
        assert torch.equal(r64["ids"].reshape(-1, 8, 3), V.cells(flat, S, gr)[0]), "the fp64 run and the fp32 chain read different cells"
        dev = {k: float((r32[k].double() - r64[k]).abs().max()) for k in ("div_approx", "divergence", "g_ctrl", "dp")}
        tt = t[None, :, None, None].expand(pts.shape[:-1]).contiguous()
        print(f"g29 {name}: seed {seed}, {flat.shape[0]} samples, {float(inside):.0%} inside, nearest face {float(R.face_distance(flat, S, gr).min()):.2e} vl; "
              f"|div_approx| up to {float(r64['div_approx'].abs().max()):.3g}, |divergence| up to {float(r64['divergence'].abs().max()):.3g}; "
              "fp32 vs fp64: " + " ".join(f"{k} {v:.2e}" for k, v in dev.items()))
        save(f"g29_dyn_voxel_div_{name}", pts=pts, t=tt, S=S, spline=spline, grid_radius=gr, seed=seed, rays=rays, times=t,
             ctrl_pts_grid=m.ctrl_pts_grid.detach(), rigidity_grid=m.rigidity_grid.detach(), e=r32["e"], div_approx=r64["div_approx"],
             divergence=r64["divergence"], g_ctrl=r64["g_ctrl"], dev=np.array([dev[k] for k in ("div_approx", "divergence", "g_ctrl", "dp")]))


IMAGE_LOSS_PROVENANCE = (
    "g30_image_loss.npz: tools/gen_golden.py g30 -- the reference's runner.load_loss_fn over tests/image_loss_ref.py COMBOS, CPU fp32\n"
    "train_parity_voxel_image_loss.json: tools/ref_train_fixture.py voxel_image_loss --epochs 200 --size 32 --crop-size 16 --steps 32 "
    "--batch-size 4 -- the reference's runner.main, CPU fp32, 8 threads\n")


def g30():
    """g30_image_loss: the reference's own runner.load_loss_fn(args, None) (runner.py:552-594) over the table of flag combinations of
    tests/image_loss_ref.py (COMBOS), in fp32, on that module's kink-free draw at P = 1025 and its hand-made edge set at P = 7: the
    loss and d loss / d got, and next to them the deviation of that fp32 result from the module's fp64 restatement (`g_dev`: per
    combination and input set the loss's and the gradient's largest absolute deviation; rgb2xyz builds an fp32 matrix and cannot run
    in fp64 itself)."""
    import types as _types
    import runner
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import image_loss_ref as R
    sets = {"draw": R.kink_free_draw(1025, 30), "edge": R.edge_set()}
    out = dict(combos=np.array([R.combo_name(c) for c in R.COMBOS]))
    dev = np.zeros((len(R.COMBOS), 2, 2))
    for si, (sname, (got, ref)) in enumerate(sets.items()):
        out[f"{sname}_got"], out[f"{sname}_ref"] = got, ref
        losses, grads = [], []
        for ci, (fns, spaces, tone, gamma) in enumerate(R.COMBOS):
            args = _types.SimpleNamespace(style_img=None, loss_fns=list(fns), color_spaces=list(spaces), tone_map=tone,
                                          gamma_correct_loss=gamma, volsdf_alternate=False, model="plain")
            fn = runner.load_loss_fn(args, None)
            with torch.enable_grad():
                x = torch.from_numpy(got).clone().requires_grad_(True)
                loss = fn(x, torch.from_numpy(ref))
                g, = torch.autograd.grad(loss, x)
            r = R.restate(got, ref, fns, spaces, tone, gamma)
            losses.append(float(loss))
            grads.append(g.numpy())
            dev[ci, si] = abs(float(loss) - r["loss"]), np.abs(g.numpy().astype(np.float64) - r["grad"]).max()
            over = max(dev[ci, si, 0] / max(r["loss_bound"], 1e-300), float((np.abs(g.numpy() - r["grad"]) / np.maximum(r["grad_bound"], 1e-300))
                                                                            [r["grad_bound"] > 0].max(initial=0.0)))
            print(f"g30 {sname:4s} {R.combo_name((fns, spaces, tone, gamma)):44s} loss {float(loss):.6f} dev {dev[ci, si, 0]:.1e} "
                  f"grad dev {dev[ci, si, 1]:.1e}  worst dev / bound {over:.2f}")
        out[f"{sname}_loss"], out[f"{sname}_grad"] = np.array(losses, np.float32), np.stack(grads).astype(np.float32)
    save("g30_image_loss", g_dev=dev, **out)
    # the two image-loss fixtures' provenance lines, in a file of their own next to PROVENANCE.txt (which describes the generator's build)
    with open(os.path.join(OUT, "PROVENANCE_image_loss.txt"), "w") as f:
        f.write(IMAGE_LOSS_PROVENANCE)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["g1", "g2", "g3", "g4", "g5", "g6", "g7", "g8", "g9", "g10", "g11", "g12", "g13", "g14", "g15", "g16", "g17", "g18", "g19", "g20", "g21", "g22", "g23", "g24", "g25", "g26", "g27", "g28", "g29", "g30"]
    for g in which:
        globals()[g]()
    with open(os.path.join(OUT, "PROVENANCE.txt"), "w") as f:
        f.write("Generated by tools/gen_golden.py from the reference at /root/reference (JulianKnodt/nerf_atlas)\n")
        f.write(f"torch {torch.__version__}, CPU fp32, threads={torch.get_num_threads()}\n")
        f.write(torch.__config__.show())
