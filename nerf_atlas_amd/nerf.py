"""Model-variant plugins of the hot path with the reference's protocol (src/nerf.py):
TinyNeRF, PlainNeRF, NeRFAE, NeRFVoxel, VolSDF, DynamicNeRF(spline) + the registries model_kinds / dyn_model_kinds / load_nerf /
load_dyn.  Every forward runs HIP kernels only; PlainNeRF with the View head takes the fully fused renderer.

Protocol kept for callers (runner.py): forward(rays) / forward((rays, times)), from_pts(...), .nerf, .refl,
.set_refl, .intermediate_size, .total_latent_size(), .set_bg, .set_sigmoid, .steps/.t_near/.t_far and, after a
forward, .ts, .alpha, .weights (+ .pts/.dp/.rigidity/.rigid_dp for dynamic models, .scale_post_act for VolSDF).
"""
import functools
import os

import torch
import torch.nn as nn

from . import autograd as ag
from . import config, ops
from . import refl
from .neural_blocks import HashEncoder, SkipConnMLP
from . import utils
from .utils import load_mip, load_sigmoid


# ------------------------------------------------------------------------------------------------- operators
_f16x_depth = 0


def _f16x_policy(fn):
    """config.f16x_on_saturation == "rerender_bf16x3": a forward whose f16x launch was flagged by the range guard
    (ops.F16xSaturated; csrc/render_ls.hip g_lsx_saturated) is rendered again in bf16x3, whose operands have fp32's range.  Only
    the outermost decorated call catches (DynamicNeRF.forward -> canonical.from_pts is one render)."""
    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        global _f16x_depth
        if _f16x_depth or config.f16x_on_saturation != "rerender_bf16x3" or config.precision != "f16x":
            return fn(self, *args, **kwargs)
        _f16x_depth += 1
        try:
            try:
                return fn(self, *args, **kwargs)
            except ops.F16xSaturated:
                with config.precision_as("bf16x3"):
                    return fn(self, *args, **kwargs)
        finally:
            _f16x_depth -= 1
    return wrapped


def compute_ts(rays, near, far, steps, lindisp=False, perturb: float = 0, rand=None):
    """src/nerf.py:29-47.  `rand` [steps] replaces the global-RNG draw; drawn here if perturb>0 and none given."""
    r_o, r_d = rays.split([3, 3], dim=-1)
    if perturb > 0 and rand is None:
        rand = utils.rand((steps,), rays.device)
    ts, mids = ops.compute_ts(near, far, steps, rays.device, lindisp, perturb, rand)
    return r_o, r_d, ts, mids


def compute_pts_ts(rays, near, far, steps, lindisp=False, perturb: float = 0, rand=None):
    """src/nerf.py:50-55."""
    r_o, r_d, ts, mids = compute_ts(rays, near, far, steps, lindisp, perturb, rand)
    pts = ops.compute_pts(rays, ts)
    return pts, ts, r_o, r_d, mids


def alpha_from_density(density, ts, r_d, softplus: bool = True):
    """src/nerf.py:60-73 (via the compositing kernel with a dummy 1-channel feature)."""
    rays = torch.cat([torch.zeros_like(r_d), r_d], dim=-1)
    feat = torch.ones(density.shape + (1,), device=density.device)
    _, alpha, weights = ops.composite(density, feat, ts, rays, softplus=softplus)
    return alpha, weights


def volumetric_integrate(weights, other):
    """src/nerf.py:79-80."""
    return ops.integrate(weights, other)


def black(_elaz_r_d, _weights): return 0
def white(_, weights): return 1 - weights[:-1].sum(dim=0).unsqueeze(-1)


def random_color(_elaz_r_d, weights, rand=None):
    """src/nerf.py:101-103: ONE uniform draw per ray (rand_like of the [..., 1] remainder) times the remainder; the draw is an
    explicit tensor here (utils.rand: the replayable random source of Q13) and a kernel does the arithmetic."""
    shape = tuple(weights.shape[1:]) + (1,)
    if rand is None: rand = utils.rand(shape, weights.device)
    return ops.sky_random(weights, rand, torch.zeros(shape, device=weights.device))


# src/nerf.py:104-109 (same keys; "mlp" is broken in the reference: Q12)
sky_kinds = {"black": black, "white": white, "mlp": "MLP_MARKER", "random": random_color}


def cat_not_none(a, b, dim=-1):
    if isinstance(a, utils.MipLatent):  # lazy IPE latent: stays lazy, the other columns ride along
        return a if b is None else a.with_rest(b)
    return a if b is None else (b if a is None else torch.cat([a, b], dim=dim))


# ------------------------------------------------------------------------------------------------- CommonNeRF
class CommonNeRF(utils.PackedCacheMixin, nn.Module):
    """src/nerf.py:147-276."""

    def __init__(self, r=None, steps: int = 64, fine_steps: int = 32, t_near: float = 0, t_far: float = 1,
                 density_std: float = 0.01, noise_std: int = 1e-2, mip=None, instance_latent_size: int = 0,
                 per_pixel_latent_size: int = 0, per_point_latent_size: int = 0, intermediate_size: int = 32,
                 sigmoid_kind: str = "thin", bg: str = "black"):
        super().__init__()
        self.t_near, self.t_far, self.steps, self.fine_steps = t_near, t_far, steps, fine_steps
        self.mip = mip
        assert instance_latent_size == 0 and per_pixel_latent_size == 0 and per_point_latent_size == 0, \
            "instance/per-pixel/per-point latents are outside the 5 configs of the hot path"
        self.per_pixel_latent_size = self.instance_latent_size = self.per_pt_latent_size = 0
        try: self.intermediate_size = intermediate_size
        except AttributeError: ...
        self.alpha = self.weights = self.ts = self.ts_ray = None
        self.noise_std = 0.2
        self._init_packed_hooks()
        self.set_bg(bg)
        if r is not None: self.refl = r(self.total_latent_size())
        self.set_sigmoid(sigmoid_kind)

    def set_bg(self, bg="black"):
        if bg not in sky_kinds: raise NotImplementedError(bg)
        if bg == "mlp":
            raise NotImplementedError("bg 'mlp' is broken in the reference (SURVEY Q12); black|white|random")
        self.bg = bg
        self.sky_color = sky_kinds[bg]
        self.bg_rand = None  # bg "random": the per-ray draw of the last forward ([..., 1])

    def set_sigmoid(self, kind="thin"):
        act = load_sigmoid(kind)
        self.sigmoid_kind = kind
        self.feat_act = act
        if hasattr(self, "refl") and self.refl is not None:
            self.refl.act = act
            self.refl.act_kind = kind  # (the name the fused paths go by: it used to keep the constructor's default here)

    def total_latent_size(self) -> int: return self.mip_size()

    def set_refl(self, r):
        if hasattr(self, "refl"): self.refl = r

    @property
    def nerf(self): return self

    def mip_size(self): return 0 if self.mip is None else self.mip.size() * 6

    def mip_latent(self, rays, ts):
        """the IPE latent as a lazy handle (utils.MipLatent): generated inside the fused MLP kernels"""
        return None if self.mip is None else self.mip.lazy(rays, ts)

    def mip_encoding(self, rays, ts):
        """src/nerf.py:256-261, intended layout; rays [B,H,W,6] of one crop."""
        return None if self.mip is None else self.mip(rays, ts)

    def _perturb(self): return 1 if self.training else 0

    def _kernel_bg(self):
        """what the fused one-kernel renderers composite against: the random background is added behind them (`_finish_sky`)"""
        return "black" if self.bg == "random" else self.bg

    def _finish_sky(self, out):
        """bg "random" behind a fused renderer that composited against black and kept its weights (src/nerf.py:99-103)"""
        if self.bg == "random":
            self.bg_rand = utils.rand(tuple(out.shape[:-1]) + (1,), out.device)
            ops.sky_random(self.weights, self.bg_rand, out)
        return out

    def _composite(self, density, feat, ts, rays, softplus=True, with_sky=True):
        bg = self.bg if with_sky else "black"
        rand = None
        if bg == "random":
            rand = self.bg_rand = utils.rand(tuple(rays.shape[:-1]) + (1,), rays.device)
        per_ray = ts.dim() > 1  # ts [*batch, T]: the fine pass of coarse -> fine training integrates over per-ray steps
        if torch.is_grad_enabled() and (density.requires_grad or feat.requires_grad):
            from .autograd import CompositeFn, CompositeRayTsFn
            fn = CompositeRayTsFn if per_ray else CompositeFn
            out, self.alpha, self.weights = fn.apply(density.contiguous(), feat.contiguous(), ts, rays, softplus, bg, rand)
            return out
        comp = ops.composite_rayts if per_ray else ops.composite
        out, self.alpha, self.weights = comp(density, feat, ts, rays, softplus=softplus, bg=bg, rand=rand)
        return out


# ------------------------------------------------------------------------------------------------- TinyNeRF
class TinyNeRF(CommonNeRF):
    """src/nerf.py:278-305 with the intended semantics density = estim[...,0] (the reference class cannot be
    constructed at HEAD: SURVEY header table)."""

    def __init__(self, out_features: int = 3, **kwargs):
        super().__init__(**kwargs)
        self.estim = SkipConnMLP(in_size=3, out=1 + out_features, latent_size=self.total_latent_size(), num_layers=6,
                                 hidden_size=256, init="xavier")

    def _fusable(self):
        """one-kernel inference on the layer-synchronous engine (csrc/render_ls.hip, MODEL 1)"""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return (config.engine == "ls" and self.mip is None and self.total_latent_size() == 0
                and self.estim.out.out_features == 4 and not self.training and not wants_grad)

    def packed_ls(self, precision: str):
        """Weight stream of the layer-synchronous renderer (cached, re-packed when any parameter changed)."""
        lin = self.estim._linears()
        return utils.packed_stream(self, "_packed_ls", precision, lin, lambda: ops.render_tiny_ls_pack(precision, *utils.linears_wb(lin)))

    @_f16x_policy
    def forward(self, rays, want_weights: bool = True):
        if self._fusable():
            _, _, self.ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps)
            prec = config.kernel_precision(has_f16x=True)
            out, self.alpha, self.weights = ops.render_tiny_ls(rays, self.ts, self.packed_ls(prec), prec, self.sigmoid_kind,
                                                                self._kernel_bg(), want_weights or self.bg == "random")
            return self._finish_sky(out)
        pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        return self.from_pts(pts, self.ts, r_o, r_d, rays=rays)

    def from_pts(self, pts, ts, r_o, r_d, refl_latent=None, rays=None):
        if rays is None: rays = torch.cat([r_o, r_d], dim=-1)
        if self._fusable() and refl_latent is None and not ag.needs_grad(pts):
            # explicit sample positions (a deformation field in front of TinyNeRF) through the same kernel
            prec = config.kernel_precision(has_f16x=True)
            out, self.alpha, self.weights = ops.render_tiny_ls(rays.contiguous(), ts, self.packed_ls(prec), prec, self.sigmoid_kind,
                                                                self._kernel_bg(), True, pts=pts.contiguous())
            return self._finish_sky(out)
        latent = self.mip_encoding(rays, ts)
        o = self.estim(pts, latent)
        density, feats = o[..., 0].contiguous(), o[..., 1:].contiguous()
        return self._composite(density, self.feat_act(feats), ts, rays)


# ------------------------------------------------------------------------------------------------- PlainNeRF
class PlainNeRF(CommonNeRF):
    """src/nerf.py:310-361.  steps_fine > 0 (train.py --steps-fine): every forward is coarse -> fine (forward_coarse_fine)."""

    steps_fine: int = 0  # (a plain attribute, neither parameter nor buffer: the state_dict does not know it)

    def __init__(self, out_features: int = 3, **kwargs):
        super().__init__(r=lambda ls: refl.View(out_features=out_features, latent_size=ls + self.intermediate_size),
                         **kwargs)
        self.first = SkipConnMLP(in_size=3, out=1 + self.intermediate_size, latent_size=self.total_latent_size(),
                                 enc=HashEncoder(), num_layers=4, hidden_size=256)

    def _fusable(self, refl_latent=None):
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return (isinstance(self.refl, refl.View) and self.mip is None and refl_latent is None
                and self.intermediate_size == 64 and self.refl.out_features == 3 and not self.training
                and not wants_grad)

    def _fusable_head(self, refl_latent=None):
        """PlainNeRF + refl.Positional / refl.PosLinearView as ONE launch of the layer-synchronous engine (csrc/ls_sched_plain_pos.inc,
        ls_sched_plain_plv.inc: MODEL 7 / 8; f16x only): "pos" | "plv" | None.  PosLinearView takes up to three refl_latent columns
        (DynamicNeRF, --dyn-refl-latent)."""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if (config.engine != "ls" or config.precision != "f16x" or self.mip is not None or self.intermediate_size != 64
                or self.training or wants_grad or self.refl.out_features != 3 or getattr(self.refl, "act_kind", None) not in ops.SIGMOID):
            return None
        n_rl = 0 if refl_latent is None else refl_latent.shape[-1]
        if type(self.refl) is refl.Positional and n_rl == 0 and self.refl.latent_size == 64:
            return "pos"
        if (type(self.refl) is refl.PosLinearView and n_rl <= 3 and self.refl.latent_size == 64 + n_rl and self.refl.im == 64
                and self.refl.act_kind in ("normal", "thin", "fat", "upshifted")):  # (the kinds MODEL 8 applies to its 67 rows in the kernel)
            return "plv"
        return None

    def packed_head_ls(self, kind: str, precision: str, n_rl: int = 0):
        r = self.refl
        heads = r.mlp._linears() if kind == "pos" else r.pos._linears() + r.view._linears()
        first = self.first._linears()

        def pack():
            if kind == "pos":
                return ops.render_plain_pos_ls_pack(precision, utils.linears_wb(first), utils.linears_wb(heads))
            return ops.render_plain_plv_ls_pack(precision, utils.linears_wb(first), utils.linears_wb(heads), n_rl)
        return utils.packed_stream(self, "_packed_head_ls", (kind, precision, n_rl), first + heads, pack)

    def _render_head(self, kind, rays, ts, want_weights, pts=None, refl_latent=None):
        want_weights = want_weights or self.bg == "random"
        r = self.refl
        if kind == "pos":
            return ops.render_plain_pos_ls(rays, ts, self.first.enc.tables(), r.mlp.enc.tables(), self.packed_head_ls("pos", "f16x"),
                                           "f16x", self.sigmoid_kind, self._kernel_bg(), want_weights, pts=pts)
        n_rl = 0 if refl_latent is None else refl_latent.shape[-1]
        return ops.render_plain_plv_ls(rays, ts, self.first.enc.tables(), r.pos.enc.tables(), self.packed_head_ls("plv", "f16x", n_rl),
                                       "f16x", self.sigmoid_kind, self._kernel_bg(), want_weights, pts=pts, refl_latent=refl_latent)

    def _fusable_mip(self, rays):
        """mip + f16x on the layer-synchronous engine (csrc/render_ls.hip MODEL 6): whole crops [B,H,W,6], 16 IPE degrees."""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return (config.engine == "ls" and config.precision == "f16x" and self.mip is not None
                and self.mip.max_deg - self.mip.min_deg == 16 and rays.dim() == 4 and rays.shape[1] >= 2
                and isinstance(self.refl, refl.View) and self.intermediate_size == 64 and self.refl.out_features == 3
                and self.total_latent_size() == 96 and not self.training and not wants_grad)

    def packed_mip_ls(self, precision: str):
        first, view = self.first._linears(), self.refl.mlp._linears()
        return utils.packed_stream(self, "_packed_mip_ls", precision, first + view,
                                   lambda: ops.render_plain_mip_ls_pack(precision, utils.linears_wb(first), utils.linears_wb(view)))

    def packed_ls(self, precision: str):
        """Weight stream of the layer-synchronous renderer (both MLPs in one buffer; cached, re-packed when any
        parameter changed)."""
        first, view = self.first._linears(), self.refl.mlp._linears()
        return utils.packed_stream(self, "_packed_ls", precision, first + view,
                                   lambda: ops.render_ls_pack(precision, utils.linears_wb(first), utils.linears_wb(view)))

    def _render_fused(self, rays, ts, want_weights, pts=None):
        """sample -> hash -> first -> elaz -> View -> sigmoid -> composite in ONE kernel (config.engine picks the
        layer-synchronous engine or the register-resident one)."""
        prec = config.kernel_precision(has_f16x=True)
        want_weights = want_weights or self.bg == "random"
        if config.engine == "ls":
            return ops.render_plain_view_ls(rays, ts, self.first.enc.tables(), self.packed_ls(prec), prec,
                                            self.sigmoid_kind, self._kernel_bg(), want_weights, pts=pts)
        _, pf = self.first.packed(prec, "plain_first")
        _, pv = self.refl.mlp.packed(prec, "plain_view")
        return ops.render_plain_view(rays, ts, self.first.enc.tables(), pf, pv, prec, self.sigmoid_kind, self._kernel_bg(),
                                     want_weights, pts=pts)

    def _train_forward_ls(self, rays, ts, pts, r_d):
        """Training (round 6): both networks' forwards as ONE launch of the layer-synchronous engine in the three-product bf16 split
        (csrc/ls_kernel.h MODEL 9) instead of twelve training Linears -- every Linear's output rows are written once for the backward
        pass and never read back by the forward.  Returns (planes [10, N, 256], (density [N], the View MLP's init rows [N, 69]),
        rgb_pre [N, 3], the stacked hash tables), or None when the step does not have the shape the kernel serves (then the
        layer-by-layer forward runs: the same three-product arithmetic with another summation order).
        `config.set_train_forward("layers")` / NA_TRAIN_LS=0 switch it off."""
        N = pts.numel() // 3
        if (config.train_forward != "ls" or config.train_precision != "bf16x3" or not torch.is_grad_enabled() or not pts.is_cuda
                or type(self.refl) is not refl.View or self.mip is not None or self.intermediate_size != 64 or self.refl.out_features != 3
                or self.refl.mlp.last_layer_act or self.first.last_layer_act or self.refl.mlp.latent_size != 64
                or r_d.shape != pts.shape[1:] or ts.dim() != 1 or ts.shape[0] != pts.shape[0]
                or not (8192 <= N <= ops.TRAIN_LS_MAX_ROWS) or os.environ.get("NA_TRAIN_ROWS") == "0"
                or os.environ.get("NA_TRAIN_MLP_FN") == "0" or os.environ.get("NA_TRAIN_FUSED_BWD") == "0"
                or not all(p.requires_grad for p in self.first.parameters()) or not all(p.requires_grad for p in self.refl.mlp.parameters())):
            return None
        enc = self.first.enc
        tables = torch.stack([e.weight for e in enc.embs])  # (differentiable: the encoder's node of this step takes the same tensor)
        with torch.no_grad():
            planes, rows, density, rgb_pre, _ = ops.train_plain_view_ls(rays.reshape(-1, 6), ts, pts.detach(), tables.detach(),
                                                                        self.packed_ls("bf16x3"), self.sigmoid_kind)
        return planes, (density, rows), rgb_pre, tables

    @_f16x_policy
    def forward(self, rays, want_weights: bool = True):
        if self.steps_fine > 0: return self.forward_coarse_fine(rays, self.steps_fine)
        self.ts_ray = None  # (only forward_coarse_fine integrates over per-ray steps)
        if self._fusable():
            _, _, self.ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps)
            out, self.alpha, self.weights = self._render_fused(rays, self.ts, want_weights)
            return self._finish_sky(out)
        head = self._fusable_head()
        if head is not None:
            _, _, self.ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps)
            out, self.alpha, self.weights = self._render_head(head, rays.contiguous(), self.ts, want_weights)
            return self._finish_sky(out)
        if self._fusable_mip(rays):
            # config 3 under f16x: sample -> hash -> IPE -> first -> View -> composite as ONE launch
            _, _, self.ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps)
            out, self.alpha, self.weights = ops.render_plain_mip_ls(
                rays.contiguous(), self.ts, self.first.enc.tables(), self.packed_mip_ls("f16x"), "f16x", self.mip.kind, float("nan"),
                self.mip.min_deg, self.mip.max_deg, self.sigmoid_kind, self._kernel_bg(), want_weights or self.bg == "random")
            return self._finish_sky(out)
        rand = None
        pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb(),
                                                   rand=rand)
        return self.from_pts(pts, self.ts, r_o, r_d, rays=rays)

    @_f16x_policy
    def forward_coarse_fine(self, rays, steps_fine: int, u=None, want_weights: bool = True):
        """Coarse -> fine rendering (BASELINE config 2 "64 + 128"; INTENDED reading of the reference's dead sample_pdf /
        CoarseFineNeRF, src/nerf.py:548-580, 1745-1779 -- see csrc/basic_ops.hip resample_ts_kernel): a coarse pass over
        `self.steps` shared steps, inverse-cdf resampling of `steps_fine` new positions per ray from its weights (u: None =
        linspace, or [steps_fine, *rays.shape[:-1]] draws), and a fine pass over the union in order -- three launches of the
        layer-synchronous engine's kernels, one network for both passes like the reference's class.
        In training mode, or with gradients wanted: the differentiable route on the operator path (`_coarse_fine_operators`)."""
        if not (self._fusable() and config.engine == "ls"):
            wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
            if isinstance(self.refl, refl.View) and self.mip is None and (self.training or wants_grad):
                return self._coarse_fine_operators(rays.contiguous(), steps_fine, u)
            raise NotImplementedError("coarse -> fine rendering runs on the fused layer-synchronous renderer (eval mode, View head)")
        rays = rays.contiguous()
        _, _, ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps)
        prec = config.kernel_precision(has_f16x=True)
        tables, packed = self.first.enc.tables(), self.packed_ls(prec)
        coarse, _, w = ops.render_plain_view_ls(rays, ts, tables, packed, prec, self.sigmoid_kind, self._kernel_bg(), True)
        self.coarse = coarse
        # `ts` keeps the protocol of every other forward -- the [T] shared (coarse) steps; the per-ray union the fine pass
        # integrated over is `ts_ray` [*batch, T + N] (weights / alpha rows follow IT: render.depth_map knows)
        self.ts = ts
        self.ts_ray = ops.resample_ts(ts, w, steps_fine, u)
        out, self.alpha, self.weights = ops.render_plain_view_ls_rayts(rays, self.ts_ray, tables, packed, prec, self.sigmoid_kind,
                                                                       self._kernel_bg(), want_weights or self.bg == "random")
        return self._finish_sky(out)

    def _coarse_fine_operators(self, rays, steps_fine: int, u=None):
        """Coarse -> fine with both passes on the operator path and in the graph: what training minimises is NeRF's joint loss over
        `self.coarse` and the returned fine image, one network for both (train.py).  The coarse pass is an ordinary forward over the
        shared steps (stratified in training mode); its weights -- constants -- place `steps_fine` new samples per ray
        (na_resample_ts; u: the caller's draws, else one utils.rand draw per new sample in training mode, linspace in eval mode),
        and the fine pass evaluates the same network at o + t d over every ray's own merged row and composites over it
        (autograd.CompositeRayTsFn).  No gradient flows through the sample positions, as in NeRF.  Density noise and the draw of
        bg "random" are drawn per pass, coarse first."""
        pts, ts, r_o, r_d, _ = compute_pts_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        self.coarse = self._from_pts_operators(pts, ts, r_o, r_d, None, rays)
        if u is None and self.training:
            u = utils.rand((steps_fine,) + tuple(rays.shape[:-1]), rays.device)
        ts_ray = ops.resample_ts(ts, self.weights.detach(), steps_fine, u)
        out = self._from_pts_operators(ops.compute_pts_rayts(rays, ts_ray), ts_ray, r_o, r_d, None, rays)
        # the protocol of the fused route: `ts` the [T] shared steps, `ts_ray` [*batch, T + N] what alpha / weights [T + N, ...] follow
        self.ts, self.ts_ray = ts, ts_ray
        return out

    def from_pts(self, pts, ts, r_o, r_d, refl_latent=None, rays=None):
        if rays is None: rays = torch.cat([r_o, r_d], dim=-1).contiguous()
        self.ts_ray = None  # (explicit positions: shared steps -- a stale per-ray row of an earlier coarse -> fine call must not reach render.depth_map)
        if self._fusable(refl_latent) and not ag.needs_grad(pts):
            # explicit sample positions (D-NeRF: spline-warped canonical points) through the same fused kernel
            out, self.alpha, self.weights = self._render_fused(rays, ts, True, pts=pts.contiguous())
            return self._finish_sky(out)
        head = self._fusable_head(refl_latent)
        if head is not None and not ag.needs_grad(pts) and (refl_latent is None or not ag.needs_grad(refl_latent)):
            # explicit sample positions (D-NeRF: warped points, + its per-sample reflectance latent) through the one-launch renderer
            out, self.alpha, self.weights = self._render_head(head, rays.contiguous(), ts, True, pts=pts.contiguous(), refl_latent=refl_latent)
            return self._finish_sky(out)
        # (refl.SphericalHarmonic: the generic branch below IS its fast path -- per-ray hoisted kernels inside the head)
        if (not self.training and not ag.needs_grad(pts, *self.parameters()) and refl_latent is None and self.mip is None
                and not isinstance(self.refl, refl.SphericalHarmonic)):
            utils.note_fallback(f"plain-unfused-{type(self.refl).__name__}-{self.intermediate_size}",
                                f"PlainNeRF with {type(self.refl).__name__} reflectance / intermediate size {self.intermediate_size} is not one of the "
                                "fused renderer's schedules (View head, intermediate 64, 3 channels): inference runs the generic MLP kernels "
                                "+ separate compositing")
        return self._from_pts_operators(pts, ts, r_o, r_d, refl_latent, rays)

    def _from_pts_operators(self, pts, ts, r_o, r_d, refl_latent, rays):
        """the operator path of `from_pts` (one kernel per operator, with its graph); ts [T] shared steps or [*batch, T] per-ray rows"""
        latent = self.mip_latent(rays, ts)  # lazy: generated in the prologues of `first` and of the View MLP
        pre = self._train_forward_ls(rays, ts, pts, r_d) if latent is None and refl_latent is None else None
        first_out = self.first(pts, latent, pre=None if pre is None else (list(pre[0][:5]), None, pre[3]))
        if (ag.needs_grad(first_out) and latent is None and refl_latent is None and type(self.refl) is refl.View and pts.is_cuda
                and not self.refl.mlp.last_layer_act and self.refl.mlp.latent_size == first_out.shape[-1] - 1
                and r_d.shape == pts.shape[1:] and os.environ.get("NA_TRAIN_ROWS") != "0"):
            # training: density | the View MLP's init rows [x, elev, azim | intermediate] by ONE kernel (autograd.PlainHeadFn; slice
            # copies, elaz, expand and two cats before), the network from its rows (SkipConnMLP.forward_rows)
            C = first_out.shape[-1]
            # (with precomputed values the node reads neither positions nor directions: no copy of the direction slice)
            density, rows = ag.PlainHeadFn.apply(first_out.reshape(-1, C), pts.reshape(-1, 3),
                                                 r_d.reshape(-1, 3).contiguous() if pre is None else None, None if pre is None else pre[1])
            density = density.reshape(pts.shape[:-1])
            if self.training and self.noise_std > 0:
                density = density + utils.randn(density.shape, density.device) * self.noise_std
            rgb = self.refl.act(self.refl.mlp.forward_rows(rows, pre=None if pre is None else (list(pre[0][5:]), pre[2]))
                                .reshape(pts.shape[:-1] + (self.refl.out_features,)))
            return self._composite(density, rgb, ts, rays)
        assert pre is None, "the one-launch training forward implies the rows path above (its `first_out` is a placeholder)"
        if ag.needs_grad(first_out):
            density, intermediate = ag.SplitHeadFn.apply(first_out)  # (the slices' gradients written side by side: autograd.py)
        else:
            density, intermediate = first_out[..., 0].contiguous(), first_out[..., 1:]
        if self.training and self.noise_std > 0:
            density = density + utils.randn(density.shape, density.device) * self.noise_std
        view = r_d.unsqueeze(0).expand_as(pts)
        rl = cat_not_none(latent, cat_not_none(intermediate, refl_latent))
        rgb = self.refl(x=pts, view=view, latent=rl)  # `intermediate` is a column slice of first_out: passed by pitch
        return self._composite(density, rgb, ts, rays)


# ------------------------------------------------------------------------------------------------- NeRFAE
class NeRFAE(CommonNeRF):
    """src/nerf.py:766-840: NeRF with a thin middle layer.  encode (Fourier, 5 x 128) -> [F.normalize] -> density_tform (5 x 64) ->
    density | intermediate; refl.View on cat[encoded, intermediate].

    Inference routes of `from_pts` (eval mode, no gradients wanted, engine "ls"):
      fused        both narrow networks as ONE launch (ops.ae_front, csrc/ae_front.hip) writing the [N, 1 + E + I] rows, then the View
                   head + compositing as one launch (ops.render_view_ls with beta=None: MODEL 2 on a density logit): E + I = 64
      front-only   the same front launch, then the generic head and compositing (a 96-wide latent, another head, refl_latent)
    Everything else -- training, E / I without a front kernel -- runs the SkipConnMLP operator path.  `latent_l2_loss` is a training
    term: the inference routes leave it as it is.  `--mip` raises (the reference's mip latent would enter `encode`; not built)."""

    def __init__(self, out_features: int = 3, encoding_size: int = 32, normalize_latent: bool = False, **kwargs):
        if kwargs.get("mip") is not None:
            raise NotImplementedError("--model ae with --mip: the IPE latent as an input of `encode` is not implemented")
        super().__init__(r=lambda _: refl.View(out_features=out_features, latent_size=encoding_size + self.intermediate_size),
                         **kwargs)
        from .neural_blocks import FourierEncoder
        self.latent_size = self.total_latent_size()
        self.encode = SkipConnMLP(in_size=3, out=encoding_size, latent_size=self.latent_size, num_layers=5, hidden_size=128,
                                  enc=FourierEncoder(input_dims=3), init="xavier")
        self.density_tform = SkipConnMLP(in_size=encoding_size, out=1 + self.intermediate_size, latent_size=0, num_layers=5,
                                         hidden_size=64, init="xavier")
        self.encoding_size = encoding_size
        self.regularize_latent = False
        self.normalize_latent = normalize_latent

    def set_regularize_latent(self):
        self.regularize_latent = True
        self.latent_l2_loss = 0

    # ---- fused inference
    def _front_ok(self, pts):
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        e = self.encode
        return (config.engine == "ls" and config.precision in ("bf16", "bf16x3", "f16x") and not self.training and not wants_grad
                and not ag.needs_grad(pts) and pts.is_cuda and ops.ae_front_supported(self.encoding_size, self.intermediate_size)
                and e.enc.freqs == 128 and e.latent_size == 0 and e.act_name == "leaky_relu"
                and self.density_tform.act_name == "leaky_relu")

    def _head_ok(self, refl_latent):
        r = self.refl
        return (type(r) is refl.View and refl_latent is None and self.encoding_size + self.intermediate_size == 64
                and r.latent_size == 64 and r.out_features == 3 and getattr(r, "act_kind", None) in ops.SIGMOID)

    def packed_front(self, precision: str):
        enc, den = self.encode._linears(), self.density_tform._linears()
        return utils.packed_stream(self, "_packed_front", precision, enc + den,
                                   lambda: ops.ae_front_pack(precision, self.encoding_size, self.intermediate_size, utils.linears_wb(enc),
                                                             utils.linears_wb(den)))

    def packed_view_ls(self, precision: str):
        lin = self.refl.mlp._linears()
        return utils.packed_stream(self, "_packed_view_ls", precision, lin, lambda: ops.render_view_ls_pack(precision, *utils.linears_wb(lin)))

    def _basis(self):
        enc = self.encode.enc
        return (enc.basis.data * float(enc.extra_scale)).contiguous() if float(enc.extra_scale) != 1.0 else enc.basis.data

    def front_rows(self, rays, ts, pts=None):
        """[T, ..., 1 + E + I] rows [density logit | encoded | intermediate] by the one-launch front."""
        prec = config.kernel_precision(has_f16x=True)
        return ops.ae_front(rays.contiguous(), ts, self._basis(), self.packed_front(prec), prec, self.encoding_size,
                            self.intermediate_size, self.normalize_latent, pts=None if pts is None else pts.contiguous())

    @_f16x_policy
    def forward(self, rays):
        pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        return self.from_pts(pts, self.ts, r_o, r_d, rays=rays)

    def compute_encoded(self, pts, ts, r_o, r_d):
        """src/nerf.py:814-822 (no instance latents, no mip: `encode` sees the positions only)."""
        return self.encode(pts, None)

    def from_pts(self, pts, ts, r_o, r_d, refl_latent=None, rays=None):
        if rays is None: rays = torch.cat([r_o, r_d], dim=-1).contiguous()
        self.ts, self.ts_ray = ts, None
        if self._front_ok(pts) and (refl_latent is None or not ag.needs_grad(refl_latent)):
            rows = self.front_rows(rays, ts, pts)
            if self._head_ok(refl_latent):
                prec = config.kernel_precision(has_f16x=True)
                out, self.alpha, self.weights = ops.render_view_ls(rays.contiguous(), ts, rows, None, self.packed_view_ls(prec), prec,
                                                                    self.refl.act_kind, self._kernel_bg(), True, pts=pts.contiguous())
                return self._finish_sky(out)
            utils.note_fallback(f"ae-front-only-{type(self.refl).__name__}-{self.encoding_size}-{self.intermediate_size}",
                                f"NeRFAE with {type(self.refl).__name__} reflectance over a {self.encoding_size} + {self.intermediate_size} "
                                "wide latent is not the fused View schedule (View head, 64 latent columns): the front runs as one "
                                "kernel, the head and the compositing run the generic kernels")
            density = rows[..., 0].contiguous()
            view = r_d.unsqueeze(0).expand_as(pts)
            rgb = self.refl(x=pts, view=view, latent=cat_not_none(rows[..., 1:], refl_latent))  # column slice: passed by pitch
            return self._composite(density, rgb, ts, rays)
        encoded = self.compute_encoded(pts, ts, r_o, r_d)
        if self.regularize_latent:
            self.latent_l2_loss = ag.RowSqnormMeanFn.apply(encoded) if ag.needs_grad(encoded) else ops.row_sqnorm_mean(encoded)
        return self.from_encoded(encoded, ts, r_d, pts, refl_latent, rays=rays)

    def from_encoded(self, encoded, ts, r_d, pts, refl_latent=None, rays=None):
        """src/nerf.py:823-840 on the operator path (HIP forward and backward kernels per Linear)."""
        if rays is None: raise ValueError("NeRFAE.from_encoded needs the rays [..., 6] (compositing reads the directions)")
        if self.normalize_latent:
            encoded = ag.RowNormalizeFn.apply(encoded) if ag.needs_grad(encoded) else ops.row_normalize(encoded)
        first_out = self.density_tform(encoded)
        if ag.needs_grad(first_out):
            density, intermediate = ag.SplitHeadFn.apply(first_out)
        else:
            density, intermediate = first_out[..., 0].contiguous(), first_out[..., 1:]
        if self.training and self.noise_std > 0:
            density = density + utils.randn(density.shape, density.device) * self.noise_std
        view = r_d.unsqueeze(0).expand_as(pts)
        rgb = self.refl(x=pts, view=view, latent=torch.cat([encoded, cat_not_none(intermediate, refl_latent)], dim=-1))
        return self._composite(density, rgb, ts, rays)


# ------------------------------------------------------------------------------------------------- grid regulariser
def random_sample_grid(grid, samples: int = 32 ** 3):
    """src/nerf.py:391-399: `samples` flat indices into grid [s0,s1,s2,C], drawn with replacement through utils.randint (under
    replay_reference_rng: torch's CPU stream at the reference's position).  The reference decodes them at once -- x = idxs % s0,
    y = idxs // s0 % s1, z = idxs // (s0 s1) % s2 --; here the kernels do (csrc/grid_ops.hip), so the flat indices are returned."""
    s0, s1, s2, _ = grid.shape
    return utils.randint(0, s0 * s1 * s2, (samples,), grid.device)


def channel_slabs(n_channels: int, width: int = ops.GRID_MAX_C):
    """[(lo, hi)]: contiguous channel slabs at most `width` wide that cover 0 .. n_channels (the grid kernels take 1 .. 32 channels; the
    spherical-harmonic voxel head has 48 at order 3 and 75 at order 4)"""
    return [(lo, min(lo + width, n_channels)) for lo in range(0, n_channels, width)]


def slab_weights(n_channels: int, width: int = ops.GRID_MAX_C):
    """the weight of each slab's mean in the mean over all channels: its share of the channels"""
    return [(hi - lo) / n_channels for lo, hi in channel_slabs(n_channels, width)]


def total_variation(grid, samples: int = 32 ** 3, idxs=None):
    """src/nerf.py:381-389 as one launch forward and one backward (autograd.GridTVFn).  idxs: explicit flat indices
    (range-checked on the host) instead of a draw.  A grid of more than 32 channels runs as contiguous channel slabs over the SAME
    indices: the term is elementwise per channel, so the mean over all channels is the width-weighted mean of the slabs' means."""
    trusted = idxs is None
    if trusted:
        idxs = random_sample_grid(grid, samples)

    def term(g):
        return ag.GridTVFn.apply(g, idxs, trusted) if ag.needs_grad(g) else ops.grid_tv(g.detach(), idxs, trusted)
    if grid.shape[-1] <= ops.GRID_MAX_C:
        return term(grid)
    slabs, weights = channel_slabs(grid.shape[-1]), slab_weights(grid.shape[-1])
    return sum(w * term(grid[..., lo:hi].contiguous()) for w, (lo, hi) in zip(weights, slabs))


def arc_len_grid(grid, samples: int = 16 ** 3, idxs=None):
    """runner.py:793-796 as one launch forward and one backward (autograd.GridSplineLenFn): the mean of arc_len
    (src/nerf.py:1509-1520) over `samples` voxels of a control-point grid [s0,s1,s2,3 m] drawn by random_sample_grid, each voxel's
    channels read as its m control points (no zero point in front).  idxs: explicit flat indices as random_sample_grid returns them
    (range-checked on the host) instead of a draw; x = idx % s0 is the slowest axis in memory, as in total_variation."""
    trusted = idxs is None
    s0, s1, s2, _ = grid.shape
    if trusted:
        idxs = random_sample_grid(grid, samples)
    elif bool(((idxs < 0) | (idxs >= s0 * s1 * s2)).any()):
        raise ValueError(f"idxs outside the grid: flat indices 0 .. {s0 * s1 * s2 - 1}")
    # the reference decodes the draw as grid[idx % s0, idx // s0 % s1, idx // (s0 s1) % s2]: that voxel's row in memory
    rows = ((idxs % s0) * s1 + idxs // s0 % s1) * s2 + idxs // (s0 * s1) % s2
    if ag.needs_grad(grid):
        return ag.GridSplineLenFn.apply(grid, rows, True)
    return ops.grid_spline_len(grid.detach(), rows, True)


# ------------------------------------------------------------------------------------------------- NeRFVoxel
class NeRFVoxel(CommonNeRF):
    """src/nerf.py:401-524: a dense grid of densities [S,S,S,1] and per-voxel colour parameters rgb [S,S,S,C], read by the reference's
    8-neighbour lookup (csrc/voxel.hip) -- no MLP anywhere.  The static model with the per-voxel RGB head
    (`--refl-kind pos`, refl.Positional.to_voxel) or the view-dependent one (`--refl-kind pos-linear-view --voxel-refl-order K`,
    refl.PosLinearView.to_voxel: rgb rows [raw rgb | (K+1)^2 spherical-harmonic coefficients], DESIGN.md 3p -- both routes below then
    run the ops.voxel_plv_* / autograd.VoxelPlvSampleFn operators), or the spherical-harmonic colour itself (`--refl-kind sph-har
    --voxel-sh-order K`, refl.SphericalHarmonic.to_voxel: rgb rows of 3 (K+1)^2 coefficients, DESIGN.md 3s -- ops.voxel_sh_* /
    autograd.VoxelShSampleFn, whose raw output is the RGB head's); `_head_spec` is the one place the head is read off.  The
    parameters keep the reference's names, so its state_dict loads.

    Routes of `forward` / `from_pts`:
      eval, no gradients  ops.voxel_render: positions, lookup, activation and compositing as ONE launch (two with bg "random")
      otherwise           autograd.VoxelSampleFn (lookup; its backward is the scatter-add into the two grids), the head's activation on
                          the colour columns (autograd.SigmoidFn), CommonNeRF._composite's nodes
    `steps_fine > 0` (`--voxel-steps-fine`, this build's flag; a plain attribute, not in the state_dict): `forward` renders coarse -> fine
    (`forward_coarse_fine`: a density-only proposal pass, ops.resample_ts, the fine pass over per-ray steps on the same two routes).
    `live` (a uint8 [S,S,S] buffer, None until `sparsify` has run): the eval routes become ops.voxel_sparse_render, which
    gathers and walks live samples only, and the operator routes mask the lookup's rows (autograd.VoxelMaskRowsFn).
    There is no density noise (the reference class has no noise_std).  Explicit positions that require a gradient (from_pts under
    DynamicNeRFVoxel) receive one from the lookup's node; the positions o + t d of `forward` are formed in the kernels and have none."""

    def __init__(self, out_features: int = 3, resolution: int = 64, alpha_init: float = 0.1, grid_radius: float = 1.3,
                 t_near: float = 0.2, t_far: float = 2, steps: int = 64, sigmoid_kind: str = "upshifted", bg: str = "black", **kwargs):
        if resolution <= 0 or resolution % 2 != 0:
            raise ValueError(f"NeRFVoxel resolution {resolution}: even resolutions only (the reference's ids are floor(.) + resolution / 2, "
                             "a half-integer truncated by .long() when the resolution is odd)")
        # (unknown kwargs of load_nerf -- mip, intermediate_size, ... -- are swallowed like the reference's **kwargs)
        super().__init__(steps=steps, t_near=t_near, t_far=t_far, sigmoid_kind=sigmoid_kind, bg=bg)
        self.resolution = resolution
        self.densities = nn.Parameter(torch.full([resolution] * 3 + [1], float(alpha_init)))
        self.rgb = nn.Parameter(torch.rand([resolution] * 3 + [out_features]))
        self.grid_radius = grid_radius
        self.voxel_len = grid_radius * 2 / resolution
        self.brdf = self._bare_brdf
        self._head = None
        self.steps_fine = 0  # > 0: forward renders coarse -> fine over steps + steps_fine samples per ray (forward_coarse_fine)
        self.register_buffer("live", None)  # uint8 [S,S,S] once `sparsify` has run: absent from a state_dict until then

    def _bare_brdf(self, params, view):
        """src/nerf.py:425: before a head is installed the colour is act(parameters)"""
        return self.feat_act(params)

    @property
    def refl(self):
        """the head installed by set_refl, else a parameter-free stand-in like the reference's property (src/nerf.py:434-435)"""
        return self._head if self._head is not None else refl.Reflectance(act=self.sigmoid_kind, latent_size=0, out_features=3)

    def set_refl(self, r):
        """src/nerf.py:436-439: the head gives up its MLP (`to_voxel`) and `rgb` is drawn again with its parameter count"""
        num_params, self.brdf = r.to_voxel()
        self._head = r
        self.rgb = nn.Parameter(torch.rand(*self.rgb.shape[:-1], num_params, device=self.rgb.device))

    def upsample(self, reso: int = 512):
        """src/nerf.py:454-459: both grids resampled to reso^3 by F.interpolate(mode="trilinear")'s arithmetic (ops.grid_upsample, one
        launch each; reso below the current resolution samples down the same way) and installed as NEW Parameters -- an optimiser that
        holds the old ones must be told (train.upsample_voxels)."""
        reso = int(reso)
        if reso < 2 or reso % 2 != 0:
            raise ValueError(f"NeRFVoxel.upsample({reso}): even resolutions only")
        if not self.densities.is_cuda:
            raise ValueError("NeRFVoxel.upsample: the grids must live on the GPU (the upsampling has no CPU implementation)")
        with torch.no_grad():
            # (trilinear upsampling is per channel: a grid of more than 32 channels is the concatenation of its slabs' results)
            self.rgb = nn.Parameter(torch.cat([ops.grid_upsample(self.rgb.data[..., lo:hi].contiguous(), reso)
                                               for lo, hi in channel_slabs(self.rgb.shape[-1])], dim=-1))
            self.densities = nn.Parameter(ops.grid_upsample(self.densities.data.contiguous(), reso))
        self._set_resolution(reso)
        if self.live is not None:
            print("[warn]: NeRFVoxel.upsample clears the liveness table (it is per voxel): call sparsify again")
            self.clear_live()

    def sparsify(self, thresh: float = 1e-2) -> float:
        """src/nerf.py:444-452 (a stub there): mark the voxels no sample needs and skip them from now on.  A voxel is kept
        iff its density's softplus(d - 1) is not below `thresh` (compared as raw densities against one fp32 constant, ops.voxel_d_thresh;
        a NaN density is kept); the buffer `live` uint8 [S,S,S] marks every cell whose samples can read a kept voxel
        (ops.voxel_live_table, one launch).  A sample outside it has alpha = weight = 0 exactly and its colour is not read: the eval
        routes gather and walk live samples only (ops.voxel_sparse_render), the operator routes mask the lookup's rows
        (autograd.VoxelMaskRowsFn).  The grids are NOT modified: the table goes with the checkpoint, a later sparsify
        replaces it, `clear_live` removes it.  Returns the live fraction of the table."""
        ops.voxel_d_thresh(thresh)  # (a bad threshold is refused whatever the device)
        if not self.densities.is_cuda:
            raise ValueError("NeRFVoxel.sparsify: the grids must live on the GPU (the liveness table has no CPU implementation)")
        with torch.no_grad():
            live, count = ops.voxel_live_table(self.densities.data, thresh)
        self.live = live
        return float(count.item()) / live.numel()

    def clear_live(self):
        """remove the liveness table: every route is the dense one again"""
        self.live = None

    def _set_resolution(self, reso: int):
        self.resolution = reso
        self.voxel_len = self.grid_radius * 2 / reso

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        """a checkpoint's grids decide the resolution (a model saved after `upsample` loads into a freshly built one): `densities` and
        `rgb` are resized before torch copies into them.  Anything else about the shapes (the channel counts) stays torch's size check."""
        den, rgb = state_dict.get(prefix + "densities"), state_dict.get(prefix + "rgb")
        if den is not None and rgb is not None and den.dim() == 4 and rgb.dim() == 4 and tuple(den.shape[:3]) != tuple(self.densities.shape[:3]):
            S = den.shape[0]
            if tuple(den.shape[:3]) != (S, S, S) or tuple(rgb.shape[:3]) != (S, S, S) or S < 2 or S % 2 != 0:
                raise ValueError(f"NeRFVoxel: a state_dict with densities {tuple(den.shape)} and rgb {tuple(rgb.shape)}: both grids must be "
                                 "cubic, of one even resolution")
            with torch.no_grad():
                self.densities = nn.Parameter(self.densities.new_empty((S, S, S, self.densities.shape[-1])))
                self.rgb = nn.Parameter(self.rgb.new_empty((S, S, S, self.rgb.shape[-1])))
            self._set_resolution(S)
        # the checkpoint decides about the liveness table too: one that has it allocates the buffer, one without clears it
        live = state_dict.get(prefix + "live")
        if live is None:
            self.live = None
        else:
            S = self.densities.shape[0]
            if live.dtype != torch.uint8 or tuple(live.shape) != (S, S, S):
                raise ValueError(f"NeRFVoxel: a state_dict whose liveness table is {live.dtype} {tuple(live.shape)} over grids of {S}^3: "
                                 f"`live` must be uint8 [{S},{S},{S}]")
            if self.live is None or tuple(self.live.shape) != (S, S, S):
                self.live = torch.empty((S, S, S), dtype=torch.uint8, device=self.densities.device)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    @property
    def intermediate_size(self): return 0

    def total_latent_size(self) -> int: return 0

    def set_sigmoid(self, kind="thin"):
        self.sigmoid_kind = kind
        self.feat_act = load_sigmoid(kind)
        if getattr(self, "_head", None) is not None:
            self._head.act, self._head.act_kind = self.feat_act, kind

    def _act_kind(self):
        """name of the colour activation for the one-launch route (the head's, once a head is installed), or None"""
        kind = self.sigmoid_kind if self._head is None else getattr(self._head, "act_kind", None)
        return kind if kind in ops.SIGMOID else None

    def _head_spec(self):
        """(kind, order) of the installed head, as every ops.voxel_* function and kernel names it: "plv" rgb rows [raw rgb | (order + 1)^2
        coefficients] (refl.PosLinearView; the order follows from the row's length, None for a row no order gives), "sh" 3 channel blocks
        of (order + 1)^2 coefficients (refl.SphericalHarmonic; the head's own order), else "rgb" with order -1"""
        kind = {refl.PosLinearView: "plv", refl.SphericalHarmonic: "sh"}.get(type(self._head), "rgb")
        return kind, self._head.order if kind == "sh" else ops.PLV_CHANNELS.get(self.rgb.shape[-1]) if kind == "plv" else -1

    def _head_kind(self): return self._head_spec()[0]

    def _plv(self): return self._head_kind() == "plv"

    def _sh_order(self):
        """the order of the installed spherical-harmonic colour head, or None"""
        kind, order = self._head_spec()
        return order if kind == "sh" else None

    def _fusable(self, pts=None):
        if self.training or ag.needs_grad(pts, self.densities, self.rgb) or self._act_kind() is None:
            return False
        kind, C = self._head_kind(), self.rgb.shape[-1]
        if kind == "rgb":
            return C == 3 and (self._head is None or type(self._head) is refl.Positional)
        return C == (3 + self._head.num_sh_coeffs if kind == "plv" else 3 * self._head.num_sh_coeffs)

    def _render(self, rays, ts, pts=None, per_ray=False):
        """the eval route as ONE launch (two with bg "random"): the shared row ts [T], at o + t d or explicit pts, or every ray's own row
        ts [*batch, M] (per_ray: the fine pass); with a liveness table the sparse renderer takes either kind of row"""
        kind, order = self._head_spec()
        grids, head = (self.densities.data, self.rgb.data), ((order,) if kind == "sh" else ())
        look = (self.grid_radius, self._act_kind(), self._kernel_bg(), True)
        family = {"rgb": "voxel", "plv": "voxel_plv", "sh": "voxel_sh"}[kind]  # (the public names: what a caller sees and a test counts)
        if self.live is not None:
            assert pts is None, "the sparse renderer forms o + t d itself"
            res = ops.voxel_sparse_render(kind, rays.contiguous(), ts, *grids, self.live, self.grid_radius, order, *look[1:])
        elif per_ray:
            res = getattr(ops, family + "_render_rayts")(rays, ts, *grids, *head, *look)
        else:
            res = getattr(ops, family + "_render")(rays.contiguous(), ts, *grids, *head, *look, pts=pts)
        out, self.alpha, self.weights = res
        return self._finish_sky(out)

    def _live_flags(self, rays, ts, pts=None):
        """uint8 [T, *batch] of the samples the lookups of `_operators` read (explicit pts, else o + t d over the shared row)"""
        if pts is not None:
            return ops.voxel_live_samples(self.live, self.grid_radius, pts=pts.detach().contiguous())
        return ops.voxel_live_samples(self.live, self.grid_radius, rays=rays.contiguous(), ts=ts)

    def _operators(self, rays, ts, r_d, pts=None):
        """the head's lookup node (the coefficients contracted with the ray's basis in the kernel) -> mask of a sparsified model -> split
        -> the head's activation (and linear scale) -> compositing"""
        kind, order = self._head_spec()
        pos = (None, ts) if pts is None else (pts.contiguous(), None)
        sh = {}
        if kind == "plv":
            raw, sh["sh"] = ag.VoxelPlvSampleFn.apply(self.densities, self.rgb, self.grid_radius, rays.contiguous(), *pos)
        elif kind == "sh":  # raw is the RGB head's [density | 3 colour logits]
            raw = ag.VoxelShSampleFn.apply(self.densities, self.rgb, order, self.grid_radius, rays.contiguous(), *pos)
        else:
            raw = ag.VoxelSampleFn.apply(self.densities, self.rgb, self.grid_radius, pos[0], rays.contiguous() if pts is None else None, pos[1])
        if self.live is not None:
            # dead samples: density -> a value whose softplus is exactly 0, colour parameters and sh -> 0; their gradient rows -> 0
            flags = self._live_flags(rays, ts, pts)
            raw = ag.VoxelMaskRowsFn.apply(raw, flags)
            sh = {k: ag.VoxelMaskRowsFn.apply(v, flags, 0.0) for k, v in sh.items()}
        if ag.needs_grad(raw):
            density, params = ag.SplitHeadFn.apply(raw)
        else:
            density, params = raw[..., 0].contiguous(), raw[..., 1:]
        return self._composite(density, self.brdf(params=params.contiguous(), view=r_d, **sh), ts, rays)

    def forward(self, rays):
        if self.steps_fine > 0: return self.forward_coarse_fine(rays, self.steps_fine)
        r_o, r_d, self.ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        self.ts_ray = None
        if self._fusable():
            return self._render(rays, self.ts)
        return self._operators(rays, self.ts, r_d)  # (positions o + t d are formed inside the lookup kernels, as na_compute_pts forms them)

    def forward_coarse_fine(self, rays, steps_fine: int, u=None):
        """Coarse -> fine rendering (`--voxel-steps-fine`, this build's flag).  A proposal pass reads the DENSITY grid alone at
        the `self.steps` shared steps (ops.voxel_proposal: the renderers' alpha / weights, no colour, no image, no graph -- the weights
        are constants); `steps_fine` new positions per ray are drawn from them by inverse cdf (ops.resample_ts; u: the caller's
        [steps_fine, *batch] draws, else one utils.rand draw per new sample in training mode, linspace in eval mode); the fine pass runs
        over every ray's own merged row, on the route `_fusable` picks: one launch in eval mode without gradients, else the operators
        (ops.compute_pts_rayts -> the head's lookup node -> CompositeRayTsFn).  There is no coarse image: the merged row contains every
        coarse step, which so receives its gradient through the fine image.  No gradient flows through the sample positions.
        Protocol of PlainNeRF's: `ts` the [steps] shared row, `ts_ray` [*batch, steps + steps_fine] what alpha / weights follow."""
        rays = rays.contiguous()
        r_o, r_d, ts, _ = compute_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        _, w = ops.voxel_proposal(rays, ts, self.densities.data, self.grid_radius)
        if u is None and self.training:
            u = utils.rand((steps_fine,) + tuple(rays.shape[:-1]), rays.device)
        ts_ray = ops.resample_ts(ts, w, steps_fine, u)
        if self._fusable():
            out = self._render(rays, ts_ray, per_ray=True)
        else:
            pts = ops.compute_pts_rayts(rays, ts_ray)
            out = self._operators(rays, ts_ray, r_d, pts=pts)
        self.ts, self.ts_ray = ts, ts_ray
        return out

    def from_pts(self, pts, ts, r_o, r_d, refl_latent=None, rays=None):
        if rays is None: rays = torch.cat([r_o, r_d], dim=-1).contiguous()
        self.ts, self.ts_ray = ts, None  # (positions that need a gradient get one from VoxelSampleFn: ops.voxel_sample_backward_pts)
        if self.live is None and self._fusable(pts):  # (the sparse launch forms o + t d itself: explicit points take the operators)
            return self._render(rays, ts, pts=pts.contiguous())
        return self._operators(rays, ts, r_d, pts=pts)


# ------------------------------------------------------------------------------------------------- VolSDF
class VolSDF(CommonNeRF):
    """src/nerf.py:861-1018, volume path only (uniform samples, Laplace density, relu, no sky term)."""

    def __init__(self, sdf, out_features: int = 3, occ_kind=None, integrator_kind="direct", w_transmission: bool = False,
                 scale_softplus: bool = False, **kwargs):
        super().__init__(**kwargs)
        assert occ_kind is None and not w_transmission, "occlusion / transmission are outside the volume path"
        self.sdf = sdf
        self.scale = nn.Parameter(torch.tensor(0.1))
        self.secondary = None
        self.out_features = out_features
        self.scale_softplus = scale_softplus

    @_f16x_policy
    def forward(self, rays):
        pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, self.t_near, self.t_far, self.steps, perturb=self._perturb())
        return self.from_pts(pts, self.ts, r_o, r_d, rays=rays)

    @property
    def intermediate_size(self): return self.sdf.intermediate_size

    def set_refl(self, r): self.sdf.refl = r

    @property
    def refl(self): return self.sdf.refl

    def _fusable_view(self, refl_latent=None):
        """View head + compositing as one kernel on the layer-synchronous engine (csrc/render_ls.hip, MODEL 2)"""
        r = self.sdf.refl
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        return (config.engine == "ls" and type(r) is refl.View and r.latent_size == 64 and r.out_features == 3
                and self.sdf.intermediate_size == 64 and getattr(r, "act_kind", None) in ops.SIGMOID and refl_latent is None
                and not self.training and not wants_grad)

    def _fusable_fourier_sdf(self):
        from . import sdf as _sdf
        from .neural_blocks import FourierEncoder
        u = self.sdf.underlying
        if type(u) is not _sdf.MLP or config.precision != "f16x" or config.engine != "ls":
            return False
        m = u.mlp
        return (type(m.enc) is FourierEncoder and m.enc.freqs == 128 and m.enc.input_dims == 3 and len(m.layers) == 6 and m.skip == 3
                and m.init.out_features == 256 and m.out.out_features == 65 and m.latent_size == 0 and m.act_name == "leaky_relu")

    def packed_fourier_sdf_ls(self, precision: str):
        lin = self.sdf.underlying.mlp._linears()
        return utils.packed_stream(self, "_packed_fourier_ls", precision, lin, lambda: ops.mlp_fourier_ls_pack(precision, *utils.linears_wb(lin)))

    def packed_view_ls(self, precision: str):
        lin = self.sdf.refl.mlp._linears()
        return utils.packed_stream(self, "_packed_view_ls", precision, lin, lambda: ops.render_view_ls_pack(precision, *utils.linears_wb(lin)))

    def packed_siren_ls(self, precision: str):
        siren, view = self.sdf.underlying.siren._linears(), self.sdf.refl.mlp._linears()
        return utils.packed_stream(self, "_packed_siren_ls", precision, siren + view,
                                   lambda: ops.render_volsdf_siren_ls_pack(precision, utils.linears_wb(siren), utils.linears_wb(view)))

    def from_pts(self, pts, ts, r_o, r_d, refl_latent=None, rays=None):
        if rays is None: rays = torch.cat([r_o, r_d], dim=-1).contiguous()
        from . import sdf as _sdf
        if (self._fusable_view(refl_latent) and not ag.needs_grad(pts) and type(self.sdf.underlying) is _sdf.SIREN):
            # the SIREN SDF network fits the layer-synchronous engine too: the whole model is ONE kernel (MODEL 3)
            scale = torch.nn.functional.softplus(self.scale.data) if self.scale_softplus else self.scale.data
            object.__setattr__(self, "scale_post_act", scale)
            prec = config.kernel_precision(has_f16x=True)
            out, self.alpha, self.weights = ops.render_volsdf_siren_ls(rays.contiguous(), ts, scale, self.packed_siren_ls(prec), prec,
                                                                        self.sdf.refl.act_kind, "black", True, pts=pts.contiguous())
            return out
        if self._fusable_view(refl_latent) and not ag.needs_grad(pts):
            # SDF network (fused MLP kernel) -> one kernel for Laplace density, View head and compositing: the colour,
            # density and [x | elev azim] tensors of the operator chain are never materialised
            if self._fusable_fourier_sdf():
                # f16x: the Fourier-MLP SDF network as ONE launch of the layer-synchronous engine (MODEL 5) instead of the
                # 3-product generic kernel; its 256 Fourier features are generated in the kernel
                enc = self.sdf.underlying.mlp.enc
                basis = (enc.basis.data * float(enc.extra_scale)).contiguous() if float(enc.extra_scale) != 1.0 else enc.basis.data
                raw = ops.mlp_fourier_ls(rays.contiguous(), ts, basis, self.packed_fourier_sdf_ls("f16x"), "f16x", pts=pts.contiguous())
            else:
                raw = self.sdf.underlying(pts)
            scale = torch.nn.functional.softplus(self.scale.data) if self.scale_softplus else self.scale.data
            object.__setattr__(self, "scale_post_act", scale)
            prec = config.kernel_precision(has_f16x=True)
            out, self.alpha, self.weights = ops.render_view_ls(rays.contiguous(), ts, raw, scale, self.packed_view_ls(prec), prec,
                                                                self.sdf.refl.act_kind, "black", True, pts=pts.contiguous())
            return out
        sdf_vals, latent = self.sdf.from_pts(pts)
        if ag.needs_grad(sdf_vals, self.scale):
            scale = torch.nn.functional.softplus(self.scale) if self.scale_softplus else self.scale
            density = ag.LaplaceDensityFn.apply(sdf_vals.contiguous(), scale)
        else:
            scale = torch.nn.functional.softplus(self.scale.data) if self.scale_softplus else self.scale.data
            density = ops.laplace_density(sdf_vals.contiguous(), scale)
        object.__setattr__(self, "scale_post_act", scale)  # plain attribute: never a second registration of the Parameter
        if self.sdf.refl.can_use_normal:
            raise NotImplementedError("normal-dependent reflectance needs autograd normals (row N1)")
        view = r_d.unsqueeze(0).expand_as(pts)
        rgb = self.sdf.refl(x=pts, view=view, normal=None, latent=latent)  # column slice of the SDF output: by pitch
        return self._composite(density, rgb, ts, rays, softplus=False, with_sky=False)

    def set_sigmoid(self, kind="thin"):
        if not hasattr(self, "sdf"): return
        self.sigmoid_kind = kind
        self.refl.act = load_sigmoid(kind)
        self.refl.act_kind = kind


# ------------------------------------------------------------------------------------------------- DynamicNeRF
class DynamicNeRF(utils.PackedCacheMixin, nn.Module):
    """src/nerf.py:1209-1303, Bezier-spline deformation (spline > 1), with `refl_latent` columns riding through the spline into the
    canonical model's reflectance (`make dnerf`: --dyn-refl-latent 3).  The delta path (spline = 0) raises at HEAD in the reference
    (SURVEY header table) and raises here too."""

    def __init__(self, canonical: CommonNeRF, spline: int = 0, refl_latent: int = 0):
        super().__init__()
        self.canonical = canonical
        self.spline = spline
        self.refl_latent = max(refl_latent, 0)
        if spline <= 1:
            raise NotImplementedError("DynamicNeRF without a spline is broken in the reference (self.dp unset); use --spline N>1")
        if self.refl_latent > 16:
            raise NotImplementedError("--dyn-refl-latent > 16 (na_bezier_warp_latent carries 1..16 columns)")
        self.spline_n = spline
        # src/nerf.py:1243-1249: with a reflectance latent the network also emits enc_rigidity | spline * refl_latent control rows
        out_dims, enc_layout = spline * 3 + 1, [0, 0]
        if self.refl_latent > 0:
            out_dims += spline * self.refl_latent + 1
            enc_layout = [1, self.refl_latent * spline]
        self.mlp_out_layout = [1, 3 * spline] + enc_layout
        self.delta_estim = SkipConnMLP(in_size=3, out=out_dims, num_layers=5, hidden_size=256, init="xavier",
                                       enc=HashEncoder())
        self.delta_estim.zero_last_layer()
        self._init_packed_hooks()

    @property
    def nerf(self): return self.canonical
    @property
    def refl(self): return self.canonical.refl
    @property
    def sdf(self): return getattr(self.canonical, "sdf", None)
    @property
    def intermediate_size(self): return self.canonical.intermediate_size + self.refl_latent
    def total_latent_size(self): return self.canonical.total_latent_size()
    def set_refl(self, r): self.canonical.set_refl(r)
    def set_bg(self, bg): self.canonical.set_bg(bg)

    @property
    def rigid_dp(self):
        """dp * rigidity (src/nerf.py:1278), only read by the flow visualisation and regularisers: formed on demand so
        the render path carries no extra elementwise pass over the samples."""
        return self.dp * self.rigidity

    def ffjord_div(self, e):
        """utils.div_approx(model.pts, model.rigid_dp) of runner.py:697-699 (src/utils.py:467-478) at the samples of the
        last forward: <e, d(rigid_dp)/d(pts) . e> per sample, e [T,B,H,W,3] the caller's randn draw.  The reference
        contracts a vector-Jacobian product with e; here the same number comes from one forward-mode sweep (hash_jvp ->
        tangent MLP -> ffjord_div kernels).  Like the reference's, the estimate has no graph."""
        est, dest = self.delta_estim.forward_with_direction_tangent(self.pts, e)
        return ops.ffjord_div(est, dest, self._tt, e.contiguous(), self.spline_n).reshape(self.pts.shape[:-1])

    def sum_jacobian_div(self):
        """`utils.divergence(model.pts, model.dp)` of runner.py:694-696 at the samples of the last forward, with its graph.  What
        the reference computes: `autograd(x, field)` differentiates the SUM of the field's three components
        (grad_outputs = ones, src/utils.py:266-277, 461-464) and the result is summed over the coordinates, i.e.
        sum_ij d dp_j / d x_i = sum_j (J . (1,1,1))_j -- the sum of all Jacobian entries, not its trace.  One direction
        tangent with e = (1,1,1) through the hash encoder and the deformation MLP (first-order graph nodes), then the
        spline, which is linear in its control points (the Bezier combination of the control points' tangents, by the warp
        kernel's own differentiable dp output).  The sweep runs in exact fp32 like the FFJORD tangent: the hash features'
        derivatives scale with the grid resolutions and largely cancel in the sum (split-bf16 GEMMs: 3 % of the result).
        [T,B,H,W,1]"""
        from . import config
        e = torch.ones_like(self.pts)
        with config.train_precision_as("fp32"):
            _, dest = self.delta_estim.forward_with_direction_tangent_graph(self.pts, e)
        dest = dest.reshape(*self.pts.shape[:-1], -1)
        _, ddp, _ = ag.BezierWarpFn.apply(dest.contiguous(), self.pts, self._tt, self.spline_n)
        return ddp.sum(dim=-1, keepdim=True)

    def _deformation_ls_mode(self):
        """the deformation network as ONE launch of the layer-synchronous engine (csrc/render_ls.hip MODEL 4) in inference: "bf16x3"
        (the three-product split, the parity default under precisions f16x / bf16x3: config.deformation_engine "ls-bf16x3"), "f16x"
        (the 1.5-product mode, opt-in: config.py says why) or None (the generic fused MLP / the training path)"""
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        d = self.delta_estim
        if not (config.engine == "ls" and config.deformation_engine != "generic" and not self.training and not wants_grad
                and isinstance(d.enc, HashEncoder) and len(d.layers) == 5 and d.init.out_features == 256 and d.skip == 3
                and d.latent_size == 0 and d.act_name == "leaky_relu"):
            return None
        n_out = d.out.out_features
        if config.precision == "f16x" and config.deformation_engine == "ls" and n_out <= 32:
            return "f16x"
        if config.precision in ("f16x", "bf16x3") and n_out <= 64:
            return "bf16x3"
        return None

    def _fusable_deformation(self):
        """the f16x instance of the above (opt-in)"""
        return self._deformation_ls_mode() == "f16x"

    def packed_deformation_ls(self, precision: str):
        lin = self.delta_estim._linears()
        return utils.packed_stream(self, "_packed_ls", precision, lin, lambda: ops.mlp_hash_ls_pack(precision, *utils.linears_wb(lin)))

    @_f16x_policy
    def forward(self, rays_t):
        rays, t = rays_t
        c = self.canonical
        self.pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, c.t_near, c.t_far, c.steps,
                                                        perturb=1 if self.training else 0)
        c.ts = self.ts
        tt = self._tt = t[None, :, None, None].expand(*self.pts.shape[:-1]).contiguous()
        mode = self._deformation_ls_mode()
        if mode is not None:
            est = ops.mlp_hash_ls(rays, self.ts, self.delta_estim.enc.tables(), self.packed_deformation_ls(mode), mode,
                                  self.delta_estim.out.out_features)
        else:
            est = self.delta_estim(self.pts)
        # (the reference hands from_pts a zero-width `enc` when refl_latent == 0, src/nerf.py:1272-1278, 1303: None here)
        enc = None
        if ag.needs_grad(est):
            res = ag.BezierWarpFn.apply(est.contiguous(), self.pts, tt, self.spline_n, self.refl_latent)
        else:
            res = ops.bezier_warp(est, self.pts, tt, self.spline_n, self.refl_latent)
        if self.refl_latent > 0:
            warped, self.dp, self.rigidity, enc = res
        else:
            warped, self.dp, self.rigidity = res
        return c.from_pts(warped, self.ts, r_o, r_d, refl_latent=enc, rays=rays)


    @_f16x_policy
    def render_keyframes(self, rays):
        """src/nerf.py:1305-1319 (runner.py:1019-1039 writes them as keyframe_NN.png): the scene rendered at each Bezier
        control point, canonical.from_pts(pts + p_k * rigidity).  The reference splits the 3*spline_n control
        coordinates into spline_n - 1 chunks, which torch.split rejects (sizes must sum to the dimension); the intended
        one frame per control point is produced here.  Keyframe k goes through the warp kernel with every control point
        set to p_k (the Bernstein weights sum to one, so dp = p_k)."""
        assert self.spline > 0
        c = self.canonical
        self.pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, c.t_near, c.t_far, c.steps, perturb=0)
        c.ts = self.ts
        est = self.delta_estim(self.pts)
        tt = torch.zeros(self.pts.shape[:-1], device=rays.device)
        frames = []
        for k in range(self.spline_n):
            est_k = torch.cat([est[..., :1]] + [est[..., 1 + 3 * k:4 + 3 * k]] * self.spline_n, dim=-1).contiguous()
            warped, _, self.rigidity = ops.bezier_warp(est_k, self.pts, tt, self.spline_n)
            frames.append(c.from_pts(warped, self.ts, r_o, r_d, rays=rays))
        return frames


# ------------------------------------------------------------------------------------------------- DynamicNeRFVoxel
class DynamicNeRFVoxel(nn.Module):
    """src/nerf.py:1526-1586: a D-NeRF with no MLP.  `ctrl_pts_grid` [S,S,S,3(spline-1)] (control points 1 .. spline-1 of a Bezier
    spline per voxel; control point 0 is zero) and `rigidity_grid` [S,S,S,1] are read by the canonical NeRFVoxel's lookup at the
    unwarped samples; warped = pts + bezier(t) * sigmoid(rigidity) goes to canonical.from_pts (csrc/dyn_voxel.hip).  The
    parameters keep the reference's names, so its state_dict loads.

    Routes of `forward((rays, t))`:
      eval, no gradients  ops.dyn_voxel_warp, then the canonical's one-launch render at the warped points (ops.voxel_render /
                          ops.voxel_plv_render by the head)
      otherwise           autograd.DynVoxelWarpFn, then the canonical's operator route, whose lookup returns the position gradient
    The reference marks `pts` as requiring a gradient in training for its two divergence regularisers; here pts stays a plain tensor and
    the Jacobian's quadratic forms come from a kernel of their own (`ffjord_div`, `sum_jacobian_div`: csrc/dyn_voxel_div.hip)."""

    def __init__(self, canonical=None, spline: int = 4):
        if not isinstance(canonical, NeRFVoxel):
            raise NotImplementedError(f"--dyn-model voxel deforms a voxel model (--model voxel), got {type(canonical).__name__}: the "
                                      "reference asserts the same (src/nerf.py:1532)")
        if spline is None or spline <= 1:
            raise ValueError(f"DynamicNeRFVoxel: spline {spline}, must have at least 2 control points (src/nerf.py:1533)")
        if spline > 11:
            raise NotImplementedError(f"DynamicNeRFVoxel: spline {spline} needs {3 * (spline - 1)} channels per voxel; the grid kernels "
                                      f"carry {ops.GRID_MAX_C} (spline <= 11)")
        super().__init__()
        self.canonical = canonical
        reso = canonical.resolution
        self.spline = spline
        self.ctrl_pts_grid = nn.Parameter(torch.randn([reso] * 3 + [3 * (spline - 1)]) * 0.3)
        self.rigidity_grid = nn.Parameter(torch.zeros([reso] * 3 + [1]))

    @property
    def nerf(self): return self.canonical
    @property
    def refl(self): return self.canonical.refl
    @property
    def sdf(self): return getattr(self.canonical, "sdf", None)
    @property
    def intermediate_size(self): return self.canonical.intermediate_size
    def total_latent_size(self): return self.canonical.total_latent_size()
    @property
    def densities(self): return self.canonical.densities
    @property
    def rgb(self): return self.canonical.rgb
    def set_refl(self, r): self.canonical.set_refl(r)
    def set_bg(self, bg): self.canonical.set_bg(bg)

    def _no_live(self, who):
        if getattr(self.canonical, "live", None) is not None:
            raise ValueError(f"DynamicNeRFVoxel.{who}: the canonical model holds a liveness table (NeRFVoxel.sparsify), which the "
                             "deformation's renderers and warp do not know; canonical.clear_live() first")

    def forward(self, rays_t):
        self._no_live("forward")
        rays, t = rays_t
        c = self.canonical
        if c.resolution != self.rigidity_grid.shape[0]:
            raise ValueError(f"DynamicNeRFVoxel: the canonical grids are {c.resolution}^3 and the deformation grids "
                             f"{self.rigidity_grid.shape[0]}^3 (the deformation grids have no resampling)")
        self.pts, self.ts, r_o, r_d, _ = compute_pts_ts(rays, c.t_near, c.t_far, c.steps, perturb=1 if self.training else 0)
        c.ts = self.ts
        tt = self._tt = t[None, :, None, None].expand(*self.pts.shape[:-1]).contiguous()
        if ag.needs_grad(self.ctrl_pts_grid, self.rigidity_grid):
            warped, self.dp, rigidity = ag.DynVoxelWarpFn.apply(self.ctrl_pts_grid, self.rigidity_grid, self.pts, tt, self.spline,
                                                                 c.grid_radius)
        else:
            warped, self.dp, rigidity = ops.dyn_voxel_warp(self.pts, tt, self.ctrl_pts_grid.data, self.rigidity_grid.data, self.spline,
                                                           c.grid_radius)
        self.rigidity = rigidity.unsqueeze(-1)
        return c.from_pts(warped, self.ts, r_o, r_d, rays=rays)

    def forward_maps(self, rays_t, depth: bool = True, flow: bool = True, rigidity: bool = True, acc: bool = False):
        """The test-time frame and its maps (runner.py:894-916) from ONE launch (ops.dyn_voxel_render): a dict of
        [B,H,W,.] tensors -- `rgb` [.,3] and, where asked for, `depth` [.,1] = sum w ts, `flow` [.,3] = sum w dp rigidity, `rigidity` [.,1]
        = sum w rigidity, `acc` [.,1] = sum of w[:-1] -- bit for bit what `forward` followed by render.depth_map / flow_map /
        rigidity_map / alpha_map gives, without the per-sample tensors.  Eval mode without gradients only.  The attributes of the last
        `forward` (`alpha`, `weights`, `dp`, `rigidity`, `pts` -- here and on the canonical model) are left untouched: nothing per sample
        is kept, and a regulariser or map that reads them still sees the last `forward`."""
        self._no_live("forward_maps")
        rays, t = rays_t
        c = self.canonical
        if self.training or ag.needs_grad(self.ctrl_pts_grid, self.rigidity_grid, c.densities, c.rgb):
            raise RuntimeError("DynamicNeRFVoxel.forward_maps renders in eval mode without gradients only (model.eval() under "
                               "torch.no_grad()); training goes through forward")
        if not c._fusable():
            raise RuntimeError(f"DynamicNeRFVoxel.forward_maps needs the canonical model's one-launch route: the per-voxel RGB head "
                               f"with 3 colour parameters (or the pos-linear-view / sph-har voxel head) and a named activation, got {type(c._head).__name__} / {c.rgb.shape[-1]} / "
                               f"{c.sigmoid_kind}")
        if c.resolution != self.rigidity_grid.shape[0]:
            raise ValueError(f"DynamicNeRFVoxel: the canonical grids are {c.resolution}^3 and the deformation grids "
                             f"{self.rigidity_grid.shape[0]}^3 (the deformation grids have no resampling)")
        _, _, ts, _ = compute_ts(rays, c.t_near, c.t_far, c.steps, perturb=0)
        want = [k for k, on in (("depth", depth), ("acc", acc), ("flow", flow), ("rigidity", rigidity)) if on]
        if c.bg == "random":
            want.append("weights")  # (the random sky is added behind the launch from the weights)
        tt = t[:, None, None].expand(rays.shape[:-1]).contiguous()
        kind, order = c._head_spec()
        res = ops.dyn_voxel_render(rays.contiguous(), tt, ts, c.densities.data, c.rgb.data, self.ctrl_pts_grid.data, self.rigidity_grid.data,
                                   self.spline, c.grid_radius, c._act_kind(), c._kernel_bg(), want=want, plv=kind == "plv",
                                   sh_order=order if kind == "sh" else None)
        weights = res.pop("weights", None)
        if weights is not None:
            kept, c.weights = c.weights, weights
            try:
                c._finish_sky(res["rgb"])
            finally:
                c.weights = kept
        return res

    @property
    def rigid_dp(self):
        """dp * rigidity (src/nerf.py:1585), formed on demand like DynamicNeRF's"""
        return self.dp * self.rigidity

    def _last_samples(self, who):
        if getattr(self, "pts", None) is None or getattr(self, "_tt", None) is None:
            raise RuntimeError(f"DynamicNeRFVoxel.{who} reads the sample positions and times of the last forward: render first")
        return self.pts, self._tt

    def ffjord_div(self, e):
        """utils.div_approx(model.pts, model.rigid_dp) of runner.py:698-699 (src/utils.py:467-478) at the samples of the last forward:
        <e, d(rigid_dp)/d(pts) . e> per sample [T,B,H,W], e [T,B,H,W,3] the caller's randn draw -- DynamicNeRF.ffjord_div's name, shape
        and meaning.  The Jacobian of the grid lookup is formed in closed form by one launch (ops.dyn_voxel_jac_quad);
        like the reference's, the estimate has no graph."""
        self._no_live("ffjord_div")
        pts, tt = self._last_samples("ffjord_div")
        with torch.no_grad():
            return ops.dyn_voxel_jac_quad(pts, tt, self.ctrl_pts_grid.data, self.rigidity_grid.data, self.spline,
                                          self.canonical.grid_radius, e.detach().reshape(pts.shape))

    def sum_jacobian_div(self):
        """`utils.divergence(model.pts, model.dp)` of runner.py:694-696 at the samples of the last forward, with its graph: the sum of
        all nine entries of d dp / d pts (DynamicNeRF.sum_jacobian_div's docstring says why it is not the trace), [T,B,H,W,1].  One
        launch, linear in ctrl_pts_grid, which is the only parameter its gradient reaches (autograd.DynVoxelJacQuadFn)."""
        self._no_live("sum_jacobian_div")
        pts, tt = self._last_samples("sum_jacobian_div")
        c = self.canonical
        if ag.needs_grad(self.ctrl_pts_grid):
            div = ag.DynVoxelJacQuadFn.apply(self.ctrl_pts_grid, pts, tt, None, self.spline, c.grid_radius)
        else:
            div = ops.dyn_voxel_jac_quad(pts, tt, self.ctrl_pts_grid.data, None, self.spline, c.grid_radius)
        return div.unsqueeze(-1)

    def spline_len(self, weights=None):
        """runner.py:784-787: the mean over the samples of the last forward of weights * arc_len(the sample's spline), the n control
        points interpolated at the unwarped `pts` with zero first (they exist only inside the kernels: autograd.DynVoxelSplineLenFn,
        DESIGN.md 3n).  weights [T, ...batch] (the canonical's compositing weights, used detached) or None for 1.  The per-sample mean
        for any batch size; the reference's own expression runs at one view only and equals it there."""
        self._no_live("spline_len")
        if getattr(self, "pts", None) is None:
            raise RuntimeError("DynamicNeRFVoxel.spline_len reads the sample positions of the last forward: render first")
        if weights is not None:
            if weights.numel() != self.pts.numel() // 3:
                raise ValueError(f"weights {tuple(weights.shape)}: one per sample of the last forward {tuple(self.pts.shape[:-1])} expected")
            weights = weights.detach().reshape(self.pts.shape[:-1]).contiguous()
        c = self.canonical
        if ag.needs_grad(self.ctrl_pts_grid):
            return ag.DynVoxelSplineLenFn.apply(self.ctrl_pts_grid, self.pts, weights, self.spline, c.grid_radius)
        return ops.dyn_voxel_spline_len(self.pts, self.ctrl_pts_grid.data, self.spline, c.grid_radius, weights)


# ------------------------------------------------------------------------------------------------- registries
def _experimental(name):
    def cons(*a, **k):
        raise NotImplementedError(f"model kind '{name}' is an experimental variant outside the hot path (SURVEY 2 row 7)")
    return cons


# src/nerf.py:1706-1720 / 1698-1704: same keys
model_kinds = {"tiny": TinyNeRF, "plain": PlainNeRF, "ae": NeRFAE, "volsdf": VolSDF, "voxel": NeRFVoxel,
               **{k: _experimental(k) for k in ["coarse_fine", "mpi", "rig", "hist"]}}
dyn_model_kinds = {"plain": DynamicNeRF, "voxel": DynamicNeRFVoxel, **{k: _experimental(k) for k in ["ae", "rig", "long"]}}


def load_nerf(args):
    """src/nerf.py:111-145."""
    from .sdf import load as load_sdf
    kwargs = {"mip": load_mip(args), "out_features": args.feature_space, "steps": args.steps, "t_near": args.near,
              "t_far": args.far, "intermediate_size": args.shape_to_refl_size, "sigmoid_kind": args.sigmoid_kind,
              "bg": args.bg}
    if args.model != "ae": args.latent_l2_weight = 0  # src/nerf.py:113
    cons = model_kinds.get(args.model, None)
    if cons is None: raise NotImplementedError(args.model)
    if args.model == "ae":
        kwargs["normalize_latent"] = getattr(args, "normalize_latent", False)
        kwargs["encoding_size"] = getattr(args, "encoding_size", 32)
    if args.model == "volsdf":
        kwargs["sdf"] = load_sdf(args, with_integrator=False)
        kwargs["occ_kind"] = getattr(args, "occ_kind", None)
    model = cons(**kwargs)
    if args.model == "ae" and getattr(args, "latent_l2_weight", 0) > 0: model.set_regularize_latent()  # src/nerf.py:143
    return model


def load_dyn(args, model, device=None):
    """src/nerf.py:1680-1696."""
    cons = dyn_model_kinds.get(args.dyn_model, None)
    if cons is None: raise NotImplementedError(f"Unknown dyn kind: {args.dyn_model}")
    if isinstance(model, NeRFAE) and cons is DynamicNeRF:
        raise NotImplementedError("--model ae under --dyn-model plain: training the deformation needs d(FourierEncoder)/d(position), which "
                                  "has no HIP backward (DESIGN.md 8); the reference's own pairing, --dyn-model ae, is broken at HEAD")
    if cons is DynamicNeRFVoxel:
        # (the reference passes refl_latent= to a constructor that does not take it, a TypeError: DESIGN.md 7; wired as evidently intended)
        if not isinstance(model, NeRFVoxel):
            raise NotImplementedError(f"--dyn-model voxel over --model {args.model}: the deformation grids are read with NeRFVoxel's cells, "
                                      "it needs --model voxel (the reference asserts the same, src/nerf.py:1532)")
        if args.dyn_refl_latent > 0:
            raise NotImplementedError(f"--dyn-refl-latent {args.dyn_refl_latent} under --dyn-model voxel: DynamicNeRFVoxel has no "
                                      "reflectance latent (src/nerf.py:1526-1531)")
        return cons(canonical=model, spline=args.spline)
    if isinstance(model, NeRFVoxel):
        raise NotImplementedError(f"--model voxel under --dyn-model {args.dyn_model}: only --dyn-model voxel deforms the sample positions of "
                                  "a voxel model (no fixture pins this pairing, DESIGN.md 8)")
    if isinstance(model, VolSDF) and cons is DynamicNeRF and args.dyn_refl_latent > 0:
        raise NotImplementedError("--dyn-refl-latent over --model volsdf: VolSDF.from_pts drops the reflectance latent (src/nerf.py:995-1013) "
                                  "while the head is built for it (runner.py:1182-1183), so the reference's first forward raises a shape error")
    return cons(canonical=model, spline=args.spline, refl_latent=args.dyn_refl_latent)
