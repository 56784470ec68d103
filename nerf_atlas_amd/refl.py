"""Colour heads on the hot path (src/refl.py:17-49,100-122,190-290,696-751): View, Positional, PosLinearView, SphericalHarmonic.
The relighting heads of the reference (Basic, Diffuse, CookTorrance, Rusin*, ...) keep their registry keys and
raise NotImplementedError (out of scope)."""
import torch
import torch.nn as nn

from . import autograd as ag
from . import ops
from . import utils
from .neural_blocks import FourierEncoder, HashEncoder, SkipConnMLP
from .utils import load_sigmoid


class IdentitySpace(nn.Module):
    def forward(self, x): return x
    @property
    def dims(self): return 3


class NoSpace(nn.Module):
    @property
    def dims(self): return 0


class Reflectance(nn.Module):
    """src/refl.py:100-122."""

    def __init__(self, act="thin", latent_size: int = 0, out_features: int = 3, bidirectional: bool = True, normal=None,
                 light=None, space=None):
        super().__init__()
        self.latent_size = latent_size
        self.out_features = out_features
        self.bidirectional = bidirectional
        self.act = load_sigmoid(act)
        self.act_kind = act if isinstance(act, str) else None  # (the fused renderers apply it in-kernel by name)

    @property
    def can_use_normal(self): return False

    @property
    def can_use_light(self): return False

    def to_voxel(self):
        """src/refl.py:129: (parameters per voxel, voxel_forward) of the heads that have a per-voxel form (NeRFVoxel.set_refl)"""
        raise NotImplementedError(f"{type(self)} does not have a voxel repr")


def _normalize(v):
    """F.normalize(view, dim=-1) on the GPU; one normalisation per RAY when the directions are broadcast along the
    sample axis."""
    if v.dim() > 1 and v.stride(0) == 0:
        return ops.normalize3(v[0].contiguous()).unsqueeze(0).expand(v.shape)
    return ops.normalize3(v.contiguous())


class View(Reflectance):
    """src/refl.py:190-207: act(mlp([x | elaz(view)], latent)); 4x256, sin activations, siren init."""

    def __init__(self, space=None, view="elaz", **kwargs):
        super().__init__(**kwargs)
        assert view == "elaz"
        self.mlp = SkipConnMLP(in_size=5, out=self.out_features, latent_size=self.latent_size, num_layers=4,
                               hidden_size=256, init="siren", activation=torch.sin)

    def forward(self, x, view, normal=None, light=None, latent=None):
        if (view.dim() == 3 and view.stride(0) == 0 and x.shape == view.shape and x.is_cuda and x.dtype == torch.float32
                and x.is_contiguous() and not view.requires_grad):
            # [T, R, 3] points, directions broadcast along the sample axis: the rows [x | elev, azim] by ONE kernel (round 5)
            from . import autograd as ag
            return self.act(self.mlp(ag.ViewInputFn.apply(x, view[0].contiguous()), latent))
        if view.dim() > 1 and view.stride(0) == 0:
            # directions broadcast along the sample axis (r_d.unsqueeze(0).expand_as(pts)): one elev/azim per RAY
            v = ops.view_elaz(view[0].contiguous()).unsqueeze(0).expand(view.shape[:-1] + (2,))
        else:
            v = ops.view_elaz(view.contiguous())
        return self.act(self.mlp(torch.cat([x, v], dim=-1), latent))


class Positional(Reflectance):
    """src/refl.py:230-245."""

    def __init__(self, space=None, **kwargs):
        super().__init__(**kwargs)
        self.mlp = SkipConnMLP(in_size=3, out=self.out_features, latent_size=self.latent_size, enc=HashEncoder(),
                               num_layers=5, hidden_size=256)

    def voxel_forward(self, params, view):
        """src/refl.py:240: the interpolated per-voxel parameters are the colour logits (self.act: autograd.SigmoidFn in a graph)"""
        return self.act(params)

    def to_voxel(self):
        """src/refl.py:241-243: the MLP is deleted, the grid holds `out_features` parameters per voxel"""
        del self.mlp
        return self.out_features, self.voxel_forward

    def forward(self, x, view, normal=None, light=None, latent=None):
        return self.act(self.mlp(x, latent))


class PosLinearView(Reflectance):
    """src/refl.py:248-290 (view='raw')."""

    def __init__(self, space=None, view="raw", intermediate_size=64, voxel_order=None, **kwargs):
        super().__init__(**kwargs)
        assert view == "raw"
        if voxel_order is not None and not (isinstance(voxel_order, int) and 0 <= voxel_order <= 4):
            raise ValueError(f"--voxel-refl-order must be an integer in 0..4, got {voxel_order!r}")
        self.voxel_order = voxel_order  # order of the per-voxel expansion `to_voxel` installs (None: no voxel form)
        self.im = intermediate_size
        self.pos = SkipConnMLP(in_size=3, out=self.out_features + self.im, latent_size=self.latent_size,
                               enc=HashEncoder(input_dims=3), num_layers=2, hidden_size=256)
        self.view = SkipConnMLP(in_size=6, out=1, latent_size=self.latent_size + self.im, num_layers=2,
                                hidden_size=128, init="siren", activation=torch.sin)

    def pos_linear_voxel_forward(self, params, view, sh=None):
        """src/refl.py:265-272: act(raw rgb) * (sigmoid(eval_sh(order, coefficients, normalize(view))) / 2 + 0.5).  NeRFVoxel's lookup
        contracts the coefficients with the ray's basis itself (csrc/voxel.hip), so `params` are the 3 interpolated colour
        parameters and `sh` the expansion in front of the sigmoid; the combination is pos_linear_combine's kernel."""
        if sh is None:
            raise ValueError("the pos-linear-view voxel head is evaluated by NeRFVoxel's lookup (ops.voxel_plv_sample): pass its `sh`")
        pos, lin = self.act(params), sh.unsqueeze(-1)
        if ag.needs_grad(lin, pos):
            return ag.PosLinearCombineFn.apply(lin, pos, self.out_features)
        return ops.pos_linear_combine(lin, pos, self.out_features)

    def to_voxel(self):
        """src/refl.py:273-280: both MLPs are deleted and the grid holds out_features + (order + 1)^2 parameters per voxel.  The
        reference hard-codes order 4 ("TODO where to pass this into this function?"); here --voxel-refl-order is that place, and
        without it the head has no voxel form."""
        if self.voxel_order is None:
            raise NotImplementedError("refl kind 'pos-linear-view' as a voxel head (src/refl.py:265-280: rgb | (order + 1)^2 spherical-"
                                      "harmonic coefficients per voxel) needs --voxel-refl-order K, K in 0..4 (the reference's is 4); "
                                      "without it --model voxel takes --refl-kind pos")
        if self.out_features != 3:
            raise NotImplementedError(f"the pos-linear-view voxel head with {self.out_features} colour parameters (3 have a kernel)")
        del self.pos
        del self.view
        self.order = order = self.voxel_order
        self.num_sh_coeffs = (order + 1) * (order + 1)
        return self.out_features + self.num_sh_coeffs, self.pos_linear_voxel_forward

    def forward(self, x, view, normal=None, light=None, latent=None):
        if hasattr(latent, "tensor") and not torch.is_tensor(latent):
            latent = latent.tensor()  # lazy IPE latent (utils.MipLatent): this head concatenates it, so materialise
        pos_all = self.act(self.pos(x, latent))  # [..., out_features + im]
        intermediate = pos_all[..., self.out_features:]
        view_latent = intermediate if latent is None else torch.cat([latent, intermediate], dim=-1)
        raw = self.view(torch.cat([x, _normalize(view)], dim=-1), view_latent)
        # (sigmoid(raw)/2 + 0.5) * pos_all[..., :out]
        if ag.needs_grad(raw, pos_all):
            return ag.PosLinearCombineFn.apply(raw, pos_all, self.out_features)
        return ops.pos_linear_combine(raw, pos_all, self.out_features)


class SphericalHarmonic(Reflectance):
    """src/refl.py:696-731: act(eval_sh(order, mlp(elaz(view), latent).reshape(..., 3, K), normalize(view))), K = (order + 1)^2; the MLP
    is 5 x 128, LeakyReLU, xavier, over [elaz(view) (2) | Fourier(elaz(view)) (256) | latent].  No light, no normal, no position.

    Exact fp32 in every precision mode (the head is 128 wide: no packed form for the fused MFMA kernels).  Two routes:
      hoisted  inference with the directions broadcast along the sample axis (PlainNeRF / DynamicNeRF): the 258 ray-constant input
               columns of `init`, `layers.0` and `layers.3` are multiplied once per RAY (ops.sh_view_terms) and enter the per-sample
               Linears as a per-ray bias (ops.linear_f32_rows over the latent columns, read where `first` left them); no [N, 2],
               [N, 256] or [N, 322] tensor exists.
      plain    training, or one direction per sample: the MLP through SkipConnMLP's own paths, then the expansion as one kernel
               (autograd.ShShadeFn / ops.sh_shade).
    The per-voxel form (`to_voxel`, --voxel-sh-order K) has no MLP: the grid holds 3 (K+1)^2 coefficients per voxel and
    NeRFVoxel's lookup contracts them with the ray's basis (csrc/voxel.hip)."""

    def __init__(self, space=None, order: int = 2, view="elaz", voxel_order=None, **kwargs):
        super().__init__(**kwargs)
        if not (isinstance(order, int) and 0 <= order <= 4):
            raise ValueError(f"spherical-harmonic order must be an integer in 0..4, got {order!r}")
        if voxel_order is not None and not (isinstance(voxel_order, int) and not isinstance(voxel_order, bool) and 0 <= voxel_order <= 4):
            raise ValueError(f"--voxel-sh-order must be an integer in 0..4, got {voxel_order!r}")
        self.voxel_order = voxel_order  # order of the per-voxel expansion `to_voxel` installs (None: no voxel form)
        if view != "elaz":
            raise NotImplementedError(f"SphericalHarmonic(view={view!r}): only the reference's default view encoding 'elaz' is built")
        self.order = order
        self.mlp = SkipConnMLP(in_size=2, out=self.out_features * (order + 1) * (order + 1), latent_size=self.latent_size,
                               enc=FourierEncoder(input_dims=2), num_layers=5, hidden_size=128, init="xavier")

    def voxel_forward(self, params, view):
        """NeRFVoxel's lookup has contracted the coefficients with the ray's basis (ops.voxel_sh_sample): `params` [..., 3] are the three
        expansions s_c, and the colour is their activation as `forward` applies it (the reference's voxel lambda applies none and
        never ran: DESIGN.md 7)"""
        return self.act(params)

    def to_voxel(self):
        """src/refl.py:715-722 as intended: the MLP is deleted and the grid holds 3 (K+1)^2 coefficients per voxel, channel-major (the
        layout of the reference's reshape(..., feats, -1)).  The reference's own form dies with torch.Size + list at src/refl.py:720;
        --voxel-sh-order K selects this one, and without it the head has no voxel form."""
        if self.voxel_order is None:
            raise NotImplementedError("refl kind 'sph-har' as a voxel head (3 (K + 1)^2 spherical-harmonic coefficients per voxel) needs "
                                      "--voxel-sh-order K, K in 0..4 (the reference's own form raises a TypeError, torch.Size + list, at "
                                      "src/refl.py:720); without it --model voxel takes --refl-kind pos")
        if self.out_features != 3:
            raise NotImplementedError(f"the sph-har voxel head with out_features = {self.out_features} colour channels (3 have a kernel)")
        del self.mlp
        self.order = order = self.voxel_order
        self.num_sh_coeffs = (order + 1) * (order + 1)
        return self.out_features * self.num_sh_coeffs, self.voxel_forward

    def _hoistable(self, view, latent):
        m = self.mlp
        return (self.out_features == 3 and view.is_cuda and view.dim() >= 2 and (view.stride(0) == 0 or view.shape[0] == 1)
                and torch.is_tensor(latent) and latent.is_cuda and latent.dtype == torch.float32
                and latent.shape[:-1] == view.shape[:-1] and latent.shape[-1] == m.latent_size and m.latent_size >= 1
                and not m.last_layer_act and len(m.layers) == 5 and m.skip == 3 and m.act_name == "leaky_relu"
                and isinstance(m.enc, FourierEncoder) and m.enc.input_dims == 2 and m.enc.freqs <= 128
                and m.init.out_features in (32, 64, 96, 128)
                and not ag.needs_grad(view, latent, *self.parameters()))

    def _latent_weights(self):
        """[init.weight[:, 258:], [layers.0.weight[:, :128] | [:, 386:]], the same of layers.3] as contiguous matrices: what is left of
        the three wide Linears once their view columns are per-ray terms (cached; rebuilt when a parameter changed)."""
        m = self.mlp
        lins = [m.init, m.layers[0], m.layers[3]]

        def pack():
            H, vc = m.init.out_features, m.in_size + m.enc.output_dims()
            ws = [m.init.weight.data[:, vc:].contiguous()]
            return ws + [torch.cat([l.weight.data[:, :H], l.weight.data[:, H + vc:]], dim=1).contiguous() for l in lins[1:]]
        return utils.packed_stream(self, "_lat_w", None, lins, pack)

    def _forward_hoisted(self, dirs, latent, kind):
        m = self.mlp
        H, vc = m.init.out_features, m.in_size + m.enc.output_dims()
        L = m.layers
        terms = ops.sh_view_terms(dirs, m.enc.basis.data, float(m.enc.extra_scale), m.init.weight.data[:, :vc], m.init.bias.data,
                                  L[0].weight.data[:, H:H + vc], L[0].bias.data, L[3].weight.data[:, H:H + vc], L[3].bias.data)
        w_init, w_0, w_3 = self._latent_weights()
        lat = latent  # (`first_out[..., 1:]`: a column slice, read with its row pitch)
        x = ops.linear_f32_rows(lat, w_init, None, "none", b_rows=terms[0])
        x = ops.linear_f32_rows(x, w_0, None, "leaky_relu", x1=lat, b_rows=terms[1])
        x = ops.linear_f32_rows(x, L[1].weight.data, L[1].bias.data, "leaky_relu")
        x = ops.linear_f32_rows(x, L[2].weight.data, L[2].bias.data, "leaky_relu")
        x = ops.linear_f32_rows(x, w_3, None, "leaky_relu", x1=lat, b_rows=terms[2])
        x = ops.linear_f32_rows(x, L[4].weight.data, L[4].bias.data, "leaky_relu")
        coeffs = ops.linear_f32_rows(x, m.out.weight.data, m.out.bias.data, "leaky_relu")
        return ops.sh_shade(coeffs, dirs, self.order, kind)

    def forward(self, x, view, normal=None, light=None, latent=None):
        if hasattr(latent, "tensor") and not torch.is_tensor(latent):
            latent = latent.tensor()  # lazy IPE latent (utils.MipLatent): these kernels read materialised columns
        if view.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("SphericalHarmonic: d(colour)/d(view direction) has no HIP backward")
        kind = self.act_kind if self.act_kind in ops.SIGMOID else "identity"
        finish = (lambda t: t) if self.act_kind in ops.SIGMOID else self.act  # (an activation passed as a callable runs behind the kernel)
        batches = view.shape[:-1]
        per_ray = view.dim() >= 2 and (view.stride(0) == 0 or view.shape[0] == 1)
        if self._hoistable(view, latent):
            dirs = view[0].reshape(-1, 3).contiguous()
            return finish(self._forward_hoisted(dirs, latent, kind).reshape(batches + (3,)))
        if per_ray:
            # directions broadcast along the sample axis: one elev / azim and one basis per RAY
            dirs = view[0].reshape(-1, 3).contiguous()
            v = ops.view_elaz(dirs).reshape((1,) + batches[1:] + (2,)).expand(batches + (2,))
        else:
            dirs = view.reshape(-1, 3).contiguous()
            v = ops.view_elaz(dirs).reshape(batches + (2,))
        coeffs = self.mlp(v, latent)
        if ag.needs_grad(coeffs):
            return finish(ag.ShShadeFn.apply(coeffs, dirs, self.order, kind))
        return finish(ops.sh_shade(coeffs, dirs, self.order, kind))


def _out_of_scope(name):
    def cons(*a, **k):
        raise NotImplementedError(f"refl kind '{name}' is a relighting head outside the volume-rendering hot path")
    return cons


# src/refl.py:733-751: same keys
refl_kinds = {
    "pos": Positional, "view": View, "pos-linear-view": PosLinearView, "sph-har": SphericalHarmonic,
    **{k: _out_of_scope(k) for k in ["view-light", "basic", "diffuse", "cook-torrance", "rusin", "rusin-helmholtz",
                                     "fourier", "weighted"]},
}


def load(args, refl_kind: str, space_kind: str, latent_size: int):
    """src/refl.py:17-49 (the light / weighted branches are out of scope)."""
    if space_kind not in ("identity", "surface", "none"):
        raise NotImplementedError()
    cons = refl_kinds.get(refl_kind, None)
    if cons is None:
        raise NotImplementedError(f"refl kind: {refl_kind}")
    if getattr(args, "light_kind", None) is not None:
        raise NotImplementedError("lights are outside the volume-rendering hot path")
    kwargs = {}
    if refl_kind == "sph-har":
        kwargs["order"] = getattr(args, "refl_order", 2)  # src/refl.py:33
        kwargs["voxel_order"] = getattr(args, "voxel_sh_order", None)  # this build's flag
    if refl_kind == "pos-linear-view":
        kwargs["voxel_order"] = getattr(args, "voxel_refl_order", None)  # this build's flag
    return cons(latent_size=latent_size, act=args.sigmoid_kind, out_features=args.feature_space,
                normal=getattr(args, "normal_kind", None), bidirectional=getattr(args, "refl_bidirectional", True), **kwargs)
