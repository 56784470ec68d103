"""Training and evaluation loops with the reference's recipe (runner.py:609-850 train, :855-995 test,
:1221-1322 main), restricted to what the five hot-path configs use: l2/l1/rmse loss and `--loss-fns ssim`, the loss wrapper `--color-spaces` /
`--tone-map` / `--gamma-correct-loss` / `--autogamma-correct-loss` (one HIP launch each way), Adam(eps 1e-7) with the
cosine schedule, random crops/views from Python's `random`, pixel jitter 0.1, stratified sampling and density noise
in training mode, `--volsdf-scale-decay`, `--delta-x-decay`, `--offset-decay`, `--sdf-eikonal` (SDF normals by forward-mode
tangents through the MLP), `--smooth-normals` in the reference's default epsilon-perturbation form (`--smooth-eps`,
`--smooth-eps-rng`, `--smooth-n-ord`), `--dyn-diverge-decay` (one differentiable direction tangent), `--ffjord-div-decay`
(forward-mode divergence estimate), `--voxel-tv-sigma` / `--voxel-tv-rgb` (total variation of NeRFVoxel's grids) and this build's
`--voxel-upsample ITER:RESO` and `--voxel-steps-fine N` (coarse -> fine sampling of --model voxel); over `--dyn-model voxel` also `--voxel-tv-bezier` / `--voxel-tv-rigidity`; `--smooth-normals --smooth-eps 0` (double backward) raises.
The test loop also renders the maps of `--depth-images` / `--flow-map` / `--rigidity-map` (render.render_frame_maps; one launch per tile for
the voxel D-NeRF) and, with `--msssim-loss`, computes SSIM per view and MS-SSIM of the test set (HIP kernels); `--render-over-time` and `--with-alpha` are read by runner.main.

Every forward and backward is a HIP kernel (nerf_atlas_amd/autograd.py); the parameter update is the reference's table of torch.optim
classes (`--opt-kind adam | sgd | adamw | rmsprop`, `--decay`), each with its step as one HIP launch (load_optim below).
With `replay_reference_rng=True` the stochastic tensors come from torch's CPU generator in the reference's order, so a run is comparable with the reference's iteration by iteration (tests/test_gpu_train.py
against tests/golden/train_parity_*.json).
"""
import argparse
import math
import os
import random
import re
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch.optim.optimizer import _get_scalar_dtype

from . import autograd as ag
from . import dist as na_dist
from . import config, loaders, nerf, refl, utils
from .render import render, render_frame, render_frame_maps

# the reference's CLI defaults for the fields used here (runner.py:38-424)
DEFAULTS = dict(
    data=None, data_kind="original", derive_kind=True, size=32, render_size=16, epochs=30000, batch_size=8,
    crop_size=16, test_crop_size=0, steps=64, steps_fine=0, mip=None, sigmoid_kind="upshifted", feature_space=3, model="plain",
    dyn_model=None, bg="black", learning_rate=5e-4, seed=1337, decay=0.0, loss_fns=["l2"], sched_min=5e-5,
    no_sched=False, shape_to_refl_size=64, refl_kind="view", refl_order=2, space_kind="identity", normal_kind=None,
    refl_bidirectional=True, sdf_kind="mlp", near=2.0, far=6.0, spline=0, dyn_refl_latent=0, time_gamma=False,
    volsdf_scale_decay=0.0, delta_x_decay=0.0, opt_step=1, clip_gradients=0.0, train_imgs=-1, serial_idxs=False,
    higher_end_chance=0, opt_kind="adam", light_kind=None, occ_kind=None, volsdf_alternate=False, test_white_bg=False,
    sdf_eikonal=0.0, ffjord_div_decay=0.0, offset_decay=0.0, dyn_diverge_decay=0.0, smooth_normals=0.0, smooth_eps=1e-3,
    smooth_eps_rng=False, smooth_n_ord=[2],
    neural_upsample=False, quiet=False,
    encoding_size=32, normalize_latent=False, latent_l2_weight=0.0,  # NeRFAE (runner.py:412-416)
    voxel_tv_sigma=0.0, voxel_tv_rgb=0.0, voxel_tv_bezier=0.0, voxel_tv_rigidity=0.0,  # runner.py:289-301
    voxel_random_spline_len_decay=0.0, spline_len_decay=0.0,  # runner.py:276-283
    voxel_upsample=[],  # this build's flag: ITER:RESO pairs, NeRFVoxel.upsample(RESO) at the start of iteration ITER
    voxel_refl_order=None,  # this build's flag: order K (0..4) of the per-voxel pos-linear-view head, the reference's hard-coded 4
    voxel_sh_order=None,  # this build's flag: order K (0..4) of the per-voxel spherical-harmonic colour head
    voxel_steps_fine=0,  # this build's flag: N resampled steps per ray, --model voxel renders coarse -> fine over steps + N
    voxel_sparsify=[],  # this build's flag: ITER:THRESH pairs, NeRFVoxel.sparsify(THRESH) at the start of iteration ITER
    depth_images=False, flow_map=False, rigidity_map=False, with_alpha=False,  # runner.py:360-392: maps next to the test frames
    render_over_time=-1, render_over_time_steps=100, render_over_time_end_sec=1.0,  # runner.py:252-261: a time sweep of one test camera
    msssim_loss=False,  # runner.py:359, :985-990: report ms-ssim next to the PSNR summary
    # runner.py:100-113, 552-594, 1159-1170: the layers the reference wraps around --loss-fns
    color_spaces=["rgb"], tone_map=False, gamma_correct_loss=1.0, autogamma_correct_loss=False,
)

def ssim_loss(x, ref):
    """--loss-fns ssim: 1 - mean over (n, c) of SSIM of the [B,h,w,3] crop against the label (ag.SSIMFn: HIP forward and backward).
    The reference's entry (runner.py:472, src/utils.py:186-188) hands the channel-last crop to a channel-first library and minimises
    the similarity itself; this is the intended dissimilarity over image channels."""
    if x.dim() != 4 or min(x.shape[1], x.shape[2]) < 11:
        raise ValueError(f"--loss-fns ssim needs a crop of at least 11 x 11 pixels (the SSIM window), got {tuple(x.shape)}: raise --crop-size")
    return 1 - ag.SSIMFn.apply(x, ref, "--loss-fns ssim").mean()


loss_map = {
    "l2": F.mse_loss,
    "l1": F.l1_loss,
    "rmse": lambda x, ref: F.mse_loss(x, ref).clamp(min=1e-10).sqrt(),
    "ssim": ssim_loss,
}


def make_args(**overrides) -> SimpleNamespace:
    """Namespace with the reference's defaults; mirrors the post-processing of runner.arguments() (:430-437)."""
    unknown = set(overrides) - set(DEFAULTS)
    assert not unknown, f"unknown arguments {sorted(unknown)}"
    a = SimpleNamespace(**{**DEFAULTS, **overrides})
    if not a.neural_upsample:
        a.render_size = a.size
        a.feature_space = 3
    if a.test_crop_size <= 0:
        a.test_crop_size = a.crop_size
    a.voxel_upsample = parse_voxel_upsample(a.voxel_upsample)
    a.voxel_sparsify = parse_voxel_sparsify(a.voxel_sparsify)
    return a


def parse_voxel_upsample(specs):
    """--voxel-upsample ITER:RESO [ITER:RESO ...] -> [(iteration, resolution)]: iterations strictly increasing, resolutions even."""
    plan = []
    for spec in specs:
        if isinstance(spec, str):
            m = re.fullmatch(r"(\d+):(\d+)", spec)
            if m is None:
                raise ValueError(f"--voxel-upsample {spec!r}: expected ITER:RESO, two non-negative integers")
            spec = (int(m.group(1)), int(m.group(2)))
        it, reso = (int(v) for v in spec)
        if reso < 2 or reso % 2 != 0:
            raise ValueError(f"--voxel-upsample {it}:{reso}: even resolutions only (NeRFVoxel's ids are floor(.) + resolution / 2)")
        if it < 0 or (plan and it <= plan[-1][0]):
            raise ValueError(f"--voxel-upsample: iterations must be increasing, got {it} after {[p[0] for p in plan]}")
        plan.append((it, reso))
    return plan


def parse_voxel_sparsify(specs):
    """--voxel-sparsify ITER:THRESH [ITER:THRESH ...] -> [(iteration, threshold)]: iterations strictly increasing, thresholds finite
    and >= 0 (0 keeps every voxel)."""
    plan = []
    for spec in specs:
        if isinstance(spec, str):
            m = re.fullmatch(r"(\d+):([^:\s]+)", spec)
            try:
                spec = (int(m.group(1)), float(m.group(2)))
            except (AttributeError, ValueError):
                raise ValueError(f"--voxel-sparsify {spec!r}: expected ITER:THRESH, a non-negative integer and a float >= 0") from None
        it, thresh = spec
        if isinstance(it, bool) or int(it) != it:
            raise ValueError(f"--voxel-sparsify {it!r}:{thresh!r}: the iteration is a non-negative integer")
        it, thresh = int(it), float(thresh)
        if not math.isfinite(thresh) or thresh < 0:
            raise ValueError(f"--voxel-sparsify {it}:{thresh}: the density threshold is a finite float >= 0")
        if it < 0 or (plan and it <= plan[-1][0]):
            raise ValueError(f"--voxel-sparsify: iterations must be increasing, got {it} after {[p[0] for p in plan]}")
        plan.append((it, thresh))
    return plan


def check_voxel_sparsify(args, is_dyn=False):
    """--voxel-sparsify ITER:THRESH: NeRFVoxel.sparsify during training of the static --model voxel; anything it cannot
    apply to raises by name.  Returns the plan."""
    plan = parse_voxel_sparsify(getattr(args, "voxel_sparsify", []) or [])
    if not plan:
        return plan
    if args.model != "voxel":
        raise ValueError(f"--voxel-sparsify over --model {args.model}: the flag marks the empty voxels of --model voxel")
    if getattr(args, "dyn_model", None) is not None or is_dyn:
        raise ValueError(f"--voxel-sparsify with --dyn-model {getattr(args, 'dyn_model', None)}: the deformation's renderers and warp do not "
                         "know the liveness table; the flag applies to the static --model voxel")
    return plan


def args_from_argv(argv) -> SimpleNamespace:
    """Parse the subset of the reference's command line that maps onto DEFAULTS (flags keep their spelling)."""
    p = argparse.ArgumentParser(allow_abbrev=False)
    p.add_argument("-d", "--data")
    for k, v in DEFAULTS.items():
        if k == "data":
            continue
        flag = "--" + k.replace("_", "-")
        if k == "learning_rate":
            p.add_argument("-lr", flag, type=float, default=v)
        elif isinstance(v, bool) and v:
            # defaults that are True (derive_kind, refl_bidirectional) get --flag / --no-flag so they can be switched off
            p.add_argument(flag, action=argparse.BooleanOptionalAction, default=True)
        elif isinstance(v, bool):
            p.add_argument(flag, action="store_true", default=False)
        elif isinstance(v, list):
            p.add_argument(flag, nargs="+", default=v, type=type(v[0]) if v else str)
        elif v is None:
            p.add_argument(flag, default=None, type=(int if k in ("spline", "voxel_refl_order", "voxel_sh_order") else str))
        else:
            p.add_argument(flag, type=type(v), default=v)
    p.add_argument("--nosave", action="store_true")
    p.add_argument("--notraintest", action="store_true")
    p.add_argument("--valid-freq", type=int, default=500)
    p.add_argument("--outdir", default="outputs/")
    ns = vars(p.parse_args(argv))
    return make_args(**{k: ns[k] for k in DEFAULTS if k in ns})


def check_voxel_refl_order(args):
    """--voxel-refl-order K: the order of the spherical-harmonic expansion PosLinearView.to_voxel installs per voxel (the reference
    hard-codes 4, src/refl.py:278).  Only meaningful for --model voxel --refl-kind pos-linear-view; anything else raises by name."""
    k = getattr(args, "voxel_refl_order", None)
    if k is None:
        return
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 4:
        raise ValueError(f"--voxel-refl-order {k!r}: an integer in 0..4 (the reference's head is order 4)")
    if args.model != "voxel":
        raise ValueError(f"--voxel-refl-order {k} over --model {args.model}: the flag sets the per-voxel head of --model voxel")
    if args.refl_kind != "pos-linear-view":
        raise ValueError(f"--voxel-refl-order {k} with --refl-kind {args.refl_kind}: the flag belongs to --refl-kind pos-linear-view")


def check_voxel_sh_order(args):
    """--voxel-sh-order K: the order of the per-voxel spherical-harmonic colour SphericalHarmonic.to_voxel installs (3 (K+1)^2
    coefficients per voxel).  Only meaningful for --model voxel --refl-kind sph-har; anything else raises by name.  --refl-order stays
    the MLP head's order."""
    k = getattr(args, "voxel_sh_order", None)
    if k is None:
        return
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 4:
        raise ValueError(f"--voxel-sh-order {k!r}: an integer in 0..4")
    if args.model != "voxel":
        raise ValueError(f"--voxel-sh-order {k} over --model {args.model}: the flag sets the per-voxel head of --model voxel")
    if args.refl_kind != "sph-har":
        raise ValueError(f"--voxel-sh-order {k} with --refl-kind {args.refl_kind}: the flag belongs to --refl-kind sph-har")


def check_voxel_steps_fine(args, is_dyn=False) -> int:
    """--voxel-steps-fine N: NeRFVoxel.steps_fine, coarse -> fine rendering of the static --model voxel (a density-only proposal pass,
    N resampled steps per ray, one fine image and no coarse one: DESIGN.md 3v).  Anything it cannot apply to raises by name.
    --steps-fine (PlainNeRF's joint coarse + fine loss) is another flag with other semantics and keeps refusing --model voxel."""
    n = getattr(args, "voxel_steps_fine", 0) or 0
    if isinstance(n, bool) or not isinstance(n, int) or n < 0:
        raise ValueError(f"--voxel-steps-fine {n!r}: the number of resampled steps per ray is a non-negative integer")
    if n == 0:
        return 0
    if int(getattr(args, "steps_fine", 0) or 0) != 0:
        raise ValueError(f"--voxel-steps-fine {n} with --steps-fine {args.steps_fine}: --steps-fine trains PlainNeRF on a joint coarse + fine "
                         "loss, --voxel-steps-fine renders --model voxel coarse -> fine with one image; give one of them")
    if args.model != "voxel":
        raise ValueError(f"--voxel-steps-fine {n} over --model {args.model}: the flag sets the sampling of --model voxel")
    if getattr(args, "dyn_model", None) is not None or is_dyn:
        raise ValueError(f"--voxel-steps-fine {n} with --dyn-model {getattr(args, 'dyn_model', None)}: the deformation is evaluated at shared "
                         "samples (a resampled deformation is a separate design); the flag applies to the static --model voxel")
    return n


def seed(s):
    """runner.py:1214-1218."""
    if s == -1:
        return
    torch.manual_seed(s)
    random.seed(s)
    np.random.seed(s)


def load_model(args, is_dyn=False, device="cuda"):
    """runner.py:1169-1211 for the supported kinds."""
    if args.model == "sdf":
        raise NotImplementedError("--model sdf (surface rendering) is outside the volume-rendering hot path")
    voxel_steps_fine = check_voxel_steps_fine(args, is_dyn)
    check_voxel_sparsify(args, is_dyn)
    steps_fine = int(getattr(args, "steps_fine", 0) or 0)
    if steps_fine < 0:
        raise ValueError(f"--steps-fine {steps_fine}: the number of resampled steps per ray cannot be negative")
    if steps_fine > 0:
        # coarse -> fine training: PlainNeRF with the View head over shared positions only
        why = (f"--model {args.model}" if args.model != "plain" else f"--refl-kind {args.refl_kind}" if args.refl_kind != "view" else
               f"--mip {args.mip}" if args.mip is not None else
               f"--dyn-model {args.dyn_model}" if (args.dyn_model is not None or is_dyn) else None)
        if why is not None:
            raise ValueError(f"--steps-fine {steps_fine} (coarse -> fine training) needs --model plain --refl-kind view without --mip "
                             f"and without a --dyn-model; got {why}")
    check_voxel_refl_order(args)
    check_voxel_sh_order(args)
    model = nerf.load_nerf(args)
    if is_dyn:
        model = nerf.load_dyn(args, model, device)
    # (--model ae: the head sees cat[encoded, intermediate], src/nerf.py:775-778, 832-836 -- the reference's runner drops the encoded
    # columns here, runner.py:1182-1183, and dies at the first forward: DESIGN.md 7)
    latent = model.intermediate_size + (args.encoding_size if args.model == "ae" else 0)
    model.set_refl(refl.load(args, args.refl_kind, args.space_kind, latent))
    if steps_fine > 0:
        model.steps_fine = steps_fine
    if voxel_steps_fine > 0:
        model.steps_fine = voxel_steps_fine
    return model.to(device)


def image_loss_torch(got, ref, loss_fns=("l2",), color_spaces=("rgb",), tone_map=False, gamma=1.0):
    """The loss ops.image_loss computes, composed from torch operators in the dtype and on the device of its arguments: what a CPU
    fit() trains with, and the wiring's reference in the tests (the definition: include/nerf_atlas_amd.h)."""
    from . import ops
    ops.image_loss_masks(loss_fns, color_spaces, gamma, "image_loss_torch")
    if gamma != 1.0:
        got = got.clamp(min=1e-10)
        got, ref = (got.sqrt(), ref.sqrt()) if gamma == 0.5 else (got.pow(gamma), ref.pow(gamma))
    if tone_map:
        got, ref = got / (1 + got), ref / (1 + ref)
    xyz = torch.tensor([[0.49, 0.31, 0.2], [0.17697, 0.8124, 0.01063], [0.0, 0.01, 0.99]], dtype=torch.float32, device=got.device).to(got.dtype)

    def space(name, v):
        if name == "rgb":
            return v
        if name == "luminance":
            return 0.2126 * v[..., 0:1] + 0.7152 * v[..., 1:2] + 0.0722 * v[..., 2:3]
        if name == "xyz":
            return (v.reshape(-1, 3) @ xyz.T) / 0.17697
        top = v.max(dim=-1).values  # hsv: the reference's rgb2hsv returns (0, 0, max)
        return torch.stack([torch.zeros_like(top), torch.zeros_like(top), top], dim=-1)
    total = 0
    for name in color_spaces:
        a, b = space(name, got), space(name, ref)
        total = total + sum(loss_map[k](a, b) for k in loss_fns) / len(loss_fns)
    return total / len(color_spaces)


def image_loss_is_default(args) -> bool:
    """none of --color-spaces / --tone-map / --gamma-correct-loss changes what --loss-fns alone computes"""
    return (list(getattr(args, "color_spaces", ["rgb"])) == ["rgb"] and not getattr(args, "tone_map", False)
            and getattr(args, "gamma_correct_loss", 1.0) == 1.0)


def load_loss_fn(args):
    if image_loss_is_default(args):
        fns = [loss_map[k] for k in args.loss_fns]
        assert len(fns) > 0, "must provide at least 1 loss function"
        if len(fns) == 1:
            return fns[0]
        return lambda x, ref: sum(fn(x, ref) for fn in fns) / len(fns)
    # the rest of the reference's wrapper (runner.py:566-594): one HIP launch each way (ag.ImageLossFn)
    from . import ops
    loss_fns, spaces, tone_map, gamma = list(args.loss_fns), list(args.color_spaces), bool(args.tone_map), args.gamma_correct_loss
    if "ssim" in loss_fns:
        raise ValueError("--loss-fns ssim together with --color-spaces / --tone-map / --gamma-correct-loss: the reference hands its "
                         "channel-first SSIM a colour-converted channel-last crop, there is nothing to reproduce (DESIGN.md 7)")
    ops.image_loss_masks(loss_fns, spaces, gamma, "load_loss_fn")
    gamma = float(gamma)

    def loss_fn(x, ref):
        if not x.is_cuda:
            return image_loss_torch(x, ref, loss_fns, spaces, tone_map, gamma)
        return ag.ImageLossFn.apply(x.contiguous(), ref.contiguous(), loss_fns, spaces, tone_map, gamma)
    return loss_fn


def auto_gamma(args, labels):
    """--autogamma-correct-loss (runner.py:1159-1170): --gamma-correct-loss from the labels' mean, on the host, once before training.
    A dynamic dataset's labels are a tuple; the mean is the image tensor's (the reference raises there: DESIGN.md 7)."""
    if not getattr(args, "autogamma_correct_loss", False):
        return
    images = labels[0] if type(labels) is tuple else labels
    weight = (math.log(0.5) / images.mean().log()).clamp(min=0).item()
    if weight < 0.55:
        weight = 0.5
    if weight >= 0.9:
        print(f"[note]: autogamma correct would darken/hardly change image ({weight}), ignoring.")
    else:
        args.gamma_correct_loss = weight
        print(f"[note]: autogamma correction weight is: {weight}")


class _OneLaunchStep:
    """In front of a torch.optim class: its step as ONE kernel (na_optim_step, csrc/optim.hip) for the parameter groups the kernel fits
    -- fp32 contiguous device tensors with dense gradients and the plain form of the rule (`_fits`) -- per element exactly the
    operations of torch's foreach implementation (torch/optim/*.py::_multi_tensor_*) in its order, each rounded like the ATen kernel
    rounds it (FMA_MASK: which multiply-adds ATen contracts; bit 0 lerp, 1 addcmul, 2 addcdiv, 3 add(alpha); tools/optim_probe.py).
    Same state keys, same state_dict: interchangeable with the torch class in both directions.  Any other group takes torch's own step
    for that group (the unhooked one: step hooks fire once per step)."""
    RULE = None       # ops.OPTIM_RULES
    TORCH = None      # the torch class whose step a group that does not fit takes
    STATE = ()        # the state tensors the kernel updates, in its order
    FMA_MASK = 0

    def _fits(self, group) -> bool:
        raise NotImplementedError

    def _launches(self, group, steps):
        """[(indices into the group's parameters with a gradient or None for all, rule, scalars, mask)]: one entry per launch, the
        scalars as torch's Python computes them; steps: the step count of every such parameter (None for a rule without state)"""
        raise NotImplementedError

    @staticmethod
    def _common_fit(group) -> bool:
        return (not group.get("maximize") and not group.get("capturable") and not group.get("differentiable") and not group.get("fused")
                and not isinstance(group["lr"], torch.Tensor))

    @staticmethod
    def _tensors_fit(ps, grads) -> bool:
        f32 = torch.float32
        for p, g in zip(ps, grads):
            if not (p.is_cuda and g.is_cuda and p.dtype is f32 and g.dtype is f32 and not p.is_sparse and not g.is_sparse
                    and p.is_contiguous() and g.is_contiguous()):
                return False
        return True

    def _count_steps(self, group, ps):
        """step += 1 for every parameter of the group, as ONE host operation where nothing changed since the last step: the step
        counts of the parameters that step together are 0-dim views of one host tensor (each still the `step` of torch's state: a
        0-dim tensor of torch's scalar dtype on the host).  Anything else -- a new parameter, a loaded state_dict, a step torch took
        -- is seen by identity, and the counts are gathered into a new tensor.  Returns the counts as floats."""
        cache = self.__dict__.setdefault("_na_steps", {})
        hit = cache.get(id(group))
        if hit is not None and len(hit[1]) == len(ps) and all(self.state[p]["step"] is v for p, v in zip(ps, hit[1])):
            buf = hit[0]
        else:
            buf = torch.tensor([float(self.state[p]["step"]) for p in ps], dtype=_get_scalar_dtype())
            views = buf.unbind(0)
            for p, v in zip(ps, views):
                self.state[p]["step"] = v
            cache[id(group)] = (buf, views)
        buf += 1
        return buf.tolist()

    @torch.no_grad()
    def step(self, closure=None):
        from . import ops
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            ps, grads = [], []
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    ps.append(p)
                    grads.append(g)
            if not ps or not self._fits(group) or not self._tensors_fit(ps, grads):
                self._torch_group_step(group)
                continue
            # every tensor is validated BEFORE any state is created or counted: a refused call leaves the optimiser as it was (a state
            # that does not exist yet will be zeros_like(p): p stands in for it; the gate above has looked at ps and grads)
            steps = None
            if self.STATE:   # (a rule without state tensors keeps no state at all, like torch's SGD, and has nothing left to validate)
                have = [self.state.get(p) for p in ps]
                ops.optim_check(self.RULE, ps, grads, *[[st[k] if st else p for p, st in zip(ps, have)] for k in self.STATE], known=2)
                for p, st in zip(ps, have):
                    if not st:  # (the torch class's _init_group)
                        st = self.state[p]
                        st["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                        for k in self.STATE:
                            st[k] = torch.zeros_like(p, memory_format=torch.preserve_format)
                steps = self._count_steps(group, ps)
            state = [[self.state[p][k] for p in ps] for k in self.STATE] + [[], []]
            for idx, rule, scalars, mask in self._launches(group, steps):
                pick = (lambda l: l) if idx is None else (lambda l: [l[i] for i in idx] if l else l)
                ops.optim_step(rule, pick(ps), pick(grads), pick(state[0]), pick(state[1]), scalars, mask, checked=True)
            # the kernel wrote the parameters through raw pointers: tell torch (an in-place update, like the torch class's own) -- the
            # packed weight streams of the fused renderers are keyed on the version counters (utils.pack_stamp) and a validation render
            # between two training steps would otherwise keep the weights of its first call
            torch.autograd.graph.increment_version(ps)
        return loss

    def _torch_group_step(self, group):
        """the torch class's step for ONE group (a group the kernel does not fit).  This runs inside the hooked step of this class: the
        torch class's own hook wrapper, where it has one, is taken off so that the step hooks fire once."""
        fn = self.TORCH.step
        if getattr(fn, "hooked", False):
            fn = fn.__wrapped__
        keep = self.param_groups
        try:
            self.param_groups = [group]
            fn(self)
        finally:
            self.param_groups = keep


class NaSGD(_OneLaunchStep, torch.optim.SGD):
    """torch.optim.SGD without momentum, dampening, nesterov and weight decay: p = p + (-lr) g.  No state."""
    RULE, TORCH, STATE, FMA_MASK = "sgd", torch.optim.SGD, (), 8

    def _fits(self, group):
        return (self._common_fit(group) and group["momentum"] == 0 and group["dampening"] == 0 and not group["nesterov"]
                and group["weight_decay"] == 0)

    def _launches(self, group, steps):
        return [(None, "sgd", [-group["lr"]], self.FMA_MASK)]


class NaRMSprop(_OneLaunchStep, torch.optim.RMSprop):
    """torch.optim.RMSprop, not centered, without momentum and weight decay.  State: `step`, `square_avg`."""
    RULE, TORCH, STATE, FMA_MASK = "rmsprop", torch.optim.RMSprop, ("square_avg",), 6

    def _fits(self, group):
        return self._common_fit(group) and group["momentum"] == 0 and not group["centered"] and group["weight_decay"] == 0

    def _launches(self, group, steps):
        alpha = group["alpha"]
        return [(None, "rmsprop", [alpha, 1 - alpha, group["eps"], -group["lr"]], self.FMA_MASK)]


class NaAdam(_OneLaunchStep, torch.optim.Adam):
    """torch.optim.Adam without amsgrad, with either form of weight decay (coupled: g + wd p in front of the update, the gradient tensor
    itself untouched; `decoupled_weight_decay`: p (1 - lr wd) in front of it).  State: `step`, `exp_avg`, `exp_avg_sq`.  FMA_MASK holds
    the three contractions of the update proper, DECAY_FMA the coupled decay's."""
    RULE, TORCH, STATE, FMA_MASK = "adam", torch.optim.Adam, ("exp_avg", "exp_avg_sq"), 7
    DECAY_FMA = 8

    def _fits(self, group):
        beta1, beta2 = group["betas"]
        # (1 - beta1 >= 0.5: ATen's lerp evaluates its other branch, b - (b - a)(1 - w), which the kernel does not)
        return (self._common_fit(group) and not group.get("amsgrad") and not isinstance(beta1, torch.Tensor)
                and not isinstance(beta2, torch.Tensor) and 1 - beta1 < 0.5)

    def _launches(self, group, steps):
        beta1, beta2 = group["betas"]
        lr, wd = group["lr"], group.get("weight_decay", 0)
        decoupled = bool(group.get("decoupled_weight_decay"))
        decay = (1 - lr * wd if wd != 0 else 1.0) if decoupled else wd
        out = []
        # one launch per distinct step count (parameters that joined later)
        counts = sorted(set(steps))
        for t in counts:
            bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
            out.append((None if len(counts) == 1 else [i for i, s in enumerate(steps) if s == t], "adamw" if decoupled else "adam",
                        [1 - beta1, beta2, 1 - beta2, bc2 ** 0.5, group["eps"], (lr / bc1) * -1, decay], self.FMA_MASK | self.DECAY_FMA))
        return out


class NaAdamW(NaAdam, torch.optim.AdamW):
    """torch.optim.AdamW (torch.optim.Adam with decoupled_weight_decay=True and the default decay 1e-2)."""
    TORCH = torch.optim.AdamW


OPT_KINDS = {  # runner.py:440-447: --opt-kind -> (this build's class, torch's)
    "adam": (NaAdam, torch.optim.Adam),
    "sgd": (NaSGD, torch.optim.SGD),
    "adamw": (NaAdamW, torch.optim.AdamW),
    "rmsprop": (NaRMSprop, torch.optim.RMSprop),
}


def load_optim(args, params):
    """runner.py:440-458: lr for every kind, eps 1e-7 except for sgd, --decay as Adam's (coupled) weight decay only."""
    if args.opt_kind == "uniform_adam":
        raise NotImplementedError("opt kind uniform_adam: the reference's UniformAdam (src/opt.py) is a dense cdist + solve per parameter, "
                                  "an experiment outside the training hot path")
    if args.opt_kind not in OPT_KINDS:
        raise NotImplementedError(f"unknown opt kind {args.opt_kind}")
    # torch's update as ONE launch where every parameter lives on the GPU (the classes above: the foreach form's operations, order and
    # rounding -- bit for bit the same trajectory, tests/test_gpu_train.py, tests/test_gpu_optim.py); NA_OPTIM=torch keeps torch's own
    # classes for every kind, NA_ADAM=torch for adam.  (torch's `fused=True` is NOT used: its update rounds differently and the
    # `--dyn-diverge-decay` recipe, whose end point measures accumulation precision, leaves the reference's basin with it --
    # profiles/r06/adam_fused_dnerf_div.log.)
    use_torch = os.environ.get("NA_OPTIM") == "torch" or (args.opt_kind == "adam" and os.environ.get("NA_ADAM") == "torch")
    cls = OPT_KINDS[args.opt_kind][1 if use_torch else 0]
    hyper = dict(lr=args.learning_rate, eps=1e-7)
    if args.opt_kind == "adam":
        hyper["weight_decay"] = args.decay
    if args.opt_kind == "sgd":
        del hyper["eps"]
    return cls(list(params), **hyper)


def offset_decay_term(model, curr_percent: float):
    """NR-NeRF offset regulariser of `make dnerf` (runner.py:633-636,777-781): exp_ratio * mean(weights.detach() *
    (|dp|^(2 - rigidity) + 3e-3 * rigidity)), exp_ratio = (1/100)^(1 - progress).  Elementwise loss arithmetic on the
    model's stored [T,B,H,W,*] outputs; its gradient enters the HIP backward through BezierWarpFn's dp / rigidity
    inputs."""
    exp_ratio = (1 / 100) ** (1 - curr_percent)
    norm_dp = torch.linalg.vector_norm(model.dp, dim=-1, keepdim=True).pow(2 - model.rigidity)
    reg = model.canonical.weights.detach()[None, ..., None] * (norm_dp + 3e-3 * model.rigidity)
    return exp_ratio * reg.mean()


def unset_voxel_tv(args, model):
    """set_per_run (runner.py:1135-1148): total-variation weights the model has no grid for are unset with the reference's warnings,
    never an error.  (The reference's second test forgets --voxel-tv-rigidity and dies in its first iteration when that weight alone is
    set on a non-voxel model; here it is unset with the others.)"""
    tv_dyn = args.voxel_tv_bezier > 0 or args.voxel_tv_rigidity > 0
    if isinstance(model, nerf.DynamicNeRFVoxel):
        return  # (all four grids exist: every weight is kept, runner.py:1137)
    if isinstance(model, nerf.NeRFVoxel):
        if tv_dyn:
            print("[warn]: model does not have bezier control points or rigidity for static scene")
            args.voxel_tv_bezier = args.voxel_tv_rigidity = 0
    elif args.voxel_tv_sigma > 0 or args.voxel_tv_rgb > 0 or tv_dyn:
        print("[warn]: model is not voxel, unsetting total variation")
        args.voxel_tv_sigma = args.voxel_tv_rgb = args.voxel_tv_bezier = args.voxel_tv_rigidity = 0


def upsample_voxels(model, opt, reso: int):
    """--voxel-upsample: NeRFVoxel.upsample(reso), then the two new Parameters take the old ones' places in the optimiser's groups and the
    old ones' state is deleted -- moments and step count restart for the grids (their shapes changed).  The schedule is left alone."""
    vox = model.nerf
    old = (vox.densities, vox.rgb)
    vox.upsample(reso)
    new = (vox.densities, vox.rgb)
    for group in opt.param_groups:
        for j, p in enumerate(group["params"]):
            for o, n in zip(old, new):
                if p is o:
                    group["params"][j] = n
    for o in old:
        opt.state.pop(o, None)
    opt.zero_grad()


def train(model, cam, labels, opt, args, sched=None, on_iter=None, rank: int = 0, world: int = 1):
    """runner.py:609-850.  Returns the list of per-iteration l2 losses (what save_losses() plots).
    world > 1: data-parallel replicas (one process per GPU, identical seeds): every rank draws the same views and
    crop, renders views idxs[rank::world], and the gradients are averaged with one flat RCCL all-reduce before the
    optimiser step (dist.allreduce_gradients); the reference's own --data-parallel is broken (SURVEY header table)."""
    dyn_voxel = isinstance(model, nerf.DynamicNeRFVoxel)
    sparsify_at = dict(parse_voxel_sparsify(getattr(args, "voxel_sparsify", []) or []))
    if sparsify_at and dyn_voxel:
        raise ValueError("--voxel-sparsify with --dyn-model voxel: the deformation's renderers and warp do not know the liveness table")
    if sparsify_at and not isinstance(model.nerf, nerf.NeRFVoxel):
        raise ValueError("--voxel-sparsify needs --model voxel (the flag calls NeRFVoxel.sparsify)")
    # ([iteration, threshold, live fraction of the table] per --voxel-sparsify event)
    sparsified = train.last_sparsify = []

    def sparsify(i):
        if i in sparsify_at:
            sparsified.append([i, sparsify_at[i], model.nerf.sparsify(sparsify_at[i])])

    if args.epochs == 0:
        sparsify(0)  # (ITER == epochs: before the test render)
        return []
    if dyn_voxel and not model.ctrl_pts_grid.is_cuda:
        # both terms contract d(rigid_dp)/d(pts) / d(dp)/d(pts) of the grid lookup (runner.py:694-699), which only csrc/dyn_voxel_div.hip
        # forms (NeRFVoxel.upsample's rule: no CPU implementation); raised before cam / labels are touched
        for flag in ("ffjord_div_decay", "dyn_diverge_decay"):
            if getattr(args, flag, 0):
                raise NotImplementedError(f"--{flag.replace('_', '-')} over --dyn-model voxel runs on the GPU only: d(dp)/d(pts) of the "
                                          "grid lookup is a HIP kernel (DESIGN.md 3q) and the model's grids are on "
                                          f"{model.ctrl_pts_grid.device}")
    if getattr(args, "dyn_diverge_decay", 0) > 0 and not hasattr(model, "sum_jacobian_div"):
        raise ValueError("--dyn-diverge-decay needs a dynamic model (--data-kind dnerf --dyn-model plain --spline N): the "
                         "reference reads model.pts / model.dp (runner.py:694-696)")
    if args.smooth_normals > 0 and args.smooth_eps <= 0:
        raise NotImplementedError("--smooth-normals with --smooth-eps 0 differentiates the normals again (double backward); "
                                  "the epsilon-perturbation form (--smooth-eps > 0, the reference's default) is implemented")
    if args.smooth_normals > 0 and not hasattr(model, "sdf"):
        raise ValueError("--smooth-normals needs an SDF model (--model volsdf)")
    if args.ffjord_div_decay and not hasattr(model, "ffjord_div"):
        raise ValueError("--ffjord-div-decay needs a dynamic model (--data-kind dnerf --dyn-model plain --spline N): the "
                         "reference reads model.pts / model.rigid_dp (runner.py:698-699)")
    if args.sdf_eikonal > 0 and not hasattr(model, "sdf"):
        raise ValueError("--sdf-eikonal needs an SDF model (--model volsdf)")
    if args.sdf_eikonal > 0 and isinstance(model, nerf.DynamicNeRF):
        raise NotImplementedError("--sdf-eikonal under a dynamic model: the reference's second, dynamic-only eikonal term (runner.py:804-808) "
                                  "adds the points to the (dp, enc) tuple of DynamicNeRF.time_estim and raises a TypeError in its first "
                                  "iteration; `make dnerf_volsdf` (makefile:127-133) trains without --sdf-eikonal")
    tv_dyn = dyn_voxel and (getattr(args, "voxel_tv_bezier", 0) > 0 or getattr(args, "voxel_tv_rigidity", 0) > 0)
    voxel_tv = getattr(args, "voxel_tv_sigma", 0) > 0 or getattr(args, "voxel_tv_rgb", 0) > 0 or tv_dyn
    upsample_at = dict(parse_voxel_upsample(getattr(args, "voxel_upsample", [])))
    if upsample_at and dyn_voxel:
        raise ValueError("--voxel-upsample with --dyn-model voxel: the reference has no resampling of ctrl_pts_grid / rigidity_grid "
                         "(src/nerf.py:1526-1586), so the deformation grids would keep the old resolution")
    if (voxel_tv or upsample_at) and not isinstance(model.nerf, nerf.NeRFVoxel):
        raise ValueError(f"{'--voxel-upsample' if upsample_at else '--voxel-tv-sigma / --voxel-tv-rgb'} needs --model voxel (fit() unsets the "
                         "total-variation weights of another model with the reference's warning)")
    for flag in ("spline_len_decay", "voxel_random_spline_len_decay"):
        # both read DynamicNeRFVoxel's ctrl_pts_grid; --dyn-model plain's own per-sample control points are not kept
        if getattr(args, flag, 0) > 0 and not dyn_voxel:
            raise ValueError(f"--{flag.replace('_', '-')} needs --dyn-model voxel (the term reads DynamicNeRFVoxel's ctrl_pts_grid), got "
                             f"{type(model).__name__}")
    len_on = getattr(args, "spline_len_decay", 0) > 0 or getattr(args, "voxel_random_spline_len_decay", 0) > 0
    device = next(model.parameters()).device
    loss_fn = load_loss_fn(args)
    times = None
    if type(labels) is tuple:
        times = labels[-1].to(device)
        labels = labels[0]
    batch_size = min(args.batch_size, labels.shape[0])
    cs = args.crop_size
    if cs != 0:
        get_crop = lambda: (random.randint(0, args.render_size - cs), random.randint(0, args.render_size - cs), cs, cs)
    else:
        get_crop = lambda: (0, 0, args.size, args.size)
    train_choices = range(labels.shape[0])
    if args.higher_end_chance > 0:
        train_choices = list(train_choices) + [0] * args.higher_end_chance + [labels.shape[0] - 1] * args.higher_end_chance
    next_idxs = (lambda i: [i % len(cam)] * batch_size) if args.serial_idxs else (lambda _: random.sample(train_choices, batch_size))

    if world > 1 and batch_size % world != 0:
        # equal shards: the mean of the per-replica mean losses is then the single-process batch loss
        raise ValueError(f"--batch-size {batch_size} must be a multiple of the {world} training replicas "
                         f"(every replica renders batch_size / world views per step)")
    losses = []
    reg_terms = train.last_reg_terms = []  # (the --dyn-diverge-decay term per iteration: a diagnostic next to the losses)
    # ([TV(densities), TV(rgb)] per iteration, + [TV(ctrl_pts_grid), TV(rigidity_grid)] for DynamicNeRFVoxel; device scalars: read after
    # the run, no sync in the loop)
    tv_terms = train.last_tv_terms = []
    # ([--spline-len-decay term, --voxel-random-spline-len-decay term] per iteration, NaN where a term is off; device scalars)
    len_terms = train.last_len_terms = []
    # (mean(alpha * div_approx^2) of --ffjord-div-decay per iteration, NaN where the flag is off; device scalars)
    ffjord_terms = train.last_ffjord_terms = []
    model.train()
    opt.zero_grad()
    for i in range(args.epochs):
        if i in upsample_at:
            upsample_voxels(model, opt, upsample_at[i])
        sparsify(i)  # (after an upsampling of the same iteration, which clears the table; the optimiser is left alone)
        idxs = next_idxs(i)
        if world > 1:
            idxs = na_dist.shard_batch(idxs, rank, world)
        ts = None if times is None else times[idxs]
        c0, c1, c2, c3 = crop = get_crop()
        ref = labels[idxs][:, c0:c0 + c2, c1:c1 + c3, :3].to(device)
        out, _rays = render(model, cam[idxs], crop, size=args.render_size, times=ts)
        loss = loss_fn(out, ref)
        assert loss.isfinite(), f"Got {loss.item()} loss"
        losses.append(loss.item())
        if getattr(args, "steps_fine", 0) > 0:
            # --steps-fine: NeRF's joint loss, the coarse image of the same network next to the fine one (the recorded loss stays the fine image's)
            loss = loss + loss_fn(model.nerf.coarse, ref)
        if getattr(args, "latent_l2_weight", 0) > 0:
            # runner.py:681 (which names a bare `latent_l2_weight`: the intended args.latent_l2_weight)
            loss = loss + args.latent_l2_weight * model.nerf.latent_l2_loss
        if args.volsdf_scale_decay > 0 and isinstance(model, nerf.VolSDF):
            loss = loss + args.volsdf_scale_decay * model.scale_post_act
        if args.delta_x_decay > 0:
            loss = loss + args.delta_x_decay * model.dp.norm(dim=-1).mean()
        if args.offset_decay > 0:
            loss = loss + offset_decay_term(model, i / args.epochs) * args.offset_decay
        reg_pts = reg_n = None
        if args.sdf_eikonal > 0 or args.smooth_normals > 0:
            # runner.py:683-689: one set of 10240 points 5 * randn for both SDF regularisers; normals by forward-mode
            # tangents ([3, N], differentiable w.r.t. the weights with first-order autograd)
            reg_pts = 5 * utils.randn(((1 << 13) * 5 // 4, 3), device)
            # The smoothing term is a DIFFERENCE of two normals <= eps = 1e-3 apart: |delta n| ~ 1e-2 against |n| ~ 4, so the
            # 2^-16 relative error of the split-bf16 GEMMs is 400x larger relative to it (measured against the reference's
            # run: per-view PSNR 0.22 dB off instead of 0.1).  Its two tangent sweeps run in exact fp32 (10 240 points:
            # 0.1 ms), like the FFJORD tangent; the eikonal term alone keeps the configured arithmetic.
            with config.train_precision_as("fp32" if args.smooth_normals > 0 else config.train_precision):
                reg_n = model.sdf.underlying.normals_tangent_major(reg_pts)
        if args.sdf_eikonal > 0:
            # runner.py:691-692: E[|d sdf/dx|] = 1
            loss = loss + args.sdf_eikonal * ag.EikonalFn.apply(reg_n)
        if args.dyn_diverge_decay > 0:
            # runner.py:694-696: utils.divergence(model.pts, model.dp).mean(), with its graph (forward-mode tangent nodes)
            div_term = model.sum_jacobian_div().mean()
            reg_terms.append(float(div_term.detach()))
            loss = loss + args.dyn_diverge_decay * div_term
        if args.ffjord_div_decay:
            # runner.py:697-700: FFJORD divergence estimate of the rigid deformation, e = randn_like(rigid_dp).  The
            # reference's div_approx builds no graph (src/utils.py:471-477: autograd.grad without create_graph), so the
            # term shifts the loss value and advances the RNG stream but contributes no gradient -- same here.
            e = utils.randn(tuple(model.pts.shape), device)
            exp_ratio = (1 / 100) ** (1 - i / args.epochs)
            div = model.ffjord_div(e).abs().square()
            ffjord_term = (model.canonical.alpha.detach() * div).mean()
            ffjord_terms.append(ffjord_term.detach())
            loss = loss + exp_ratio * args.ffjord_div_decay * ffjord_term
        else:
            ffjord_terms.append(float("nan"))
        if args.smooth_normals > 0:
            # runner.py:711-727, the epsilon-perturbation form "from unisurf": normals at the points and at points a random
            # direction of length eps away should agree.  Draw order of the reference: random.random() (with
            # --smooth-eps-rng), then randn_like(pts).
            s_eps = args.smooth_eps
            if args.smooth_eps_rng:
                s_eps = random.random() * s_eps
            perturb = F.normalize(utils.randn(tuple(reg_pts.shape), device), dim=-1) * s_eps
            with config.train_precision_as("fp32"):
                delta_n = reg_n - model.sdf.underlying.normals_tangent_major(reg_pts + perturb)  # [3, N]
            smoothness = 0
            for o in args.smooth_n_ord:
                smoothness = smoothness + torch.linalg.norm(delta_n, ord=int(o), dim=0).sum()
            loss = loss + args.smooth_normals * smoothness
        if voxel_tv:
            # runner.py:772-773: one draw of 32^3 voxels per term, densities first (every data-parallel rank draws the same ones from
            # the same seed, so the averaged gradient is the single-process one)
            tv_terms.append([float("nan")] * (4 if dyn_voxel else 2))
            if args.voxel_tv_sigma > 0:
                tv = nerf.total_variation(model.nerf.densities)
                tv_terms[-1][0] = tv.detach()
                loss = loss + args.voxel_tv_sigma * tv
            if args.voxel_tv_rgb > 0:
                tv = nerf.total_variation(model.nerf.rgb)
                tv_terms[-1][1] = tv.detach()
                loss = loss + args.voxel_tv_rgb * tv
            # runner.py:774-775: the deformation grids after them, in the reference's draw order
            if tv_dyn and args.voxel_tv_bezier > 0:
                tv = nerf.total_variation(model.ctrl_pts_grid)
                tv_terms[-1][2] = tv.detach()
                loss = loss + args.voxel_tv_bezier * tv
            if tv_dyn and args.voxel_tv_rigidity > 0:
                tv = nerf.total_variation(model.rigidity_grid)
                tv_terms[-1][3] = tv.detach()
                loss = loss + args.voxel_tv_rigidity * tv
        if len_on:
            len_terms.append([float("nan")] * 2)
            if args.spline_len_decay > 0:
                # runner.py:784-787: "only apply this to visible points": the samples of this iteration's forward, weighted by the
                # (detached) compositing weights
                term = model.spline_len(model.canonical.weights)
                len_terms[-1][0] = term.detach()
                loss = loss + args.spline_len_decay * term
            if args.voxel_random_spline_len_decay > 0:
                # runner.py:792-796: one draw of 16^3 voxels of ctrl_pts_grid (every data-parallel rank draws the same ones), weighted
                # by the flag itself -- the reference's line names --random-spline-len-decay
                term = nerf.arc_len_grid(model.ctrl_pts_grid)
                len_terms[-1][1] = term.detach()
                loss = loss + args.voxel_random_spline_len_decay * term
        if args.opt_step != 1:
            loss = loss / args.opt_step
        loss.backward()
        if world > 1:
            na_dist.allreduce_gradients(model.parameters(), world)
        if args.clip_gradients > 0:
            torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_gradients)
        if i % args.opt_step == 0:
            opt.step()
            opt.zero_grad()
        if sched is not None:
            sched.step()
        if on_iter is not None:
            on_iter(i, losses[-1])
    sparsify(args.epochs)  # (ITER == epochs: after the last step, before the test render)
    return losses


def test(model, cam, labels, args):
    """runner.py:855-995: every view rendered in test_crop_size tiles without jitter; per-image PSNR.  Returns (psnrs, frames); the
    per-view maps of the map flags are left in test.last_maps."""
    device = next(model.parameters()).device
    times = None
    if type(labels) is tuple:
        times = labels[-1].to(device)
        labels = labels[0]
    if args.test_crop_size <= 0:
        args.test_crop_size = args.render_size
    psnrs, gots = [], []
    # runner.py:894-916: with --depth-images / --flow-map / --rigidity-map every view's maps are rendered with it (one launch per tile for
    # the voxel D-NeRF) and kept per view, {name: [size,size,C]}, next to the frames; [] when no flag is set
    want = [k for k, flag in (("depth", "depth_images"), ("flow", "flow_map"), ("rigidity", "rigidity_map")) if getattr(args, flag, False)]
    maps = test.last_maps = []
    model.eval()
    for i in range(labels.shape[0]):
        ts = None if times is None else times[i:i + 1]
        exp = labels[i, ..., :3].to(device)
        if want:
            frame = render_frame_maps(model, cam[i:i + 1], args.render_size, args.test_crop_size, times=ts, want=want)
            got = frame.pop("rgb")
            maps.append(frame)
        else:
            got = render_frame(model, cam[i:i + 1], args.render_size, args.test_crop_size, times=ts)
        gots.append(got)
        psnrs.append(float(utils.mse2psnr(F.mse_loss(got, exp))))
    return psnrs, gots


def test_similarity(gots, labels):
    """--msssim-loss (runner.py:985-990, src/utils.py:190-195): (SSIM per view, MS-SSIM of the test set or None).  Both are means over
    the channels of a view; MS-SSIM is one float, the mean over views and channels as the reference's size_average computes it.  Frames
    whose smaller side is 160 or less print `msssim failed: <reason>` and leave None, as the reference's try / except does."""
    from . import ops
    if type(labels) is tuple:
        labels = labels[0]
    ssims, ms = [], []
    for got, exp in zip(gots, labels):  # (a view at a time: the test set of a scene does not fit twice next to the model)
        x, y = got[None, ..., :3], exp[None, ..., :3].to(got.device)
        ssims.append(float(ops.ssim(x, y, flag="--msssim-loss")[0].mean()))
        if ms is not None:
            try:
                ms.append(float(ops.ms_ssim(x, y, flag="--msssim-loss").mean()))
            except ValueError as e:
                print(f"msssim failed: {e}")
                ms = None
    return ssims, (None if not ms else float(np.mean(ms)))


def fit(args, device="cuda", replay_reference_rng=False, init=None, on_iter=None):
    """runner.main() (:1221-1322): seed, load the training set, build model + optimiser + schedule, train, load the
    test set, evaluate.  `init(model)` may overwrite the initial parameters (parity runs use procedural weights);
    with replay_reference_rng the torch stream is re-seeded with seed+1 after it, as tools/ref_train_fixture.py does."""
    rank, world = 0, 1
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:  # torchrun: one replica per GPU
        rank, world, local = na_dist.init_from_env()
        device = f"cuda:{local if torch.cuda.device_count() > local else 0}"  # debug: several replicas on one GPU
        torch.cuda.set_device(torch.device(device))
    seed(args.seed)
    labels, cam, _ = loaders.load(args, training=True)
    cam = cam.to(device)
    is_dyn = type(labels) is tuple
    model = load_model(args, is_dyn, device)
    if init is not None:
        init(model)
    prev = utils.random_source
    if replay_reference_rng:
        utils.set_random_source(utils.ReferenceStreamRandom())
        torch.manual_seed(args.seed + 1)
    try:
        if args.train_imgs > 0:
            labels = tuple(l[:args.train_imgs] for l in labels) if is_dyn else labels[:args.train_imgs]
            cam = cam[:args.train_imgs]
        model.nerf.steps, model.nerf.t_near, model.nerf.t_far = args.steps, args.near, args.far  # set_per_run :1048-1050
        unset_voxel_tv(args, model)
        auto_gamma(args, labels)
        opt = load_optim(args, model.parameters())
        sched = None if args.no_sched else torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=args.epochs,
                                                                                       eta_min=args.sched_min)
        losses = train(model, cam, labels, opt, args, sched=sched, on_iter=on_iter, rank=rank, world=world)
    finally:
        utils.set_random_source(prev)
    test_labels, test_cam, _ = loaders.load(args, training=False)
    test_cam = test_cam.to(device)
    if args.test_white_bg:
        model.set_bg("white")
    psnrs, gots = test(model, test_cam, test_labels, args)
    extra = {}
    if getattr(args, "msssim_loss", False):
        with torch.no_grad():
            extra["test_ssim"], extra["test_msssim"] = test_similarity(gots, test_labels)
    return dict(extra, model=model, losses=losses, sparsify=[list(e) for e in getattr(train, "last_sparsify", [])], reg_terms=list(getattr(train, "last_reg_terms", [])),
                tv_terms=[[float(v) for v in row] for row in getattr(train, "last_tv_terms", [])],
                ffjord_terms=[float(v) for v in getattr(train, "last_ffjord_terms", [])],
                len_terms=[[float(v) for v in row] for row in getattr(train, "last_len_terms", [])], test_psnr=psnrs, test_psnr_mean=float(np.mean(psnrs)), frames=gots,
                maps=list(getattr(test, "last_maps", [])), test_labels=test_labels, test_cam=test_cam, rank=rank, world=world)
