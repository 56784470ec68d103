#!/usr/bin/env python3
"""Train the REAL reference (/root/reference runner.main, CPU, in-process shims of SURVEY.md App. A) on the analytic
scene of tools/make_scene.py and record what the build's training step must reproduce (SURVEY 8(d) PSNR item (iii)):

    tests/golden/train_parity_<name>.json = { recipe (argv, seeds), per-iteration l2 losses, test-set PSNRs }

Determinism contract shared with nerf_atlas_amd/train.py:
  * the dataset is regenerated bit-identically by make_scene on either side;
  * initial parameters are procedural (oracle/procedural.proc_param keyed by state_dict name), written into the
    reference model right after runner.load_model;
  * `random.seed(seed)` (crops, view indices) and, after the parameters are written, `torch.manual_seed(seed + 1)`;
    every stochastic tensor of an iteration (pixel jitter u then v, stratified `rand[T]`, density noise) is then a
    draw from torch's CPU generator in the reference's order, which the build replays.

Runs only in the build container; nothing of the reference is copied or travels.

    python tools/ref_train_fixture.py plain [--epochs 300]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle.procedural import proc_param  # noqa: E402
from tools.make_scene import make_scene  # noqa: E402

REF = "/root/reference"

DYN_VOXEL_MAKE = ["--data-kind", "dnerf", "--near", "2", "--far", "6", "--model", "voxel", "--dyn-model", "voxel", "-lr", "1e-2", "--loss-fns", "l2",
                  "--spline", "4", "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4", "--voxel-tv-bezier", "1e-4", "--voxel-tv-rigidity", "1e-4",
                  "--higher-end-chance", "1", "--offset-decay", "30"]
DYN_VOXEL_MAKE_TAIL = ["--sigmoid-kind", "upshifted", "--voxel-random-spline-len-decay", "1e-5", "--refl-kind", "pos-linear-view"]
DYN_VOXEL_DIV_WEIGHT = os.environ.get("NA_DYN_VOXEL_DIV_WEIGHT", "0.1")   # (the committed fixture records the weight used in its argv)

RECIPES = {
    # name: (dynamic scene?, reference argv after the data flags)
    "plain": (False, ["--model", "plain", "--refl-kind", "view"]),
    # `make original` (reference makefile:8-13: --model plain --refl-kind pos -lr 2e-4 --loss-fns l2) on the small scene
    "original": (False, ["--model", "plain", "--refl-kind", "pos", "--loss-fns", "l2", "-lr", "2e-4"]),
    # `make nerf-sh` (reference makefile:64-72: --model plain --refl-kind sph-har --sigmoid-kind leaky_relu -lr 1e-3) on the small
    # scene, recorded with --epochs 200
    "nerf_sh": (False, ["--model", "plain", "--refl-kind", "sph-har", "--sigmoid-kind", "leaky_relu", "-lr", "1e-3"]),
    # `make ae` (reference makefile:380-384: --model ae -lr 1e-3 --no-sched --loss-fns l2, crop 20) on the small scene, with the
    # 32 + 32 wide latent of the class's own defaults; recorded with --epochs 200 --crop-size 20.  The reference's runner cannot run
    # `--model ae` as shipped (runner.py:1182-1183 installs a head without the encoded columns, the first forward raises): the
    # load_model hook below installs the head the class's constructor builds (src/nerf.py:775-778) and everything else is runner.main
    "ae": (False, ["--model", "ae", "--refl-kind", "view", "--loss-fns", "l2", "-lr", "1e-3", "--no-sched",
                   "--shape-to-refl-size", "32"]),
    # `make voxel` (reference makefile:30-34: --model voxel -lr 1e-2, no --refl-kind) with the head that has a voxel form (`pos`; the
    # shipped recipe's default `view` raises in View.to_voxel).  The rate is raised to 5e-2: the shipped 1e-2 reaches only 0.58 x its
    # starting loss in 300 iterations on this scene, too little for a parity run to pin anything.  The reference's runner cannot run
    # `--model voxel` as shipped (runner.py:1048 reads model.nerf.steps, NeRFVoxel has no `nerf`): the load_model hook below installs
    # the property and everything else is runner.main.  Recorded with --epochs 200 --size 32 --crop-size 16 --steps 32 --batch-size 4
    "voxel": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "-lr", "5e-2"]),
    # the `voxel` recipe plus both total-variation terms (runner.py:289-295, 772-773: two draws of 32^3 voxel indices per iteration
    # from torch's stream, densities first).  Recorded with the `voxel` recipe's flags; the fixture also carries that recipe's
    # trajectory (`losses_without_tv`, copied from train_parity_voxel.json after checking that the two argv differ in the two weights
    # only) and the two TV values of every iteration (`tv_terms`).  The weights are chosen so that the two trajectories separate by ten
    # times the parity bar (2e-3) within the first 50 iterations: the fixture then pins the terms, not only the stream position.
    "voxel_tv": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "-lr", "5e-2", "--voxel-tv-sigma", "0.02",
                         "--voxel-tv-rgb", "0.02"]),
    # the `voxel` recipe under the rest of the reference's loss wrapper (runner.py:552-594, src/utils.py:198-204, 279-314): two loss functions
    # in three colour spaces, tone-mapped, under a square-root gamma.  Recorded with the `voxel` recipe's flags; the fixture also carries
    # that recipe's trajectory (`losses_without_flags`, copied from train_parity_voxel.json after checking that the two argv differ in
    # the four loss flags only) and asserts that the two curves separate by ten times the parity bar (2e-4) within the first 10
    # iterations: the fixture then pins the loss, not only the stream position.
    "voxel_image_loss": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "rmse", "-lr", "5e-2", "--color-spaces", "rgb",
                                 "xyz", "hsv", "--tone-map", "--gamma-correct-loss", "0.5"]),
    # the `voxel` recipe under the other optimisers of the reference's table (runner.py:440-458: --opt-kind rmsprop / adamw / sgd; eps
    # 1e-7, AdamW with torch's default decay 1e-2).  Recorded with the `voxel` recipe's flags.  Each kind at a rate at which it learns on
    # this scene in 200 iterations: SGD at rates 1 .. 500 does not leave the start (the l2 gradient of a voxel is ~1e-6).
    "voxel_rmsprop": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "--opt-kind", "rmsprop", "-lr", "2e-2"]),
    "voxel_adamw": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "--opt-kind", "adamw", "-lr", "5e-2"]),
    "voxel_sgd": (False, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "--opt-kind", "sgd", "-lr", "5000"]),
    # `make dyn_voxel` (reference makefile: --model voxel --dyn-model voxel) with the head that has a voxel form here (`pos`; the shipped
    # recipe's pos-linear-view head is the `dyn_voxel_plv` recipe below), both deformation-grid total-variation terms (runner.py:774-775: two more draws of 32^3
    # voxel indices per iteration, after the sigma / rgb terms' place in the stream) and the NR-NeRF offset term through model.dp /
    # model.rigidity.  The rate is the `voxel` recipe's 5e-2, for that recipe's reason (the shipped 1e-2 barely leaves the start in 200
    # iterations on this scene).  The reference's load_dyn cannot build the class as shipped (src/nerf.py:1688-1696 passes refl_latent=
    # to a constructor that does not take it, a TypeError): the load_model hook below makes load_dyn drop the keyword for this class,
    # next to the `voxel` hook (model.nerf) that the canonical model needs; everything else is runner.main.  Recorded with the `voxel`
    # fixtures' flags: --epochs 200 --size 32 --crop-size 16 --steps 32 --batch-size 4
    "dyn_voxel": (True, ["--model", "voxel", "--refl-kind", "pos", "--loss-fns", "l2", "-lr", "5e-2", "--data-kind", "dnerf",
                         "--dyn-model", "voxel", "--spline", "4", "--voxel-tv-bezier", "0.02", "--voxel-tv-rigidity", "0.02",
                         "--offset-decay", "1"]),
    # `make dyn_voxel` with its shipped head: the `dyn_voxel` recipe with --refl-kind pos-linear-view (PosLinearView.to_voxel,
    # src/refl.py:273-280: 3 + 25 parameters per voxel, order 4).  Same rate, same recording flags; this build is given the argv plus
    # its own --voxel-refl-order 4
    "dyn_voxel_plv": (True, ["--model", "voxel", "--refl-kind", "pos-linear-view", "--loss-fns", "l2", "-lr", "5e-2", "--data-kind", "dnerf",
                             "--dyn-model", "voxel", "--spline", "4", "--voxel-tv-bezier", "0.02", "--voxel-tv-rigidity", "0.02",
                             "--offset-decay", "1"]),
    # `make dyn_voxel` AS SHIPPED (reference makefile:36-45), --ffjord-div-decay 0.3 included: every flag of its command line that bears
    # on training, in its order, with its values (the rate too: 1e-2).  Left out are the flags of the run's surroundings (-d, --size,
    # --epochs, --crop-size, --batch-size, --steps, --test-crop-size, --seed: this tool's; --save / --load / --save-freq / --loss-window /
    # --replace: checkpoints; --depth-images / --flow-map / --rigidity-map: panels of the test frames).  The reference adds 0 x the
    # --voxel-random-spline-len-decay term but draws its indices.  Recorded with the voxel fixtures' sizes and --epochs 60;
    # the fixture carries mean(alpha * div_approx^2) of every iteration (`ffjord_terms`) and, for the first five, the same number from an
    # fp64 copy of the model at the same positions with the same draw (`ffjord_terms64`)
    "dyn_voxel_make": (True, DYN_VOXEL_MAKE + ["--ffjord-div-decay", "0.3"] + DYN_VOXEL_MAKE_TAIL),
    # the same recipe with --dyn-diverge-decay in --ffjord-div-decay's place (`reg_terms`: the term of every iteration; `reg_terms64`: the
    # fp64 copy's, first five), and the loss curve of the recipe with neither flag (`losses_without_flag`, recorded with --out and folded in
    # with --base).  The weight is the smallest of 0.1, 1, 10, ... at which the last 10 losses of the two curves differ by more than 2e-3
    "dyn_voxel_div": (True, DYN_VOXEL_MAKE + ["--dyn-diverge-decay", DYN_VOXEL_DIV_WEIGHT] + DYN_VOXEL_MAKE_TAIL),
    "dyn_voxel_nodiv": (True, DYN_VOXEL_MAKE + DYN_VOXEL_MAKE_TAIL),   # (never committed: --out, then --base)
    "dnerf": (True, ["--model", "plain", "--refl-kind", "view", "--data-kind", "dnerf", "--dyn-model", "plain",
                     "--spline", "4"]),
    # `make dnerf`'s regularisers (reference makefile:106-114) on the small scene: NR-NeRF offset decay + the FFJORD
    # divergence estimate (whose randn_like draw advances the RNG stream every iteration), opt-step 3, upshifted sigmoid
    "dnerf_make": (True, ["--model", "plain", "--refl-kind", "pos-linear-view", "--data-kind", "dnerf", "--dyn-model",
                          "plain", "--spline", "6", "--higher-end-chance", "1", "--offset-decay", "60",
                          "--ffjord-div-decay", "0.5", "--sigmoid-kind", "upshifted", "--opt-step", "3"]),
    # `make dnerf` AS SHIPPED (makefile:106-114): the same + `--dyn-refl-latent 3` -- the deformation network's extra columns ride
    # through the spline into the PosLinearView head (round 6: src/nerf.py:1245-1248, 1272-1278, 1303)
    "dnerf_make_rl3": (True, ["--model", "plain", "--refl-kind", "pos-linear-view", "--data-kind", "dnerf", "--dyn-model",
                              "plain", "--spline", "6", "--higher-end-chance", "1", "--offset-decay", "60",
                              "--ffjord-div-decay", "0.5", "--sigmoid-kind", "upshifted", "--opt-step", "3",
                              "--dyn-refl-latent", "3"]),
    # the "exact divergence" regulariser of the deformation field (runner.py:694-696): autograd of model.dp w.r.t. model.pts with
    # create_graph -- a double backward through the hash encoder, the deformation MLP and the spline in the reference
    "dnerf_div": (True, ["--model", "plain", "--refl-kind", "view", "--data-kind", "dnerf", "--dyn-model", "plain",
                         "--spline", "4", "--dyn-diverge-decay", "0.05"]),
    "volsdf": (False, ["--model", "volsdf", "--sdf-kind", "siren", "--refl-kind", "view", "--near", "2", "--far", "6"]),
    # BASELINE config 5's other SDF network (`make volsdf`'s --sdf-kind mlp: Fourier-encoded SkipConnMLP, src/sdf.py:250-258) with
    # the eikonal term of the VolSDF recipes and the upshifted sigmoid (makefile:21-28, 127-133)
    # (`make dnerf_volsdf`, makefile:127-133 -- D-NeRF over a VolSDF canonical model with --sdf-eikonal -- cannot be recorded: the reference
    # raises at runner.py:807, `pts + dp` with dp the (dp, enc) tuple of DynamicNeRF.time_estim.)
    "volsdf_mlp": (False, ["--model", "volsdf", "--sdf-kind", "mlp", "--refl-kind", "view", "--near", "2", "--far", "6",
                           "--sdf-eikonal", "1e-5", "--sigmoid-kind", "upshifted", "-lr", "3e-4"]),
    # `make dnerf_volsdf` (makefile:127-133) without its --sdf-eikonal (see above: that term raises in the reference): D-NeRF with a
    # six-point spline over VolSDF's Fourier-encoded MLP SDF network and the PosLinearView head -- the deformation network learns
    # through d(FourierEncoder)/d(position).  Recorded short, on the smallest scene, for a test of a few seconds:
    # --epochs 30 --size 16 --crop-size 8 --steps 8
    "dnerf_volsdf": (True, ["--model", "volsdf", "--sdf-kind", "mlp", "--data-kind", "dnerf", "--dyn-model", "plain", "--spline", "6",
                            "--refl-kind", "pos-linear-view", "--sigmoid-kind", "upshifted", "--near", "2", "--far", "6", "-lr", "3e-4",
                            "--loss-fns", "l2"]),
    # the SDF regularisers of the reference's VolSDF recipes (makefile:85-95): eikonal + normal smoothing by the unisurf
    # epsilon perturbation with a random radius (one random.random() and two randn draws per iteration in the RNG streams)
    "volsdf_smooth": (False, ["--model", "volsdf", "--sdf-kind", "siren", "--refl-kind", "view", "--near", "2", "--far", "6",
                              "--sdf-eikonal", "1e-2", "--smooth-normals", "1e-2", "--smooth-eps-rng"]),
}


def shims():
    def stub(name, subs=()):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        for s in subs:
            sm = types.ModuleType(f"{name}.{s}")
            sm.__path__ = []
            sys.modules[f"{name}.{s}"] = sm
            setattr(m, s, sm)
    stub("torchvision", ["models", "transforms", "io"])
    tf = types.ModuleType("torchvision.transforms.functional")
    sys.modules["torchvision.transforms.functional"] = tf
    sys.modules["torchvision.transforms"].functional = tf
    stub("imageio")
    sys.path.insert(0, REF)
    nn.Module.cuda = lambda self, *a, **k: self


def fill_procedural(module):
    sd = module.state_dict()
    with torch.no_grad():
        for name, t in sd.items():
            if name.endswith("primes") or t.numel() == 0 or name == "scale" or name.endswith(".scale"):
                continue
            if name.startswith("delta_estim.out."):
                continue  # the deformation head keeps the reference's zero initialisation (src/nerf.py:1256)
            v = torch.from_numpy(proc_param(name, tuple(t.shape)))
            if name.endswith("basis"):
                v = v * (16.0 if "sdf" in name else 32.0)
            t.copy_(v.to(t.dtype))


def main():
    a = argparse.ArgumentParser()
    a.add_argument("name", choices=sorted(RECIPES))
    a.add_argument("--epochs", type=int, default=300)
    a.add_argument("--size", type=int, default=48)
    a.add_argument("--crop-size", type=int, default=24)
    a.add_argument("--batch-size", type=int, default=2)
    a.add_argument("--steps", type=int, default=48)
    a.add_argument("--seed", type=int, default=1337)
    a.add_argument("--threads", type=int, default=8)
    a.add_argument("--out", default=None, help="write the fixture here instead of tests/golden/train_parity_<name>.json "
                   "(sensitivity runs: the same recipe under another thread count = another summation order)")
    a.add_argument("--base", default=None, metavar="JSON", help="dyn_voxel_div: the dyn_voxel_nodiv run (made with --out JSON) whose losses are "
                   "recorded as `losses_without_flag`")
    a.add_argument("--add-run", default=None, metavar="JSON", help="no training: record another run of the same recipe (made with --threads N "
                   "--out JSON) in the committed fixture as `other_runs` -- the reference's own spread under another summation order")
    cfg = a.parse_args()
    if cfg.add_run:
        path = os.path.join(REPO, "tests", "golden", f"train_parity_{cfg.name}.json")
        fx, other = json.load(open(path)), json.load(open(cfg.add_run))
        assert fx["argv"] == other["argv"] and fx["seed"] == other["seed"] and fx["threads"] != other["threads"], "another run of the SAME recipe"
        run = dict(threads=other["threads"], test_psnr=other["test_psnr"], losses_first10=other["losses"][:10],
                   loss_linf=float(np.abs(np.array(fx["losses"]) - np.array(other["losses"])).max()),
                   psnr_linf=float(np.abs(np.array(fx["test_psnr"]) - np.array(other["test_psnr"])).max()))
        fx["other_runs"] = [r for r in fx.get("other_runs", []) if r["threads"] != run["threads"]] + [run]
        json.dump(fx, open(path, "w"), indent=1)
        print(f"{path}: the {other['threads']}-thread run differs by {run['loss_linf']:.2e} in the worst loss and {run['psnr_linf']:.4f} dB in the worst view")
        return
    torch.set_num_threads(cfg.threads)
    dynamic, model_argv = RECIPES[cfg.name]
    scene = dict(size=cfg.size, n_train=12, n_test=3, dynamic=dynamic)

    shims()
    import src.nerf as rnerf
    import src.utils as rutils
    rnerf.with_transmission = False
    rutils.git_hash = lambda: "nogit"
    import runner
    runner.git_hash = lambda: "nogit"
    runner.device = "cpu"
    runner.save_plot = lambda *a, **k: None

    captured = {"losses": None, "psnr": []}
    real_psnr = rutils.mse2psnr

    def mse2psnr(x):
        v = real_psnr(x)
        captured["psnr"].append(float(v))
        return v
    rutils.mse2psnr = mse2psnr
    real_div = rutils.divergence

    def divergence(x, field):  # (the --dyn-diverge-decay term per iteration: a diagnostic recorded next to the losses)
        v = real_div(x, field)
        captured.setdefault("reg_terms", []).append(float(v.mean().detach()))
        return v
    rutils.divergence = divergence
    real_div_approx = rutils.div_approx
    is_dyn_voxel_div = cfg.name in ("dyn_voxel_make", "dyn_voxel_div")

    def term64(kind, e=None):
        """the regulariser's term from an fp64 copy of the model run at the fp32 run's positions (and with its draw): the reference's own
        arithmetic in double at the same state.  The global random stream is left where it was."""
        m, m64, (rays, t) = captured["model"], captured["model64"], captured["rays_t"]
        state = torch.get_rng_state()
        m64.load_state_dict({k: v.detach().double() for k, v in m.state_dict().items()})
        m64.train(m.training)
        for k in ("steps", "t_near", "t_far"):  # (runner.set_per_run writes them after load_model)
            setattr(m64.canonical, k, getattr(m.canonical, k))
        pts = m.pts.detach().double()
        orig_pts, orig_randn = rnerf.compute_pts_ts, torch.randn_like

        def at_pts(*a_, **k_):  # (the fp32 run's perturbed steps too: alpha depends on them)
            _, _, r_o, r_d, mids = orig_pts(*a_, **k_)
            return pts.clone(), m.ts.detach().double(), r_o, r_d, mids
        rnerf.compute_pts_ts = at_pts
        try:
            with torch.enable_grad():
                m64((rays.double(), t.double()))
                if kind == "ffjord":
                    torch.randn_like = lambda x, **k_: e.double()
                    v = real_div_approx(m64.pts, m64.rigid_dp)
                    out = float((m64.canonical.alpha.detach() * v.abs().square()).mean())
                else:
                    out = float(real_div(m64.pts, m64.dp).mean())
        finally:
            rnerf.compute_pts_ts, torch.randn_like = orig_pts, orig_randn
            torch.set_rng_state(state)
        return out

    def div_approx(x, fn_x):  # (mean(alpha * div_approx^2) per iteration: what --ffjord-div-decay weights)
        state = torch.get_rng_state()
        v = real_div_approx(x, fn_x)
        if is_dyn_voxel_div:
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            e = torch.randn_like(fn_x)
            assert torch.equal(torch.get_rng_state(), after)
            m = captured["model"]
            terms = captured.setdefault("ffjord_terms", [])
            terms.append(float((m.canonical.alpha.detach() * v.detach().abs().square()).mean()))
            if len(terms) <= 5:
                captured.setdefault("ffjord_terms64", []).append(term64("ffjord", e))
        return v
    rutils.div_approx = div_approx
    if is_dyn_voxel_div:
        def divergence(x, field):
            v = real_div(x, field)
            terms = captured.setdefault("reg_terms", [])
            terms.append(float(v.mean().detach()))
            if len(terms) <= 5:
                captured.setdefault("reg_terms64", []).append(term64("divergence"))
            return v
        rutils.divergence = divergence
    real_tv = rnerf.total_variation

    def total_variation(grid, samples=32 ** 3):  # (the two --voxel-tv-* terms per iteration, densities then rgb)
        v = real_tv(grid, samples)
        captured.setdefault("tv_terms", []).append(float(v.detach()))
        return v
    rnerf.total_variation = total_variation
    runner.save_losses = lambda args, losses: captured.__setitem__("losses", list(losses))
    real_load_model = runner.load_model

    def load_model(args, light, is_dyn=False):
        if args.model == "voxel" and not hasattr(rnerf.NeRFVoxel, "nerf"):  # (see RECIPES["voxel"])
            rnerf.NeRFVoxel.nerf = property(lambda self: self)
        if getattr(args, "dyn_model", None) == "voxel":  # (see RECIPES["dyn_voxel"])
            cons = rnerf.dyn_model_kinds["voxel"]
            if not getattr(cons, "_drops_refl_latent", False):
                def dyn_voxel(canonical, spline=4, refl_latent=0, _cons=cons):
                    return _cons(canonical, spline=spline)
                dyn_voxel._drops_refl_latent = True
                rnerf.dyn_model_kinds["voxel"] = dyn_voxel
        m = real_load_model(args, light, is_dyn)
        if args.model == "ae":  # (see RECIPES["ae"])
            import src.refl as rrefl
            m.set_refl(rrefl.load(args, args.refl_kind, args.space_kind, args.encoding_size + m.intermediate_size))
        fill_procedural(m)
        if is_dyn_voxel_div:  # (term64 replays the iteration's forward)
            import copy
            captured["model"], captured["model64"] = m, copy.deepcopy(m).double()
            forward = m.forward
            m.forward = lambda rays_t: (captured.__setitem__("rays_t", rays_t), forward(rays_t))[1]
        torch.manual_seed(cfg.seed + 1)
        return m
    runner.load_model = load_model

    with tempfile.TemporaryDirectory() as td:
        data = make_scene(os.path.join(td, "scene"), **scene) + "/"
        out = os.path.join(td, "out")
        argv = ["-d", data, "--size", str(cfg.size), "--crop-size", str(cfg.crop_size), "--test-crop-size",
                str(cfg.size), "--batch-size", str(cfg.batch_size), "--steps", str(cfg.steps), "--epochs",
                str(cfg.epochs), "--seed", str(cfg.seed), "--nosave", "--quiet", "--notraintest", "--valid-freq",
                "1000000", "--outdir", out] + model_argv
        sys.argv = ["runner.py"] + argv
        t0 = time.time()
        runner.main()
        dt = time.time() - t0
        results = open(os.path.join(out, "results.txt")).read()
    printed = [float(line.split("PSNR")[1]) for line in results.splitlines() if "PSNR" in line]
    psnrs = captured["psnr"][-len(printed):]  # full precision of what results.txt rounds to 3 decimals
    assert all(abs(a - b) < 6e-4 for a, b in zip(psnrs, printed)), (psnrs, printed)
    mean = float(np.mean(psnrs))
    fixture = dict(
        what="reference runner.main() on the analytic scene; see tools/ref_train_fixture.py",
        name=cfg.name, scene=scene, seed=cfg.seed,
        argv=[x for x in argv if x not in (data, out, "-d", "--outdir")],
        recipe=dict(size=cfg.size, crop_size=cfg.crop_size, batch_size=cfg.batch_size, steps=cfg.steps,
                    epochs=cfg.epochs, model_argv=model_argv, lr=5e-4, sched_min=5e-5, adam_eps=1e-7, near=2.0, far=6.0),
        losses=[float(x) for x in captured["losses"]],
        test_psnr=psnrs, test_psnr_mean=mean, reg_terms=captured.get("reg_terms", []),
        torch=torch.__version__, threads=cfg.threads, wall_s=round(dt, 1),
    )
    if cfg.name in ("dyn_voxel_make", "dyn_voxel_div", "dyn_voxel_nodiv"):
        tv = captured["tv_terms"]
        fixture["tv_terms"] = [tv[i:i + 4] for i in range(0, len(tv), 4)]  # (densities, rgb, ctrl_pts_grid, rigidity_grid) per iteration
        for k in ("ffjord_terms", "ffjord_terms64", "reg_terms64"):
            if k in captured:
                fixture[k] = captured[k]
    if cfg.name == "dyn_voxel_div":
        base = json.load(open(cfg.base))
        drop = lambda av: [x for i, x in enumerate(av) if not (x == "--dyn-diverge-decay" or (i and av[i - 1] == "--dyn-diverge-decay"))]
        assert drop(fixture["argv"]) == base["argv"] and base["seed"] == cfg.seed, "record dyn_voxel_nodiv with the same flags"
        fixture["losses_without_flag"] = base["losses"]
        fixture["diverge_weight"] = float(DYN_VOXEL_DIV_WEIGHT)
        sep = float(np.abs(np.array(fixture["losses"][-10:]) - np.array(base["losses"][-10:])).max())
        fixture["separation_last10"] = sep
        print(f"dyn_voxel_div: weight {DYN_VOXEL_DIV_WEIGHT}: the curves with and without the term differ by {sep:.2e} in the last 10 losses")
        assert sep > 10 * 2e-4, "raise the weight (NA_DYN_VOXEL_DIV_WEIGHT) until the two reference curves separate"
    if cfg.name in ("dyn_voxel", "dyn_voxel_plv"):
        tv = captured["tv_terms"]
        fixture["tv_terms"] = [tv[i:i + 2] for i in range(0, len(tv), 2)]  # (ctrl_pts_grid, rigidity_grid) per iteration
    if cfg.name == "voxel_tv":
        tv = captured["tv_terms"]
        fixture["tv_terms"] = [tv[i:i + 2] for i in range(0, len(tv), 2)]
        with open(os.path.join(REPO, "tests", "golden", "train_parity_voxel.json")) as f:
            base = json.load(f)
        drop = lambda av: [x for i, x in enumerate(av) if not (x.startswith("--voxel-tv-") or (i and av[i - 1].startswith("--voxel-tv-")))]
        assert drop(fixture["argv"]) == base["argv"] and base["seed"] == cfg.seed, "record voxel_tv with the flags of the voxel fixture"
        fixture["losses_without_tv"] = base["losses"]
        sep = np.abs(np.array(fixture["losses"][:50]) - np.array(base["losses"][:50])).max()
        print(f"voxel_tv: the trajectories with and without the terms separate by {sep:.2e} within the first 50 iterations")
    if cfg.name == "voxel_image_loss":
        with open(os.path.join(REPO, "tests", "golden", "train_parity_voxel.json")) as f:
            base = json.load(f)
        loss_flags = ("--loss-fns", "--color-spaces", "--tone-map", "--gamma-correct-loss")

        def drop(av):  # (a loss flag and the values behind it)
            out, skipping = [], False
            for x in av:
                if x in loss_flags:
                    skipping = True
                elif skipping and not (x.startswith("-") and not re.fullmatch(r"-?[0-9.e+-]+", x)):
                    continue
                else:
                    skipping = False
                    out.append(x)
            return out
        assert drop(fixture["argv"]) == drop(base["argv"]) and base["seed"] == cfg.seed, "record voxel_image_loss with the flags of the voxel fixture"
        fixture["losses_without_flags"] = base["losses"]
        sep = float(np.abs(np.array(fixture["losses"][:10]) - np.array(base["losses"][:10])).max())
        fixture["separation_first10"] = sep
        print(f"voxel_image_loss: the curves with and without the four flags separate by {sep:.2e} within the first 10 iterations")
        assert sep > 10 * 2e-4, "the two reference curves do not separate: the fixture would pin only the stream position"
    path = cfg.out or os.path.join(REPO, "tests", "golden", f"train_parity_{cfg.name}.json")
    with open(path, "w") as f:
        json.dump(fixture, f, indent=1)
    print(f"{path}: {len(fixture['losses'])} iterations in {dt:.0f} s, loss {fixture['losses'][0]:.4f} -> "
          f"{np.mean(fixture['losses'][-20:]):.4f}, test PSNR {psnrs} mean {mean}")


if __name__ == "__main__":
    main()
