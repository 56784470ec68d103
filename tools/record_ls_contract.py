"""Record (and replay) the host contract of the layer-synchronous engine: tests/golden/ls_contract.json.

    python tools/record_ls_contract.py [--sections abi,pack,render] [--out PATH]

Three sections, all taken through the C ABI alone (nerf_atlas_amd._lib), so the same file runs against any commit:
  abi     return codes of every LS entry point for arguments that fail validation (no GPU needed: they return before any HIP call)
  pack    sha256 of every weight stream (entry x precision), packed into a zero-filled buffer
  render  sha256 of every output of every render / rows entry (entry x precision, want_weights on), 3 rays x 33 steps, and R = 0
Weights and inputs are integer arithmetic (element i of tensor k = (((i * 2654435761 + 40503 k) mod 65536) - 32768) / 2^shift), rays
come from na_raygen.  A render case is run twice and recorded only if both runs agree bit for bit (else it is listed under "unstable").
tests/test_ls_contract.py and tests/test_gpu_ls_contract.py replay the sections with the functions below.
"""
import argparse
import ctypes as C
import hashlib
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
import torch  # noqa: E402

from nerf_atlas_amd import _lib  # noqa: E402

DEFAULT_OUT = os.path.join(REPO, "tests", "golden", "ls_contract.json")
T = 33  # one step into the second 32-step block
ALL = ("bf16", "bf16x3", "f16", "f16x")
X = ("f16x",)
PREC = {p: i for i, p in enumerate(ALL)}
SIG_THIN, SIG_IDENTITY, BG_WHITE = 1, 11, 1
FAKE = 0x1000  # a non-null pointer for the abi cases: validation only looks at null-ness, and every case fails validation

_H = [(256, 256)]
FIRST = [(256, 38), (256, 294)] + 3 * _H + [(65, 256)]
VIEW = [(256, 69), (256, 325)] + 3 * _H + [(3, 256)]
MIP_FIRST = [(256, 134), (256, 390)] + 3 * _H + [(65, 256)]
MIP_VIEW = [(256, 165), (256, 421)] + 3 * _H + [(3, 256)]
POS = [(256, 102), (256, 358)] + 2 * _H + [(256, 358)] + _H + [(3, 256)]
TINY = [(256, 3), (256, 259)] + 2 * _H + [(256, 259)] + 2 * _H + [(4, 256)]
SIREN = [(256, 3), (256, 259)] + 2 * _H + [(256, 259)] + _H + [(65, 256)]
FOURIER = [(256, 259), (256, 515)] + 2 * _H + [(256, 515)] + 2 * _H + [(65, 256)]


def PLV(n): return [(256, 102 + n), (256, 358 + n), (256, 256), (67, 256), (128, 134 + n), (128, 262 + n), (128, 128), (1, 128)]
def HASH(n): return [(256, 38), (256, 294)] + 2 * _H + [(256, 294)] + _H + [(n, 256)]


# pack entries: symbol -> (precisions, Linear shapes per group, whether a bias may be None); called as
# symbol(precision, w0, b0[, w1, b1], *extra, packed, stream)
PACKS = {
    "na_render_ls_pack": (ALL, [FIRST, VIEW], True),
    "na_render_plain_mip_ls_pack": (X, [MIP_FIRST, MIP_VIEW], False),
    "na_render_plain_pos_ls_pack": (X, [FIRST, POS], False),
    "na_render_plain_plv_ls_pack": (X, [FIRST, PLV], False),    # extra: n_rl
    "na_render_tiny_ls_pack": (ALL, [TINY], True),
    "na_render_view_ls_pack": (ALL, [VIEW], True),
    "na_render_volsdf_siren_ls_pack": (ALL, [SIREN, VIEW], True),
    "na_mlp_hash_ls_pack": (("bf16x3", "f16x"), [HASH], True),  # extra: n_out
    "na_mlp_fourier_ls_pack": (X, [FOURIER], True),
}
HASH_N_OUT = {"bf16x3": (1, 32, 33, 64), "f16x": (1, 32)}

# render / rows entries: symbol -> (argument names in ABI order, precisions, pack symbol, workspace-size symbol, outputs)
_TAIL = ["prec", "sig", "bg", "alpha", "weights", "out"]
_WS = ["ws", "wsb", "stream"]
_OAW = ("out", "alpha", "weights")
RENDERS = {
    "na_render_plain_view_ls": (["rays", "pts", "R", "ts", "T", "tables", "packed"] + _TAIL + _WS, ALL, "na_render_ls_pack",
                                "na_render_ls_workspace_bytes", _OAW),
    "na_render_plain_view_ls_rayts": (["rays", "R", "ts_ray", "T", "tables", "packed"] + _TAIL + _WS, ALL, "na_render_ls_pack",
                                      "na_render_ls_workspace_bytes", _OAW),
    "na_train_plain_view_ls": (["rays", "pts", "R", "ts", "T", "tables", "packed", "sig", "planes", "view_rows", "density", "rgb_pre",
                                "out"] + _WS, ("bf16x3",), "na_render_ls_pack", "na_render_ls_workspace_bytes",
                               ("planes", "view_rows", "density", "rgb_pre", "out")),
    "na_render_plain_mip_ls": (["rays", "B", "H", "W", "ts", "T", "tables", "packed", "prec", "mip_kind", "min_deg", "max_deg", "t_end",
                                "sig", "bg", "alpha", "weights", "out"] + _WS, X, "na_render_plain_mip_ls_pack",
                               "na_render_ls_workspace_bytes", _OAW),
    "na_render_plain_pos_ls": (["rays", "pts", "R", "ts", "T", "tables", "tables2", "packed"] + _TAIL + _WS, X,
                               "na_render_plain_pos_ls_pack", "na_render_head_ls_workspace_bytes", _OAW),
    "na_render_plain_plv_ls": (["rays", "pts", "R", "ts", "T", "tables", "tables2", "rl", "rl_ld", "n_rl", "packed"] + _TAIL + _WS, X,
                               "na_render_plain_plv_ls_pack", "na_render_head_ls_workspace_bytes", _OAW),
    "na_render_tiny_ls": (["rays", "pts", "R", "ts", "T", "packed"] + _TAIL + ["stream"], ALL, "na_render_tiny_ls_pack", None, _OAW),
    "na_render_view_ls": (["rays", "pts", "R", "ts", "T", "feat", "feat_ld", "beta", "packed"] + _TAIL + _WS, ALL,
                          "na_render_view_ls_pack", "na_render_ls_workspace_bytes", _OAW),
    "na_render_volsdf_siren_ls": (["rays", "pts", "R", "ts", "T", "beta", "packed"] + _TAIL + _WS, ALL,
                                  "na_render_volsdf_siren_ls_pack", "na_render_ls_workspace_bytes", _OAW),
    "na_mlp_hash_ls": (["rays", "pts", "R", "ts", "T", "tables", "packed", "prec", "n_out", "y", "y_ld", "stream"], ("bf16x3", "f16x"),
                       "na_mlp_hash_ls_pack", None, ("y",)),
    "na_mlp_fourier_ls": (["rays", "pts", "R", "ts", "T", "basis", "packed", "prec", "y", "y_ld", "stream"], X,
                          "na_mlp_fourier_ls_pack", None, ("y",)),
}
POINTERS = {"rays", "pts", "ts", "ts_ray", "tables", "tables2", "packed", "alpha", "weights", "out", "ws", "feat", "beta", "rl", "y",
            "basis", "planes", "view_rows", "density", "rgb_pre"}
VALIDATION_CODES = (-1, -2, -3, -5)  # NA_EINVAL, NA_ENULL, NA_EUNSUPPORTED, NA_EWORKSPACE


# ------------------------------------------------------------------------------------------------------------- abi (no GPU)
def _abi_base(lib, name):
    fields, precs, _, ws_fn, _ = RENDERS[name]
    v = {f: FAKE for f in fields if f in POINTERS}
    v.update(R=1, T=T, B=1, H=2, W=2, prec=PREC[precs[0]], sig=SIG_THIN, bg=0, stream=0, feat_ld=65, rl_ld=3, n_rl=0, mip_kind=1,
             min_deg=0, max_deg=16, t_end=float("nan"), n_out=32, y_ld=65 if name == "na_mlp_fourier_ls" else 32)
    v["wsb"] = getattr(lib, ws_fn)(T, 4 if "B" in fields else 1) if ws_fn else 0  # (mip: R = B H W)
    return v


def _abi_render_cases(lib, name):
    """(case, argument values) of one render entry: every case changes the valid base so that a validation check fails"""
    fields, precs = RENDERS[name][:2]
    base = _abi_base(lib, name)
    nulls = {f: 0 for f in fields if f in POINTERS}
    empty = {"B": 0} if "B" in fields else {"R": 0}
    cases = [("T0", {"T": 0}), ("R0_null", {**nulls, **empty}), ("R1_null", nulls)]
    if "prec" in fields:
        cases += [(f"prec{p}", {"prec": p}) for p in (0, 1, 2, 3, 99) if p not in [PREC[q] for q in precs]]
        cases += [("null_and_prec99", {**nulls, "prec": 99})]
    if "sig" in fields:
        cases += [("sig-1", {"sig": -1}), ("sig12", {"sig": SIG_IDENTITY + 1})]
    if "bg" in fields:
        cases += [("bg2", {"bg": 2})]
    if "wsb" in fields:
        cases += [("ws_short", {"wsb": base["wsb"] - 1})]
        if "bg" in fields:
            cases += [("bg2_and_ws_short", {"bg": 2, "wsb": base["wsb"] - 1})]
    if "feat_ld" in fields:
        cases += [("feat_ld64", {"feat_ld": 64})]
    if "max_deg" in fields:
        cases += [("deg15", {"max_deg": 15}), ("H1", {"H": 1}), ("mip_kind2", {"mip_kind": 2})]
    if "n_rl" in fields:
        cases += [("n_rl4", {"n_rl": 4}), ("n_rl3_null_rl", {"n_rl": 3, "rl": 0}), ("n_rl3_ld2", {"n_rl": 3, "rl_ld": 2})]
    if "y_ld" in fields:
        cases += [("y_ld_short", {"y_ld": base["y_ld"] - 1})]
    if "n_out" in fields:
        cases += [("n_out0", {"n_out": 0}), ("n_out33_f16x", {"prec": PREC["f16x"], "n_out": 33, "y_ld": 33}),
                  ("n_out65_bf16x3", {"prec": PREC["bf16x3"], "n_out": 65, "y_ld": 65})]
    if "basis" in fields:
        cases += [("basis_unaligned", {"basis": FAKE + 4})]
    if name == "na_train_plain_view_ls":
        cases += [("rows_2p22", {"R": (1 << 22) // T + 1})]
    for tag, change in cases:
        v = dict(base, **change)
        yield tag, [v[f] for f in fields]


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _abi_pack_cases(name):
    precs, groups, _ = PACKS[name]
    extra = {"na_render_plain_plv_ls_pack": (0,), "na_mlp_hash_ls_pack": (32,)}.get(name, ())
    n = [len(g(0) if callable(g) else g) for g in groups]

    def args(prec, fill=FAKE, top=True, packed=FAKE, extra=extra):
        arrs = []
        for k in n:
            arrs += [_ptr_array([fill] * k) if top else None] * 2
        return [prec] + arrs + list(extra) + [packed, 0]
    ok = PREC[precs[-1]]
    cases = [("null", args(ok, top=False, packed=0)), ("null_packed", args(ok, packed=0)), ("null_weight", args(ok, fill=0)),
             ("null_and_prec99", args(99, top=False, packed=0))]
    cases += [(f"prec{p}", args(p)) for p in (0, 1, 2, 3, 99) if p not in [PREC[q] for q in precs]]
    if name == "na_render_plain_plv_ls_pack":
        cases += [("n_rl4", args(ok, extra=(4,))), ("n_rl-1", args(ok, extra=(-1,)))]
    if name == "na_mlp_hash_ls_pack":
        cases += [("n_out33_f16x", args(PREC["f16x"], extra=(33,))), ("n_out65_bf16x3", args(PREC["bf16x3"], extra=(65,))),
                  ("n_out0", args(ok, extra=(0,)))]
    return cases


def run_abi():
    """{case id: return code} of every LS entry point; the size queries are recorded as their values"""
    lib = _lib.load()
    rec = {}
    for name in RENDERS:
        for tag, args in _abi_render_cases(lib, name):
            rc = getattr(lib, name)(*args)
            assert rc in VALIDATION_CODES or (tag == "R0_null" and rc == 0), (name, tag, rc)  # nothing here may reach a launch
            rec[f"{name}/{tag}"] = rc
    for name in PACKS:
        for tag, args in _abi_pack_cases(name):
            rc = getattr(lib, name)(*args)
            assert rc in VALIDATION_CODES, (name, tag, rc)
            rec[f"{name}/{tag}"] = rc
        for p in (0, 1, 2, 3, 99):
            rec[f"{name.replace('_pack', '_packed_bytes')}/prec{p}"] = getattr(lib, name.replace("_pack", "_packed_bytes"))(p)
    for fn in ("na_render_ls_workspace_bytes", "na_render_head_ls_workspace_bytes"):
        for t, r in ((0, 1), (T, -1), (T, 0), (T, 3)):
            rec[f"{fn}/T{t}_R{r}"] = getattr(lib, fn)(t, r)
    return rec


# ------------------------------------------------------------------------------------------------------------- pack / render (GPU)
def tensor(k, shape, shift, device):
    n = math.prod(shape)
    i = torch.arange(n, dtype=torch.int64)
    v = ((i * 2654435761 + 40503 * k) % 65536 - 32768).to(torch.float32) / float(1 << shift)
    return v.reshape(shape).to(device)


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def pack(lib, name, prec, shift, extra=(), no_bias=False):
    """the stream of one pack entry in a zero-filled buffer (Linear j of group g: tensors 100 g + 2 j and + 1; no_bias: the odd Linears'
    biases are None)"""
    dev = torch.device("cuda", 0)
    keep, arrs = [], []
    for g, shapes in enumerate(PACKS[name][1]):
        shapes = shapes(*extra) if callable(shapes) else shapes
        ws = [tensor(100 * g + 2 * j, s, shift, dev) for j, s in enumerate(shapes)]
        bs = [None if no_bias and j % 2 else tensor(100 * g + 2 * j + 1, (s[0],), shift, dev) for j, s in enumerate(shapes)]
        keep += [ws, bs]
        arrs += [_ptr_array([w.data_ptr() for w in ws]), _ptr_array([0 if b is None else b.data_ptr() for b in bs])]
    nbytes = getattr(lib, name.replace("_pack", "_packed_bytes"))(PREC[prec])
    assert nbytes > 0, (name, prec)
    packed = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    rc = getattr(lib, name)(PREC[prec], *arrs, *extra, packed.data_ptr(), _stream())
    assert rc == 0, (name, prec, rc, lib.na_last_error())
    torch.cuda.synchronize()
    return packed


def pack_cases():
    """(case id, entry, precision, extra, no_bias)"""
    for name, (precs, _, none_ok) in PACKS.items():
        for prec in precs:
            extras = [(n,) for n in HASH_N_OUT[prec]] if name == "na_mlp_hash_ls_pack" else \
                [(0,), (3,)] if name == "na_render_plain_plv_ls_pack" else [()]
            for extra in extras:
                tag = f"{name}/{prec}" + "".join(f"/{e}" for e in extra)
                yield tag, name, prec, extra, False
            if none_ok:
                yield f"{name}/{prec}" + "".join(f"/{e}" for e in extras[-1]) + "/no_bias", name, prec, extras[-1], True


def run_pack(shift):
    lib = _lib.load()
    return {tag: digest(pack(lib, name, prec, shift, extra, no_bias)) for tag, name, prec, extra, no_bias in pack_cases()}


class NonFinite(Exception):
    pass


class Inputs:
    """the rays, steps, tables and rows every render case reads (3 rays: fewer rays than sample groups; mip: one 2 x 2 crop)"""

    def __init__(self, shift):
        from nerf_atlas_amd import ops
        dev = torch.device("cuda", 0)
        c2w = torch.tensor([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 4.0]]], device=dev)
        focal = 0.5 * 64 / math.tan(0.5 * 0.6911)
        self.rays = ops.raygen(c2w, focal, 64, (28, 28, 1, 3)).reshape(3, 6)
        self.rays_mip = ops.raygen(c2w, focal, 64, (28, 28, 2, 2))
        self.ts = (2.0 + torch.arange(T, dtype=torch.float32) / 8).to(dev)
        self.tables, self.tables2 = tensor(900, (8, 65536, 4), shift, dev), tensor(901, (8, 65536, 4), shift, dev)
        self.basis = tensor(904, (3, 128), shift - 6, dev)
        self.beta = torch.tensor([0.25], device=dev)
        self.shift, self.dev, self.ops = shift, dev, ops


def render(lib, I, name, prec, extra=(), empty=False):
    """one call of a render / rows entry on zero-filled outputs -> {output: sha256}"""
    fields, _, pack_sym, ws_fn, outs = RENDERS[name]
    dev = I.dev
    mip = "B" in fields
    rays = (I.rays_mip[:0] if empty else I.rays_mip) if mip else (I.rays[:0] if empty else I.rays)
    R = rays.numel() // 6
    N = T * R
    n_rl = extra[0] if name == "na_render_plain_plv_ls" else 0
    n_out = extra[0] if name == "na_mlp_hash_ls" else 65
    z = lambda *s: torch.zeros(s, device=dev, dtype=torch.float32)  # noqa: E731
    t = {"rays": rays, "ts": I.ts, "ts_ray": (I.ts[None, :] + torch.arange(R, device=dev)[:, None] / 64).contiguous(),
         "pts": I.ops.compute_pts(rays, I.ts) if name == "na_train_plain_view_ls" and R else None,
         "tables": I.tables, "tables2": I.tables2, "basis": I.basis, "beta": I.beta,
         "feat": tensor(902, (N, 65), I.shift, dev), "rl": tensor(903, (N, 3), I.shift, dev)[:, :n_rl].contiguous() if n_rl else None,
         "packed": pack(lib, pack_sym, prec, I.shift, extra if pack_sym in ("na_render_plain_plv_ls_pack", "na_mlp_hash_ls_pack") else ()),
         "alpha": z(T, R), "weights": z(T, R), "out": z(R, 3), "y": z(N, n_out), "planes": z(10, N, 256), "view_rows": z(N, 69),
         "density": z(N), "rgb_pre": z(N, 3)}
    wsb = getattr(lib, ws_fn)(T, R) if ws_fn else 0
    t["ws"] = torch.zeros(max(wsb, 1), device=dev, dtype=torch.uint8)
    v = {k: 0 if x is None else x.data_ptr() for k, x in t.items()}
    v.update(R=R, T=T, B=rays.shape[0], H=2, W=2, prec=PREC[prec], sig=SIG_THIN, bg=BG_WHITE, stream=_stream(), wsb=wsb, feat_ld=65,
             rl_ld=max(n_rl, 1), n_rl=n_rl, n_out=n_out, y_ld=n_out, mip_kind=1, min_deg=0, max_deg=16, t_end=float("nan"))
    rc = getattr(lib, name)(*[v[f] for f in fields])
    assert rc == 0, (name, prec, extra, rc, lib.na_last_error())
    torch.cuda.synchronize()
    for o in outs:
        if not bool(torch.isfinite(t[o]).all()):
            raise NonFinite(f"{name}/{prec}: {o}")
    return {o: digest(t[o]) for o in outs}


def render_cases():
    """(case id, entry, precision, extra, empty batch)"""
    for name, (_, precs, _, _, _) in RENDERS.items():
        for prec in precs:
            extras = [(n,) for n in HASH_N_OUT[prec]] if name == "na_mlp_hash_ls" else \
                [(0,), (3,)] if name == "na_render_plain_plv_ls" else [()]
            for extra in extras:
                yield f"{name}/{prec}" + "".join(f"/{e}" for e in extra), name, prec, extra, False
            yield f"{name}/{prec}/R0", name, prec, extras[-1], True


def run_render(shift, only=None):
    lib = _lib.load()
    I = Inputs(shift)
    return {tag: render(lib, I, name, prec, extra, empty) for tag, name, prec, extra, empty in render_cases()
            if only is None or tag in only}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sections", default="abi,pack,render")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    sections = a.sections.split(",")
    if "abi" in sections:
        rec["abi"] = run_abi()
    if "pack" in sections or "render" in sections:
        shift = 19
        while True:  # every recorded output is finite: halve the scale of the weights and inputs until it is
            try:
                first, second = run_render(shift), run_render(shift)
                break
            except NonFinite as e:
                print(f"shift {shift}: {e} is not finite, halving the scale", flush=True)
                shift += 1
                assert shift < 28
        rec["shift"] = shift
        rec["unstable"] = sorted(k for k in first if first[k] != second[k])
        rec["render"] = {k: v for k, v in first.items() if k not in rec["unstable"]}
        rec["pack"] = run_pack(shift)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"wrote {a.out}: " + ", ".join(f"{k} {len(v)}" for k, v in rec.items() if isinstance(v, (dict, list))), flush=True)


if __name__ == "__main__":
    main()
