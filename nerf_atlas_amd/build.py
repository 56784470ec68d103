"""Build libnerf_atlas_amd.so (HIP, gfx950) in-tree with hipcc.  No CPU fallback exists: if this library is
missing the package raises on first use.

    python -m nerf_atlas_amd.build [--force] [--jobs N] [--stress]

Environment:
  NA_BUILD_STRESS=1   also build libnerf_atlas_amd_lag3.so, the timing-stress variant of the layer-synchronous renderer the
                      determinism tests load (the four heaviest units compiled a second time).  Off for a user's build; CI --
                      __graft_entry__.build(), tests/test_isa_guard.py, tests/test_gpu_determinism.py -- asks for it explicitly.
  NA_HAZARD_SCAN=warn the build-time ISA scans (fp6-conversion operand overlap, MFMA / transcendental results read early by
                      inline asm, packed fp32 in render_ls_kernel) are text heuristics over the compiler's listing, conservative
                      by construction: under another ROCm version a false positive must not make the library unbuildable.
                      "warn" prints the finding to stderr and goes on; the default (and CI) is the hard gate.
  NA_EXTRA_HIPCC_FLAGS extra compiler flags (experiments).
"""
import argparse
import concurrent.futures as cf
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libnerf_atlas_amd.so")
ARCH = "gfx950"

# (source, extra flags, object suffix)
UNITS = [
    ("basic_ops.hip", [], ""),
    ("linear_f32.hip", [], ""),
    ("sh_head.hip", [], ""),
    ("ae_front.hip", [], ""),
    ("fourier_grad.hip", [], ""),
    ("composite_rayts.hip", [], ""),
    ("voxel.hip", [], ""),
    ("voxel_fine.hip", [], ""),
    ("voxel_sparse.hip", [], ""),
    ("dyn_voxel.hip", [], ""),
    ("dyn_voxel_render.hip", [], ""),
    ("spline_len.hip", [], ""),
    ("dyn_voxel_div.hip", [], ""),
    ("grid_ops.hip", [], ""),
    ("ssim.hip", [], ""),
    ("image_loss.hip", [], ""),
    ("optim.hip", [], ""),
    ("backward.hip", [], ""),
    ("train_gemm.hip", [], ""),
    ("train_bwd.hip", [], ""),
    ("train_fwd.hip", [], ""),
    ("march.hip", [], ""),
    ("mlp_fused.hip", [], ""),
    ("mlp_fwd_inst.hip", ["-DNA_PREC_INST=0"], "_bf16"),
    ("mlp_fwd_inst.hip", ["-DNA_PREC_INST=1"], "_bf16x3"),
    ("mlp_fwd_inst.hip", ["-DNA_PREC_INST=2"], "_f16"),
    ("render_fused.hip", ["-DNA_PREC_INST=0"], "_bf16"),
    ("render_fused.hip", ["-DNA_PREC_INST=1"], "_bf16x3"),
    # -fno-slp-vectorize: no compiler-formed packed-fp32 (v_pk_*_f32) arithmetic in the layer-synchronous kernel.  With it
    # the kernel's output is bit-reproducible under every timing variation tried (DESIGN 3b "reproducibility"); the speed
    # is the same.  The flag is a fence around a mechanism nobody has root-caused, so the BUILD checks what it is for: these
    # units are compiled with -save-temps and `check_isa` refuses a render_ls_kernel that contains packed fp32 arithmetic
    # (a toolchain bump that re-enables it under another pass name fails the build instead of the determinism tests).
    ("render_ls.hip", ["-DNA_PREC_INST=0", "-fno-slp-vectorize"], "_bf16", True),
    ("render_ls.hip", ["-DNA_PREC_INST=1", "-fno-slp-vectorize"], "_bf16x3", True),
    ("render_ls.hip", ["-DNA_PREC_INST=2", "-fno-slp-vectorize"], "_f16", True),
    ("render_ls.hip", ["-DNA_PREC_INST=3", "-fno-slp-vectorize"], "_f16x", True),
]
# Fourth field: True = the full ISA check (render_ls_kernel: no packed fp32) + the hazard scans; "hazard" (every other unit) =
# the hazard scans only -- fp6-conversion operand overlap, MFMA / transcendental results read early by inline asm
# (check_cvt_overlap, check_mfma_use, check_trans_use): what the compiler's hazard recogniser cannot see is checked for the
# whole library, not only where it was found.
UNITS = [u if len(u) == 4 else u + ("hazard",) for u in UNITS]
# The timing-stress build of the layer-synchronous renderer: sample group 1 runs THREE phases behind group 0 instead of one.
# This is the configuration in which the unexplained round-2 events (DESIGN 3b "reproducibility": 16 samples of one block off
# by 1e-3 in one run of 20 ... 10^3) were frequent enough to count -- 10^3 .. 10^5 differing elements per 200 runs without
# the two fences (compositing in front of the gathers, no SLP-formed packed fp32).  It is built next to the product library
# (same objects, the four render_ls units recompiled) so that tests/test_gpu_determinism.py exercises the fences on every
# GPU run instead of only when somebody remembers tools/ls_repeat.py variants.
STRESS_FLAGS = ["-DNA_LS_LAG_OVERRIDE=3"]
STRESS_UNITS = [(u[0], u[1] + STRESS_FLAGS, u[2] + "_lag3", u[3]) for u in UNITS if u[0] == "render_ls.hip"]
STRESS_LIB = os.path.join(HERE, "libnerf_atlas_amd_lag3.so")
ISA_FORBIDDEN = re.compile(r"^\s*(v_pk_(?:mul|add|fma)_f32)\b")
ISA_KERNEL = "render_ls_kernel"
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-value"] + os.environ.get("NA_EXTRA_HIPCC_FLAGS", "").split()


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build the HIP extension")
    return exe


def _headers_digest() -> str:
    """sha256 over every header a unit can include (csrc/*.h, csrc/*.inc, include/*.h): content, not mtime."""
    h = hashlib.sha256()
    for root in (CSRC, os.path.join(HERE, "..", "include")):
        for f in sorted(os.listdir(root)):
            if f.endswith((".h", ".inc")):
                h.update(f.encode())
                with open(os.path.join(root, f), "rb") as fh:
                    h.update(fh.read())
    return h.hexdigest()


def _unit_digest(unit, headers: str) -> str:
    src, extra, suffix, isa = unit
    h = hashlib.sha256(headers.encode())
    h.update(" ".join(FLAGS + extra + (["-save-temps=obj", "isa-check-v6", str(isa)] if isa else [])).encode())
    with open(os.path.join(CSRC, src), "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()


def _obj_path(unit):
    src, _, suffix = unit[:3]
    return os.path.join(OBJ, os.path.splitext(src)[0] + suffix + ".o")


def _isa_dir(unit):
    return os.path.splitext(_obj_path(unit))[0] + ".isa"


def isa_listings():
    """[(unit name, path of the device assembly listing)] of the units that are built with the ISA check"""
    out = []
    for u in UNITS:
        if u[3] is True and os.path.isdir(_isa_dir(u)):
            out += [(os.path.basename(_obj_path(u)), os.path.join(_isa_dir(u), f)) for f in sorted(os.listdir(_isa_dir(u)))
                    if f.endswith(".s") and "amdgcn" in f]
    return out


def hazard_listings():
    """[(unit name, listing path)] of EVERY unit of both libraries (the hazard scans run on all of them)"""
    out = []
    for u in UNITS + STRESS_UNITS:
        if u[3] and os.path.isdir(_isa_dir(u)):
            out += [(os.path.basename(_obj_path(u)), os.path.join(_isa_dir(u), f)) for f in sorted(os.listdir(_isa_dir(u)))
                    if f.endswith(".s") and "amdgcn" in f]
    return out


HEADLINE_SYMBOL = "_ZN2na2ls16render_ls_kernelILi3ELi0EEEvNS0_4ArgsE"  # render_ls_kernel<NA_PREC_F16X, MODEL 0>: bench.py's kernel
HEADLINE_PIN = os.path.join(CSRC, "ls_headline_isa.sha256")


def function_isa_digest(listing: str, symbol: str):
    """sha256 of the instructions of ONE function of a device listing (comments, directives and blank lines dropped, local labels
    kept, their per-function NUMBER dropped -- `.LBB11_3` and `.LBB13_3` are the same label of the same function once another
    instantiation is added to the unit): what tests/test_isa_guard.py pins for the headline kernel -- a change to a schedule file of another MODEL, to the
    packing code or to the C ABI must leave it untouched; a change that moves it is re-blessed on purpose
    (`python tools/check_isa.py --bless-headline`, then the determinism / stress tests on the GPU).  None if the symbol is absent."""
    h, inside, n = hashlib.sha256(), False, 0
    with open(listing) as fh:
        for line in fh:
            if not inside:
                inside = line.startswith(symbol + ":")
                continue
            if line.startswith(".Lfunc_end"):
                break
            t = line.split(";")[0].strip()
            if not t or (t.startswith(".") and not t.endswith(":")):
                continue
            h.update(re.sub(r"\.LBB\d+_", ".LBB_", t).encode() + b"\n")
            n += 1
    return (h.hexdigest(), n) if n else None


def check_isa(listing: str, kernel: str = ISA_KERNEL, forbidden=ISA_FORBIDDEN):
    """Scan a device assembly listing (-save-temps) for forbidden instructions inside every function whose symbol contains
    `kernel`.  Returns {symbol: [(line number, mnemonic)]} of the offenders and the list of functions scanned."""
    bad, seen, cur = {}, [], None
    with open(listing) as fh:
        for n, line in enumerate(fh, 1):
            if cur is None:
                m = re.match(r"^(\w+):", line)
                if m and kernel in m.group(1) and not m.group(1).startswith(".L"):
                    cur = m.group(1)
                    seen.append(cur)
                continue
            if line.startswith(".Lfunc_end") or line.lstrip().startswith(".end_amdhsa_kernel"):
                cur = None
                continue
            m = forbidden.match(line)
            if m:
                bad.setdefault(cur, []).append((n, m.group(1)))
    return bad, seen


_CVT_MNEMONIC = re.compile(r"^\s*(v_cvt_scalef32_(?:2xpk16|pk32)_(?:fp6|bf6)_\w+)\s+(.*)$")
_VREG = re.compile(r"^v\[(\d+):(\d+)\]$|^v(\d+)$")


def _vrange(op):
    """'v[4:9]' -> (4, 9), 'v7' -> (7, 7); anything else (an SGPR, a literal) -> None"""
    m = _VREG.match(op.strip())
    if not m:
        return None
    return (int(m.group(1)), int(m.group(2))) if m.group(1) is not None else (int(m.group(3)), int(m.group(3)))


def check_cvt_overlap(listing: str):
    """The multi-pass fp6 conversions -- v_cvt_scalef32_2xpk16_{fp6,bf6}_f32 vdst[6], src0[16], src1[16], scale and
    v_cvt_scalef32_pk32_{fp6,bf6}_{f16,bf16,f32} vdst[6], src[16|32], scale -- write their destination while they still read
    their operands (hardware probe tools/hw/cvt_fp6_overlap.hip: a scale in vdst[1] corrupts destination dwords 2..5, a
    destination on the LAST six registers of src1 dwords 3..5; a destination on the FIRST six registers of a source, or a scale
    in vdst[5], is fine), and the compiler (ROCm 7.2) does not mark the destination early-clobber -- its register allocator
    produced `v[0:5], v[32:47], v[48:63], v1` for the fp6 weight pack under another instruction scheduler.  Every instance in
    the whole listing (all functions) must therefore keep a VGPR scale outside the destination and the destination either
    disjoint from a source or on that source's first six registers.  The mnemonic is matched FIRST: an instance whose operand
    list does not parse is an offender, not a silent pass (a scalar or literal scale is accepted and cannot overlap).
    Returns [(line number, text)] of the offenders and the number scanned."""
    bad, n_seen = [], 0
    with open(listing) as fh:
        for n, line in enumerate(fh, 1):
            m = _CVT_MNEMONIC.match(line)
            if not m:
                continue
            n_seen += 1
            ops = [o.strip() for o in m.group(2).split(";")[0].split(",")]
            ops = [o for o in ops if o and not o.startswith(("op_sel", "clamp", "neg", "abs"))]
            want = 4 if "2xpk16" in m.group(1) else 3
            if len(ops) < want:
                bad.append((n, line.strip()))
                continue
            dst = _vrange(ops[0])
            srcs = [_vrange(o) for o in ops[1:want - 1]]
            scale = _vrange(ops[want - 1])  # None: SGPR / literal scale
            if dst is None or any(r is None for r in srcs):
                bad.append((n, line.strip()))
                continue
            d0, d1 = dst
            ok = True
            if scale is not None and d0 <= scale[0] <= d1:
                ok = False
            for s0, s1 in srcs:
                overlap = not (d1 < s0 or s1 < d0)
                if overlap and d0 != s0:
                    ok = False
            if not ok:
                bad.append((n, line.strip()))
    return bad, n_seen


# transcendental VALU ops (the "trans" unit): v_exp / v_log / v_rcp / v_rcp_iflag / v_rsq / v_sqrt / v_sin / v_cos, any float type
_TRANS = re.compile(r"^\s*(v_(?:exp|log|rcp|rcp_iflag|rsq|sqrt|sin|cos)(?:_legacy)?_(?:f16|f32|f64|bf16)(?:_e32|_e64|_sdwa|_dpp)?)\s+(.*)$")
_VALU = re.compile(r"^\s*(v_\w+)\s+(.*)$")
_VTOK = re.compile(r"v\[(\d+):(\d+)\]|\bv(\d+)\b")


def check_trans_use(listing: str):
    """CDNA3 / CDNA4 need ONE wait state between a transcendental VALU op and a non-transcendental VALU op that reads its result
    (the "trans forwarding hazard").  LLVM inserts it for the instructions it selects (GCNHazardRecognizer) but does not look at
    the operands of INLINE ASSEMBLY: an `asm("v_fma_mix_f32 ...")`, `asm("v_max3_f32 ...")` or asm fp6 conversion scheduled
    directly behind the op that produces its operand reads the register's OLD contents in 30-50 % of the lanes, depending on how
    the SIMD's waves interleave (hardware probe tools/hw/trans_use_hazard.hip).  Round 4: x::store_block<NA_ACT_SIN> of
    csrc/render_ls.hip (v_sin_f32 activations -> asm residual / fp6 conversions) made the mip renderer differ from run to run in
    the last bit of a few pixels.  Every trans op in the listing (all functions) must therefore NOT be followed immediately by a
    VALU instruction that names one of its destination registers (the destination itself counts: conservative).  Since the
    compiler keeps this invariant for its own instructions, an offender is an inline-asm consumer.
    Returns [(line number, trans text, next text)] and the number of trans ops scanned."""
    bad, n_seen = [], 0
    prev = None  # (line number, text, (d0, d1)) of a trans op whose next instruction has not been seen yet
    with open(listing) as fh:
        for n, line in enumerate(fh, 1):
            t = line.split(";")[0].rstrip()
            if not t.strip() or t.lstrip().startswith((".", "//")) or re.match(r"^[\w.$]+:", t):
                continue  # blank, directive, label (a fall-through into a label keeps the adjacency)
            if t.strip().split()[0] in ("s_branch", "s_endpgm", "s_setpc_b64"):
                prev = None
                continue
            if prev is not None:
                m = _VALU.match(t)
                if m and not _TRANS.match(t):
                    d0, d1 = prev[2]
                    for a, b, c in _VTOK.findall(m.group(2)):
                        lo, hi = (int(a), int(b)) if a else (int(c), int(c))
                        if not (hi < d0 or d1 < lo):
                            bad.append((prev[0], prev[1], t.strip()))
                            break
                prev = None
            m = _TRANS.match(t)
            if m:
                n_seen += 1
                dst = _vrange(m.group(2).split(",")[0])
                if dst is not None:
                    prev = (n, t.strip(), dst)
    return bad, n_seen


_MFMA = re.compile(r"^\s*(v_mfma_\w+)\s+(.*)$")


def _mfma_passes(mnemonic: str, text: str) -> int:
    """passes of an MFMA as far as the hazard rules need them (LLVM GCNHazardRecognizer, gfx950): 8 for the 32x32x16 f16 / bf16
    ops and for the f8f6f4 ops with both operands in a 6- or 4-bit format (cbsz, blgp >= 2), 4 for their 16x16 forms, 16 for
    everything else (conservative)."""
    small = "16x16" in mnemonic
    if re.search(r"_(?:f16|bf16)(?:_e64)?$", mnemonic) and re.search(r"32x32x16|16x16x32", mnemonic):
        return 4 if small else 8
    if "f8f6f4" in mnemonic:
        c, b = re.search(r"cbsz:(\d)", text), re.search(r"blgp:(\d)", text)
        narrow = c is not None and b is not None and int(c.group(1)) >= 2 and int(b.group(1)) >= 2
        return (4 if narrow else 8) if small else (8 if narrow else 16)
    return 16


def check_mfma_use(listing: str):
    """The matrix core writes its result several passes after issue and the hardware does NOT interlock a VALU instruction that
    reads it early: the compiler inserts s_nop for the instructions it selects (passes + 4 wait states measured in every listing
    of this library: 12 for the 8-pass ops) but is blind to INLINE ASSEMBLY, and a non-volatile asm statement may be scheduled
    across a barrier right behind the MFMA that produces its operand.  Round 4: the asm v_max3_f32 / v_fma_mix_f32 / fp6
    conversions of x::store_block on the accumulators of first.out ran 3 wait states behind the last MFMA in one instance of the
    mip renderer -> R / T planes built from a partly written accumulator, last-bit run-to-run differences in a few pixels
    (tools/mip_det_probe.py; the same class as tools/hw/trans_use_hazard.hip).  Every non-MFMA VALU instruction that names a
    register of an MFMA's destination must be at least passes + 4 wait states behind it (s_nop N counts N + 1, any other
    instruction 1); a later MFMA that overwrites the destination ends the window.  Returns [(line, mfma, consumer, waits)], n."""
    bad, n_seen = [], 0
    live = []  # [line, text, d0, d1, need, waits]
    with open(listing) as fh:
        for n, line in enumerate(fh, 1):
            t = line.split(";")[0].rstrip()
            if not t.strip() or t.lstrip().startswith((".", "//")):
                continue
            if re.match(r"^[\w.$]+:", t):
                if not t.startswith(".L"):
                    live = []  # a new function
                continue
            tt = t.strip()
            m = _MFMA.match(t)
            mn = tt.split()[0]
            if mn in ("s_branch", "s_endpgm", "s_setpc_b64"):
                live = []  # no fall-through: what follows is reached by jumps only (the compiler's own cross-block care)
                continue
            inc = 1
            if mn == "s_nop":
                try:
                    inc = int(tt.split()[1]) + 1
                except (IndexError, ValueError):
                    inc = 1
            if m:
                dst = _vrange(m.group(2).split(",")[0])
                if dst is not None:
                    live = [e for e in live if e[3] < dst[0] or dst[1] < e[2]]  # (accumulating into the same registers: SrcC rule)
                for e in live:
                    e[5] += 1
                n_seen += 1
                if dst is not None:
                    live.append([n, tt, dst[0], dst[1], _mfma_passes(m.group(1), t) + 4, 0])
                continue
            if mn.startswith("v_") and live:
                ops = tt.split(None, 1)[1] if " " in tt else ""
                for a, b, c in _VTOK.findall(ops):
                    lo, hi = (int(a), int(b)) if a else (int(c), int(c))
                    for e in live:
                        if not (hi < e[2] or e[3] < lo) and e[5] < e[4]:
                            bad.append((e[0], e[1], f"line {n}: {tt}", e[5]))
                            e[5] = 1 << 20  # report an MFMA once
            for e in live:
                e[5] += inc
            live = [e for e in live if e[5] < 24]
    return bad, n_seen


_WIDE_STORE = re.compile(r"^\s*(buffer_store_dwordx[34])\s+(v\[\d+:\d+\])\s*,\s*([^,]+),\s*(s\[\d+:\d+\])\s*,\s*(\S+)")


def check_store_data_overwrite(listing: str):
    """A buffer store of more than 8 bytes reads its data registers AFTER it has issued: a VALU instruction that overwrites one of
    them within the next two wait states can reach the register first.  LLVM's hazard recogniser (GCNHazardRecognizer::
    createsVALUHazard, gfx940+: 2 wait states) inserts the wait -- but only when the store's soffset field is NOT an SGPR; with
    an SGPR soffset it assumes the hardware has had time.  On gfx950 it has not (round 5: the g_x stores of csrc/train_bwd.hip,
    `buffer_store_dwordx4 v[182:185], v176, s[20:23], s33 offen` directly followed by `v_lshlrev_b32 v182, 16, v171`, wrote the
    shifted bf16 instead of the gradient in lanes 12-15 / 28-31 of some waves, 272 of 2 M elements, timing dependent; hardware
    probe tools/hw/store_soffset_hazard.hip).  Every 12- / 16-byte buffer store with an SGPR soffset in the listing (all
    functions) must therefore not be followed within two wait states (s_nop N counts N + 1) by a VALU instruction whose
    DESTINATION overlaps the store's data.  Returns [(line, store, writer, waits)] and the number of such stores scanned."""
    bad, n_seen = [], 0
    live = []  # [line, text, d0, d1, waits]
    with open(listing) as fh:
        for n, line in enumerate(fh, 1):
            t = line.split(";")[0].rstrip()
            if not t.strip() or t.lstrip().startswith((".", "//")):
                continue
            if re.match(r"^[\w.$]+:", t):
                if not t.startswith(".L"):
                    live = []
                continue
            tt = t.strip()
            mn = tt.split()[0]
            if mn in ("s_branch", "s_endpgm", "s_setpc_b64"):
                live = []
                continue
            if mn.startswith("v_") and live and not mn.startswith("v_cmp") and " " in tt:
                dst = _vrange(tt.split(None, 1)[1].split(",")[0])
                if dst is not None:
                    for e in live:
                        if not (dst[1] < e[2] or e[3] < dst[0]):
                            bad.append((e[0], e[1], f"line {n}: {tt}", e[4]))
            inc = 1
            if mn == "s_nop":
                try:
                    inc = int(tt.split()[1]) + 1
                except (IndexError, ValueError):
                    inc = 1
            for e in live:
                e[4] += inc
            live = [e for e in live if e[4] < 2]
            m = _WIDE_STORE.match(t)
            if m and re.match(r"^s\d+$", m.group(5)):
                n_seen += 1
                d = _vrange(m.group(2))
                live.append([n, tt, d[0], d[1], 0])
    return bad, n_seen


def _scan_failed(msg: str):
    """A build-time ISA scan found something: hard error, or a warning under NA_HAZARD_SCAN=warn (module docstring)."""
    if os.environ.get("NA_HAZARD_SCAN", "error").lower() == "warn":
        print("[nerf_atlas_amd] WARNING (NA_HAZARD_SCAN=warn, build continues): " + msg, file=sys.stderr)
        return
    raise RuntimeError(msg + "\n(NA_HAZARD_SCAN=warn turns the scans into warnings if this is a false positive of another toolchain.)")


def _compile(unit):
    src, extra, suffix, isa = unit
    obj = _obj_path(unit)
    if not isa:
        cmd = [hipcc()] + FLAGS + extra + ["-c", os.path.join(CSRC, src), "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}{suffix}:\n{r.stderr[-4000:]}")
        return obj
    # own directory: the intermediate files are named after the SOURCE, and three units share render_ls.hip
    d = _isa_dir(unit)
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    tmp = os.path.join(d, os.path.splitext(src)[0] + ".o")
    cmd = [hipcc()] + FLAGS + extra + ["-save-temps=obj", "-c", os.path.join(CSRC, src), "-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}{suffix}:\n{r.stderr[-4000:]}")
    for f in os.listdir(d):  # keep the device listing only
        if not (f.endswith(".s") and "amdgcn" in f) and f != os.path.basename(tmp):
            os.remove(os.path.join(d, f))
    listings = [os.path.join(d, f) for f in os.listdir(d) if f.endswith(".s")]
    if not listings:
        raise RuntimeError(f"{src}{suffix}: -save-temps produced no device listing, the ISA check cannot run")
    for lst in listings:
        cbad, _ = check_cvt_overlap(lst)
        if cbad:
            _scan_failed(f"{src}{suffix}: a multi-pass fp6 conversion whose destination overlaps its scale or the tail of a source "
                               f"({cbad[0][1]} at line {cbad[0][0]} of {lst}): the hardware then packs wrong values (tools/hw/cvt_fp6_overlap.hip). "
                               "Change the surrounding code until the register allocator separates them.")
        tbad, _ = check_trans_use(lst)
        if tbad:
            _scan_failed(f"{src}{suffix}: a transcendental result is read by the very next VALU instruction (line {tbad[0][0]} of {lst}: "
                               f"{tbad[0][1]} -> {tbad[0][2]}): an inline-asm consumer the hazard recogniser cannot see; the hardware "
                               "then reads the register's old contents (tools/hw/trans_use_hazard.hip).  Fence the asm's operands.")
        sbad, _ = check_store_data_overwrite(lst)
        if sbad:
            _scan_failed(f"{src}{suffix}: the data of a 16-byte buffer store with an SGPR soffset is overwritten {sbad[0][3]} wait states "
                               f"after issue (line {sbad[0][0]} of {lst}: {sbad[0][1][:70]} -> {sbad[0][2]}): the compiler inserts no wait "
                               "for that form and gfx950 needs one (tools/hw/store_soffset_hazard.hip).  Put the row step into the "
                               "vector offset (soffset 0) so that the hazard recogniser covers the store.")
        mbad, _ = check_mfma_use(lst)
        if mbad:
            _scan_failed(f"{src}{suffix}: an MFMA result is read {mbad[0][3]} wait states after issue (line {mbad[0][0]} of {lst}: "
                               f"{mbad[0][1][:60]} ... -> {mbad[0][2]}): an inline-asm consumer the hazard recogniser cannot see; the "
                               "hardware then reads a partly written accumulator (tools/hw/mfma_use_hazard.hip).  Fence the asm's operands.")
        if isa is not True:
            continue
        bad, seen = check_isa(lst)
        if not seen:
            _scan_failed(f"{src}{suffix}: no function named *{ISA_KERNEL}* in {lst}: the ISA check looked at nothing")
        if bad:
            first = "; ".join(f"{k}: {v[0][1]} at line {v[0][0]} (+{len(v) - 1} more)" for k, v in bad.items())
            _scan_failed(f"{src}{suffix}: packed fp32 arithmetic inside {ISA_KERNEL} ({first}).  The kernel is only known "
                               f"to be bit-reproducible without it (DESIGN 3b); see tools/check_isa.py")
    shutil.move(tmp, obj)
    return obj


def build(force: bool = False, jobs: int = 0, verbose: bool = True, stress=None) -> str:
    """Compile the units whose (source, headers, flags) digest changed since the object was built, then link.
    Up-to-date-ness is decided by content hashes recorded next to the objects (build/digests.json), never by mtime:
    a fresh checkout, an edited header and a changed flag all rebuild exactly what they touch.
    stress: also build the timing-stress library (None: NA_BUILD_STRESS=1 in the environment)."""
    if stress is None:
        stress = os.environ.get("NA_BUILD_STRESS", "0") == "1"
    units = [u for u in UNITS + (STRESS_UNITS if stress else []) if os.path.exists(os.path.join(CSRC, u[0]))]
    os.makedirs(OBJ, exist_ok=True)
    stamp = os.path.join(OBJ, "digests.json")
    try:
        with open(stamp) as fh:
            old = json.load(fh)
    except (OSError, ValueError):
        old = {}
    headers = _headers_digest()
    new = {os.path.basename(_obj_path(u)): _unit_digest(u, headers) for u in units}
    stale = [u for u in units if force or not os.path.exists(_obj_path(u))
             or old.get(os.path.basename(_obj_path(u))) != new[os.path.basename(_obj_path(u))]]
    lib_key = "__lib_stress__" if stress else "__lib__"
    if (not stale and os.path.exists(LIB) and (not stress or os.path.exists(STRESS_LIB))
            and old.get(lib_key) == hashlib.sha256("".join(sorted(new.values())).encode()).hexdigest()):
        return LIB
    jobs = jobs or min(max(len(stale), 1), os.cpu_count() or 4)
    if verbose:
        print(f"[nerf_atlas_amd] compiling {len(stale)} of {len(units)} units for {ARCH} with {jobs} jobs", file=sys.stderr)
    with cf.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(_compile, stale))
    twin = {(u[0], u[2][:-len("_lag3")]): u for u in units if u in STRESS_UNITS}
    targets = [(LIB, lambda u: u not in STRESS_UNITS)]
    if stress:
        targets.append((STRESS_LIB, lambda u: u in STRESS_UNITS or (u not in STRESS_UNITS and (u[0], u[2]) not in twin)))
    for lib, pick in targets:
        objs = [_obj_path(u) for u in units if pick(u)]
        cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    digest = hashlib.sha256("".join(sorted(v for k, v in new.items())).encode()).hexdigest()
    keep = {k: v for k, v in old.items() if k not in new and not k.startswith("__lib")}  # (objects of the variant not built now)
    new = dict(keep, **new)
    new[lib_key] = digest
    if stress:  # the product library was linked from the same objects
        new["__lib__"] = hashlib.sha256("".join(sorted(v for k, v in new.items() if not k.startswith("__lib") and "_lag3" not in k)).encode()).hexdigest()
    with open(stamp, "w") as fh:
        json.dump(new, fh, indent=1)
    return LIB


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("--jobs", type=int, default=0)
    ap.add_argument("--stress", action="store_true", help="also build the timing-stress library (NA_BUILD_STRESS=1)")
    a = ap.parse_args()
    print(build(a.force, a.jobs, stress=True if a.stress else None))
