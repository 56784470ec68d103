"""The hash, Fourier / positional, elevation / azimuth and mip encoders at their edges, against the fp64 references and the derived
per-element bounds of tests/encoder_ref.py: the standalone kernels (csrc/basic_ops.hip, csrc/backward.hip, csrc/fourier_grad.hip), the
view terms of csrc/sh_head.hip and the hash / Fourier prologues of the fused networks (na_mlp_forward, na_mlp_hash_ls,
na_mlp_fourier_ls).  Non-finite positions and directions must stay loud, and must stay in their own row.

Not reached from here: the encoder inside na_ae_front (its entry returns the networks' outputs, never the features) and ray_elaz_kernel
(csrc/ls_pack.h: it writes into the layer-synchronous renderers' workspace); both call the helpers tested below.

Worst error / bound measured on the MI355X when these tests were written (the tests print them):
  hash      set        forward  gradient (standalone, _rows)  jvp          fused (error / max |y|, bf16x3 unless named)
            lattice    .34      .04  .05                      .20          mlp_forward 1.5e-5 (bar 5e-5), mlp_hash_ls 1.4e-5 (5e-5),
            below      .31      .05  .04                      .17            f16x 3.8e-5 (1e-4): lattice + below + tiny_neg together
            tiny_neg   .24      .04  .04                      .18
            far        .23      .03  .04                      .13          mlp_forward 1.5e-5, mlp_hash_ls 1.2e-5, f16x 3.8e-5 (|x| < 2^15)
            bulk       .34      .05  .05                      .22
            (the forward ratios are the fp32 oracle's to the last digit: with -ffp-contract=off the kernel is the oracle's arithmetic)
  fourier   set        sin      cos      libm                 the bounds: 1.25 x 1.45e-7 = 1.81e-7, 1.25 x 5.81e-7 = 7.26e-7, 4u = 2.38e-7
            P          .67      .78      .22                  worst errors on the GPU: sin 1.45e-7, cos 5.8e-7 -- the restated
            L          .67      .78      .28                  sincos_cw's own figures (1 / 1.25 = .80): the cosine is NOT inside
            E          .80      .79      .16                  the 5e-7 csrc/common.h used to quote
            bulk sigma 16 / 32 against 2e-4: .02 / .04; positional (4 and 5 bands) against 4u: .25 / .24
            fused on P: mlp_forward bf16x3 1.2e-5 (bar 3e-4), mlp_fourier_ls f16x 3.4e-5 (2e-4)
  elev/azim set        elevation  azimuth                     (na_view_elaz = na_view_rows = na_plain_head_rows bit for bit;
            axes       .09        .12                          na_sh_view_terms' two columns: .41)
            poles      .14        .03
            seam       .20        .25
            zero       .09        .12                         (and the fp32 oracle's bits)
            norms      .41        .15
            bulk       .33        .30
  mip       cylinder H = 4 .31, H = 2 .25; cone H = 4 .25, H = 2 .24
With the fmaxf / fminf clamps elev_azim had before, test_elaz_non_finite_direction_stays_loud and test_sh_view_terms_features fail on
the MI355X: a NaN x component gave (elevation, azimuth) = (1.42e-3, 3 pi / 4), an Inf one azimuth pi where the reference has NaN.
"""
import math

import pytest
import torch

import oracle as O
import encoder_ref as ER

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from nerf_atlas_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def tabs():
    return ER.hash_tables().cuda()


def same_or_both_nan(a, b):
    """bit for bit, a NaN matching any NaN"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape:
        return False
    both = a.isnan() & b.isnan()
    return bool((both | (a.view(torch.int32) == b.view(torch.int32))).all())


# =============================================================================================================== hash
HASH_CASES = ER.HASH_SETS + tuple(f"n{n}" for n in ER.HASH_COUNTS)


@pytest.fixture(scope="module")
def hash_cases():
    """name -> (x [N, 3], fp64 reference): the five named sets and the prefixes of their concatenation"""
    t = ER.hash_tables()
    out = {name: (x, ER.hash_ref(x, t)) for name, x in ER.hash_sets().items()}
    head = ER.hash_concat()[:max(ER.HASH_COUNTS)].contiguous()
    ref = ER.hash_ref(head, t)
    for n in ER.HASH_COUNTS:
        out[f"n{n}"] = (head[:n].contiguous(), {k: v[:, :, :n] if k == "idx" else v[:n] for k, v in ref.items()})
    return out


@pytest.mark.parametrize("name", HASH_CASES)
def test_hash_forward(ops, tabs, hash_cases, name):
    """na_hash_encode: indices the oracle's bit for bit, features inside the bound, the raw columns a copy; on the lattice the level-0
    features ARE the addressed table row; na_hash_encode_rows (lead 0 / 1, with and without the input) is the cat of its parts."""
    x, ref = hash_cases[name]
    xg = x.cuda()
    feats, idx = ops.hash_encode(xg, tabs, include_input=True, want_indices=True)
    assert torch.equal(idx.cpu(), ref["idx"]), name
    assert ER.bits_equal(feats[:, :3], x)
    r = ER.worst_ratio(feats[:, 3:], ref["feat"], ER.hash_fwd_bound(ref))
    print(f"\n[hash forward {name}] N = {x.shape[0]}: worst error / bound {r:.3f}")
    assert r <= 1.0, (name, r)
    bare = ops.hash_encode(xg, tabs, include_input=False)
    assert ER.bits_equal(bare, feats[:, 3:])
    if name == "lattice":
        n = ER.N_LATTICE_FULL
        assert ER.bits_equal(bare[:n, :4], ER.hash_tables()[0][ref["idx"][0, 0, :n]])
        for l in range(8):     # the four zero rows sit on the lattice of every level
            assert ER.bits_equal(bare[-4:, 4 * l:4 * l + 4], ER.hash_tables()[l][ref["idx"][l, 0, -4:]])
    for lead in (0, 1):
        for inc in (True, False):
            rows = ops.hash_encode_rows(xg, tabs, include_input=inc, lead=lead)
            want = torch.cat([xg] * (lead + int(inc)) + [bare], dim=-1)
            assert ER.bits_equal(rows, want), (name, lead, inc)


@pytest.mark.parametrize("name", HASH_CASES)
def test_hash_position_gradient_and_jvp(ops, tabs, hash_cases, name):
    """na_hash_encode_backward_input, its _rows form (gradient rows read in place, lead 0 / 1) and na_hash_encode_jvp inside their
    bounds: on `lattice` and `below` the derivative is that of the cell floor selects (the reference differentiates that cell)."""
    x, ref = hash_cases[name]
    xg, N = x.cuda(), x.shape[0]
    worst = {}
    g = ER.hash_probe(N, 601, 35)
    want, bound = ER.hash_grad_ref(ref, g[:, 3:], g_in=g[:, :3])
    worst["grad"] = ER.worst_ratio(ops.hash_encode_backward_input(xg, tabs, g.cuda(), include_input=True), want, bound)
    want, bound = ER.hash_grad_ref(ref, g[:, 3:])
    worst["grad, no input"] = ER.worst_ratio(ops.hash_encode_backward_input(xg, tabs, g[:, 3:].contiguous().cuda(), include_input=False), want, bound)
    for lead in (0, 1):
        for inc in (True, False):
            k = lead + int(inc)
            gr = ER.hash_probe(N, 602 + 2 * lead + int(inc), 32 + 3 * k)
            want, bound = ER.hash_grad_ref(ref, gr[:, 3 * k:], g_in=gr[:, 3 * lead:3 * lead + 3] if inc else None, g_lead=gr[:, :3] if lead else None)
            got = ops.hash_encode_backward_input_rows(xg, tabs, gr.cuda(), inc, lead)
            worst[f"rows lead {lead} input {int(inc)}"] = ER.worst_ratio(got, want, bound)
    tan = ER.hash_probe(N, 610, 3)
    want, bound = ER.hash_jvp_ref(ref, tan)
    t = ops.hash_encode_jvp(xg, tabs, tan.cuda(), include_input=True)
    assert ER.bits_equal(t[:, :3], tan)
    worst["jvp"] = ER.worst_ratio(t[:, 3:], want, bound)
    assert ER.bits_equal(ops.hash_encode_jvp(xg, tabs, tan.cuda(), include_input=False), t[:, 3:])
    print(f"\n[hash derivatives {name}] N = {N}: worst error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (name, worst)


@pytest.mark.parametrize("bad,row,axis", [(NAN, 0, 0), (INF, 37, 1), (-INF, 64, 2)])
def test_hash_non_finite_position_stays_in_its_row(ops, tabs, bad, row, axis):
    """one NaN / +Inf / -Inf coordinate in a 65-point batch: that point's 32 features and its 32 jvp columns are NaN, its position
    gradient is NaN on the two other axes (the derivative along an axis does not contain that axis's own weight -- in the reference's
    autograd either --, so that one component is a finite number made of whatever cell the conversion of a NaN selects), every other
    row keeps the bits of the clean run, and no index leaves the table."""
    x = ER.hash_concat()[:65].clone()
    g, tan = ER.hash_probe(65, 620, 35).cuda(), ER.hash_probe(65, 621, 3).cuda()

    def run(p):
        f, idx = ops.hash_encode(p.cuda(), tabs, include_input=True, want_indices=True)
        return f.cpu(), idx.cpu(), ops.hash_encode_backward_input(p.cuda(), tabs, g, include_input=True).cpu(), \
            ops.hash_encode_jvp(p.cuda(), tabs, tan, include_input=True).cpu(), ops.hash_encode_rows(p.cuda(), tabs, True, 1).cpu()

    clean = run(x)
    assert all(bool(torch.isfinite(c).all()) for c in (clean[0], clean[2], clean[3], clean[4]))
    x[row, axis] = bad
    f, idx, gx, t, rows = run(x)
    assert int(idx.min()) >= 0 and int(idx.max()) <= 65535
    keep = torch.arange(65) != row
    assert bool(f[row, 3:].isnan().all()) and bool(t[row, 3:].isnan().all()) and bool(rows[row, 6:].isnan().all())
    others = [a for a in range(3) if a != axis]
    assert bool(gx[row, others].isnan().all()) and not bool(gx[row, axis].isinf())
    for got, was in zip((f, gx, t, rows), (clean[0], clean[2], clean[3], clean[4])):
        assert ER.bits_equal(got[keep], was[keep])
    assert torch.equal(idx[:, :, keep], clean[1][:, :, keep])
    assert ER.bits_equal(t[row, :3], tan[row].cpu())


# ============================================================================================================ Fourier
def _latent(N, L=3):
    """a column slice of a wider buffer: row pitch 7"""
    return ER.hash_probe(N, 630, 7).cuda()[:, 2:2 + L]


@pytest.mark.parametrize("name", ["P", "L", "E"])
def test_fourier_argument_exact(ops, name):
    """na_fourier_encode on argument-exact inputs: below the switch inside 1.25 x the restated sincos_cw's worst error, above it inside
    4u (libm); every F (16-byte and scalar path), D, power-of-two scale and N.  na_fourier_rows is cat([x, encode, latent]) bit for
    bit, and the backward that reads the saved features gives the bits of the one that recomputes them."""
    xs, bs = ER.fourier_sets()[name]
    worst = {"sin": 0.0, "cos": 0.0, "libm": 0.0}
    ws, wc = ER.cw_worst()
    counts = ER.N_VARIANTS + ((xs.shape[0],) if xs.shape[0] > max(ER.N_VARIANTS) else ())
    for N in counts:
        for D in ER.D_VARIANTS:
            for F in ER.F_VARIANTS:
                x, b = ER.fourier_variant(name, N, D, F)
                xg, bg = x.cuda(), b.cuda()
                for scale in ER.SCALES:
                    ref, bound = ER.fourier_ref(x, b, scale)
                    out = ops.fourier_encode(xg, bg, scale)
                    err = (out.cpu().double() - ref).abs()
                    assert bool(torch.isfinite(err).all())
                    ratio = err / bound
                    small = torch.cat([ER.fourier_m(x, b, scale).abs() <= ER.CW_SWITCH] * 2, dim=-1)
                    if bool(small[:, :F].any()):
                        worst["sin"] = max(worst["sin"], float(ratio[:, :F][small[:, :F]].max()))
                        worst["cos"] = max(worst["cos"], float(ratio[:, F:][small[:, F:]].max()))
                    if bool((~small).any()):
                        worst["libm"] = max(worst["libm"], float(ratio[~small].max()))
                    assert float(ratio.max()) <= 1.0, (name, N, D, F, scale, float(ratio.max()), float(err.max()))
                    lat = _latent(N)
                    rows = ops.fourier_rows(xg, bg, scale, latent=lat)
                    assert ER.bits_equal(rows, torch.cat([xg, out, lat], dim=-1)), (name, N, D, F, scale)
                    assert ER.bits_equal(ops.fourier_rows(xg, bg, scale), torch.cat([xg, out], dim=-1))
                    g = ER.hash_probe(N, 631, D + 2 * F + 3).cuda()
                    again = ops.fourier_encode_backward_input(xg, bg, scale, g, col0=D, lead=True)
                    saved = ops.fourier_encode_backward_input(xg, bg, scale, g, col0=D, lead=True, saved=rows, saved_col0=D)
                    assert ER.bits_equal(saved, again), (name, N, D, F, scale)
    print(f"\n[fourier {name}] worst error / bound: sin {worst['sin']:.3f}, cos {worst['cos']:.3f} (|m| <= 3e3: bounds "
          f"{ER.CW_MARGIN * ws:.3e} / {ER.CW_MARGIN * wc:.3e}), libm {worst['libm']:.3f} (bound {ER.LIBM:.3e})")


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_fourier_non_finite_coordinate_stays_in_its_row(ops, bad):
    for F in (128, 6):
        x, b = ER.fourier_variant("P", 33, 3, F)
        clean = ops.fourier_encode(x.cuda(), b.cuda()).cpu()
        x = x.clone()
        x[7, 1] = bad
        out = ops.fourier_encode(x.cuda(), b.cuda()).cpu()
        rows = ops.fourier_rows(x.cuda(), b.cuda()).cpu()
        keep = torch.arange(33) != 7
        assert bool(out[7].isnan().all()) and bool(rows[7, 3:].isnan().all())
        assert ER.bits_equal(out[keep], clean[keep]) and ER.bits_equal(rows[keep][:, 3:], clean[keep])


def test_fourier_bulk_and_positional(ops):
    """random inputs at the reference's sigma 16 / 32 against fp64 at the budget of the fp32 argument; the positional encoder (16-byte
    path: 4 bands, scalar path: 5) against fp64 sin / cos of the one fp32 product, 4u"""
    for sigma in (16, 32):
        x, b, ref = ER.fourier_bulk(sigma)
        r = ER.worst_ratio(ops.fourier_encode(x.cuda(), b.cuda()), ref, torch.full_like(ref, ER.BULK_TOL))
        print(f"\n[fourier bulk sigma {sigma}] worst error / 2e-4: {r:.3f}")
        assert r <= 1.0
    for NB in (4, 5):
        x, bands, ref = ER.positional_case(NB)
        for N in (1, 31, 257):
            r = ER.worst_ratio(ops.positional_encode(x[:N].contiguous().cuda(), bands.cuda()), ref[:N], torch.full_like(ref[:N], ER.LIBM))
            print(f"[positional {NB} bands, N = {N}] worst error / 4u: {r:.3f}")
            assert r <= 1.0, (NB, N, r)


# ================================================================================================ elevation / azimuth
def _elaz_users(ops, dirs, T=3, C=4):
    """elev / azim of every ray from na_view_elaz, na_view_rows and na_plain_head_rows (each [R, 2]) after checking the copies"""
    R = dirs.shape[0]
    dg = dirs.cuda()
    a = ops.view_elaz(dg)
    pts = ER.hash_probe(T * R, 640, 3).cuda().reshape(T, R, 3)
    rows = ops.view_rows(pts, dg)
    assert ER.bits_equal(rows[..., :3], pts)
    first = ER.hash_probe(T * R, 641, 1 + C).cuda()
    density, hr = ops.plain_head_rows(first, pts.reshape(T * R, 3), dg)
    assert ER.bits_equal(density, first[:, 0]) and ER.bits_equal(hr[:, :3], pts.reshape(-1, 3)) and ER.bits_equal(hr[:, 5:], first[:, 1:])
    b, c = rows[..., 3:], hr[:, 3:5].reshape(T, R, 2)
    for t in range(T):
        assert same_or_both_nan(b[t], a) and same_or_both_nan(c[t], a), t
    return a.cpu()


def test_elaz_edges(ops):
    """the axes, the tilted poles, both sides of the azimuth seam, the zero vector in its eight sign patterns, tiny and huge norms and
    a random bulk through na_view_elaz, na_view_rows and na_plain_head_rows: inside the bounds, the three bit-identical, the
    zero-direction rows the fp32 oracle's bit for bit"""
    dirs, zero = ER.elaz_dirs()
    ref, bound = ER.elaz_ref(dirs)
    got = _elaz_users(ops, dirs)
    ratio = (got.double() - ref).abs() / bound
    worst = {}
    start = 0
    for n, s in ER.elaz_sets().items():
        worst[n] = ratio[start:start + s.shape[0]].max(dim=0).values.tolist()
        start += s.shape[0]
    print("\n[elev / azim] worst error / bound (elevation, azimuth): " + ", ".join(f"{k} {v[0]:.3f} {v[1]:.3f}" for k, v in worst.items()))
    assert bool(torch.isfinite(ratio).all()) and float(ratio.max()) <= 1.0, worst
    assert ER.bits_equal(got[zero], O.dir_to_elev_azim(dirs[zero]))


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_elaz_non_finite_direction_stays_loud(ops, bad):
    """a NaN component makes the norm NaN: elevation and azimuth are NaN, as in the reference.  An Inf component is NaN after the
    normalisation (Inf / Inf) while the two others become 0: the reference's azimuth (Inf in x or y) or elevation (Inf in z) is NaN
    and the other one finite, and so is the kernels'.  Either way the ray is loud, and the other rays keep their bits."""
    dirs, _ = ER.elaz_dirs()
    clean = _elaz_users(ops, dirs)
    for comp in range(3):
        row = dirs.shape[0] - 5 - comp
        d = dirs.clone()
        d[row, comp] = bad
        got = _elaz_users(ops, d)
        want = O.dir_to_elev_azim(d)
        assert bool(want[row].isnan().any())
        assert torch.equal(got[row].isnan(), want[row].isnan()), (bad, comp, got[row], want[row])
        if math.isnan(bad):
            assert bool(got[row].isnan().all())
        fin = ~want[row].isnan()
        assert bool(((got[row][fin].double() - want[row][fin].double()).abs() <= 4 * ER.U * math.pi).all())
        keep = torch.arange(dirs.shape[0]) != row
        assert ER.bits_equal(got[keep], clean[keep])


def test_sh_view_terms_features(ops):
    """the features inside na_sh_view_terms read out through one-hot slices of w_init: [elev, azim] inside the elevation / azimuth
    bounds on the direction set, all 258 equal to na_view_elaz + na_fourier_encode (a one-hot row is an exact sum: f + zeros), and a
    NaN direction is NaN in its own ray only"""
    dirs, zero = ER.elaz_dirs()
    R, F, H = dirs.shape[0], 128, 128
    basis = ER.fourier_sets()["P"][1][:2].contiguous().cuda() * (1.0 / 16.0)
    zb, zw = torch.zeros(H, device="cuda"), torch.zeros(H, 2 + 2 * F, device="cuda")

    def features(d):
        cols = []
        for c0 in range(0, 2 + 2 * F, H):
            w = torch.zeros(H, 2 + 2 * F, device="cuda")
            n = min(H, 2 + 2 * F - c0)
            w[torch.arange(n), c0 + torch.arange(n)] = 1.0
            cols.append(ops.sh_view_terms(d.cuda(), basis, 1.0, w, zb, zw, zb, zw, zb)[0][:, :n])
        return torch.cat(cols, dim=-1)

    f = features(dirs)
    ea = ops.view_elaz(dirs.cuda())
    want = torch.cat([ea, ops.fourier_encode(ea, basis)], dim=-1)
    assert f.shape == (R, 258) and torch.equal(f, want)
    ref, bound = ER.elaz_ref(dirs)
    r = ER.worst_ratio(f[:, :2], ref, bound)
    print(f"\n[sh_view_terms] elevation / azimuth worst error / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(f[zero, :2].cpu(), O.dir_to_elev_azim(dirs[zero]))
    d = dirs.clone()
    d[40, 2] = NAN
    g = features(d).cpu()
    keep = torch.arange(R) != 40
    assert bool(g[40].isnan().all()) and torch.equal(g[keep], f.cpu()[keep])


# ================================================================================================================ mip
@pytest.mark.parametrize("kind", ["cylinder", "cone"])
@pytest.mark.parametrize("H", [4, 2])
def test_mip_argument_exact(ops, H, kind):
    """na_mip_encode on the argument-exact crops: T 1 / 2 / 5, an explicit closing edge and the one derived from ts (t_end = NaN), degrees
    0..16 (the 16-byte path) and 2..5 (18 features: the scalar path)"""
    worst = 0.0
    rays = ER.mip_crop(H)
    for T in ER.MIP_T:
        ts = ER.MIP_TS[:T].contiguous()
        for form in ("explicit", "nan"):
            end = ER.mip_t_end(T, form)
            for lo, hi in ((0, 16), (2, 5)):
                ref, bound = ER.mip_ref(rays, ts, kind, end, lo, hi)
                got = ops.mip_encode(rays.cuda(), ts.cuda(), kind, end if form == "explicit" else NAN, lo, hi)
                assert got.shape == ref.shape
                r = ER.worst_ratio(got, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (H, kind, T, form, lo, hi, r)
    print(f"\n[mip {kind} H = {H}] worst error / bound {worst:.3f}")


# ============================================================================================ fused hash / Fourier prologues
def _golden_net(case):
    from conftest import load_golden, golden_params
    g = load_golden(f"g6_mlp_{case}")
    p = golden_params(g, sigma=16.0)
    L = int(g["layers"])
    ws = [p["init.weight"]] + [p[f"layers.{i}.weight"] for i in range(L)] + [p["out.weight"]]
    bs = [p["init.bias"]] + [p[f"layers.{i}.bias"] for i in range(L)] + [p["out.bias"]]
    return g, p, [w.cuda() for w in ws], [b.cuda() for b in bs]


def _chain(ops, g, p, x, feats):
    """the network in exact fp32 (na_linear_f32) on [x | features from the standalone encoder]: tests/test_gpu_ops.py's _linear_chain"""
    act, L = str(g["act"]), int(g["layers"])
    init = torch.cat([x, feats], dim=-1)
    h = ops.linear_f32(init, p["init.weight"].cuda(), p["init.bias"].cuda())
    for i in range(L):
        skip = (i % 3 == 0) and i != L - 1
        h = ops.linear_f32(h, p[f"layers.{i}.weight"].cuda(), p[f"layers.{i}.bias"].cuda(), pre_act=act, x1=init if skip else None)
    return ops.linear_f32(h, p["out.weight"].cuda(), p["out.bias"].cuda(), pre_act=act)


def _hash_edge_sets():
    s = ER.hash_sets()
    return {"near": torch.cat([s["lattice"], s["below"], s["tiny_neg"]]), "far": s["far"]}


def _golden_tables(p):
    return torch.stack([p[f"enc.embs.{i}.weight"] for i in range(8)]).cuda()


def test_fused_prologues_of_mlp_forward(ops):
    """na_mlp_forward in bf16x3 with the hash prologue on lattice + below + tiny_neg and on far (each against its own max |y|: the far
    rows are 1e7 times larger) and with the Fourier prologue on set P, against the fp32 chain fed by the standalone encoder"""
    import test_gpu_ops as TGO
    g, p, ws, bs = _golden_net("first")
    desc = TGO._desc_for(ops, g, p)
    packed = ops.mlp_pack(desc, "bf16x3", ws, bs)
    tables = _golden_tables(p)
    for tag, x in _hash_edge_sets().items():
        xg = x.cuda()
        ref = _chain(ops, g, p, xg, ops.hash_encode(xg, tables))
        y = ops.mlp_forward(desc, "bf16x3", packed, xg, None, tables)
        err = float((y - ref).abs().max()) / float(ref.abs().max())
        print(f"\n[mlp_forward hash prologue, {tag}] N = {x.shape[0]}: error / max |y| {err:.2e} (bar 5e-5)")
        assert err <= 5e-5, (tag, err)
    g, p, ws, bs = _golden_net("sdfmlp")
    desc = TGO._desc_for(ops, g, p)
    packed = ops.mlp_pack(desc, "bf16x3", ws, bs)
    x, b = ER.fourier_sets()["P"]
    xg, bg = x.cuda(), b.cuda()
    ref = _chain(ops, g, p, xg, ops.fourier_encode(xg, bg))
    y = ops.mlp_forward(desc, "bf16x3", packed, xg, None, bg)
    err = float((y - ref).abs().max()) / float(ref.abs().max())
    print(f"[mlp_forward Fourier prologue, P] error / max |y| {err:.2e} (bar 3e-4)")
    assert err <= 3e-4, err


def _as_samples(x, T=4):
    """N points as explicit positions [T, R, 3] of R rays (the rays themselves are not read for the positions)"""
    R = x.shape[0] // T
    pts = x[:T * R].contiguous().cuda().reshape(T, R, 3)
    rays = torch.zeros(R, 6, device="cuda")
    rays[:, 5] = 1.0
    return pts, rays, torch.linspace(2.0, 6.0, T, device="cuda")


@pytest.mark.parametrize("prec,tol", [("bf16x3", 5e-5), ("f16x", 1e-4)])
def test_fused_hash_prologue_of_mlp_hash_ls(ops, prec, tol):
    """na_mlp_hash_ls with explicit positions on the hash edge sets, at the bars tests/test_gpu_models.py holds it to row by row (5e-5
    bf16x3, 1e-4 f16x, relative to max(1, |ref|)).  f16x carries the raw position in half-precision pieces: `far` is taken up to
    |x| < 2^15 there."""
    g, p, ws, bs = _golden_net("delta6")
    n_out = ws[-1].shape[0]
    packed = ops.mlp_hash_ls_pack(prec, ws, bs)
    tables = _golden_tables(p)
    for tag, x in _hash_edge_sets().items():
        if prec == "f16x":
            x = x[x.abs().max(dim=1).values < 2.0 ** 15]
        pts, rays, ts = _as_samples(x)
        flat = pts.reshape(-1, 3)
        ref = _chain(ops, g, p, flat, ops.hash_encode(flat, tables))
        y = ops.mlp_hash_ls(rays, ts, tables, packed, prec, n_out, pts=pts).reshape(-1, n_out)
        err = float((y - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        print(f"\n[mlp_hash_ls {prec}, {tag}] N = {flat.shape[0]}: error / max(1, |ref|) {err:.2e} (bar {tol:.0e})")
        assert err <= tol, (prec, tag, err)


def test_fused_fourier_prologue_of_mlp_fourier_ls(ops):
    """na_mlp_fourier_ls (f16x) with explicit positions on set P at the bar of tests/test_gpu_models.py (2e-4 relative to max(1, |ref|))"""
    g, p, ws, bs = _golden_net("sdfmlp")
    packed = ops.mlp_fourier_ls_pack("f16x", ws, bs)
    x, b = ER.fourier_sets()["P"]
    pts, rays, ts = _as_samples(x)
    flat = pts.reshape(-1, 3)
    ref = _chain(ops, g, p, flat, ops.fourier_encode(flat, b.cuda()))
    y = ops.mlp_fourier_ls(rays, ts, b.cuda(), packed, "f16x", pts=pts).reshape(-1, 65)
    err = float((y - ref).abs().max()) / max(1.0, float(ref.abs().max()))
    print(f"\n[mlp_fourier_ls f16x, P] N = {flat.shape[0]}: error / max(1, |ref|) {err:.2e} (bar 2e-4)")
    assert err <= 2e-4, err
