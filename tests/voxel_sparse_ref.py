"""Restatement of NeRFVoxel.sparsify (csrc/voxel_sparse.hip; `--voxel-sparsify`), the bounds the GPU tests hold the sparse
renderer to, and the rays, rows and tables they share.  Imported by tests/test_voxel_sparse_ref.py (CPU) and the GPU tests.

  d_thresh     the raw density whose softplus(d - 1) is the threshold: 1 + log(expm1(thresh)) in Python doubles, rounded once to fp32;
               -inf for thresh == 0
  table        keep = !(d < d_thresh) (a NaN density is kept); live[x,y,z] = any keep in the window x..x+2, y..y+2, z..z+2 clamped at
               S-1.  Compare and integer logic only: EXACT, the kernel's table is torch.equal to it.
  flags        a sample is live iff live[lower ids of voxel_ref.cells] != 0 or a coordinate is not finite (membership fixed in fp32
               like every voxel reference): exact as well
  sparse_ref   voxel_fine_ref.fine_ref with the density of dead samples set to -inf in front of the softplus (sigma = 0, alpha = 0,
               weight = 0) and their colours to 0 (they are not read); with a table of ones it IS fine_ref
  bounds       voxel_fine_ref.fine_bounds' on the dense lookup, with the relative error of sigma and the colour error of a dead sample 0:
               nothing is computed there.  (fp64's f = 1 - 0 + 1e-10 at a dead step against the kernel's untouched walk is inside the
               TINY terms of composite_ref.forward_bounds.)  Dead entries of alpha and weights are tested for == 0, not against a bound.
"""
import math

import torch

import composite_ref as CR
import voxel_fine_ref as F
import voxel_plv_ref as P
import voxel_ref as V
import voxel_sh_ref as H

GR = V.GRID_RADIUS
LANES = 16   # lanes per ray of the shipped sparse renderer: the edges of the compaction are multiples of it
MID = 0.64   # keeps ~5 % of voxel_ref.grid_values' densities (uniform in +-1): tables that are neither empty nor full at S = 4, 6, 16


# ------------------------------------------------------------------------------------------------------------ table
def d_thresh(thresh):
    thresh = float(thresh)
    if not math.isfinite(thresh) or thresh < 0:
        raise ValueError(thresh)
    if thresh == 0:
        return float("-inf")
    try:
        d = 1 + math.log(math.expm1(thresh))
    except OverflowError:
        d = 1 + thresh
    return float(torch.tensor(d, dtype=torch.float64).float())


def keep_of(den, thresh):
    """den [S,S,S,1] or [S,S,S] fp32 -> bool [S,S,S]"""
    assert den.dtype == torch.float32
    S = den.shape[0]
    return ~(den.reshape(S, S, S) < torch.tensor(d_thresh(thresh), dtype=torch.float32))


def table_from_keep(keep):
    """bool [S,S,S] -> uint8 [S,S,S]: the OR over the 3 x 3 x 3 window at and above each voxel, clamped at S-1"""
    S = keep.shape[0]
    live = torch.zeros_like(keep)
    for i in range(3):
        for j in range(3):
            for k in range(3):
                ix, iy, iz = ((torch.arange(S) + o).clamp(max=S - 1) for o in (i, j, k))
                live |= keep[ix][:, iy][:, :, iz]
    return live.to(torch.uint8)


def table_of(den, thresh):
    return table_from_keep(keep_of(den, thresh))


def flags_of(pts, live, grid_radius=GR):
    """pts [N,3] fp32, live uint8 [S,S,S] -> bool [N]"""
    S = live.shape[0]
    ids, _ = V.cells(pts, S, grid_radius)
    lo = ids[:, 0]
    return (live[lo[:, 0], lo[:, 1], lo[:, 2]] != 0) | ~torch.isfinite(pts).all(dim=-1)


def reads_kept(pts, keep, grid_radius=GR):
    """bool [N]: one of the 8 corners the lookup of pts reads is a kept voxel"""
    S = keep.shape[0]
    ids, _ = V.cells(pts, S, grid_radius)
    return keep.reshape(-1)[V.rows_of(ids, S)].any(dim=1)


def axis_spread(pts, S, grid_radius=GR):
    """[N,3] int64: upper id - lower id per axis (the premise of the 3-wide window: 0, 1 or 2)"""
    ids, _ = V.cells(pts, S, grid_radius)
    return ids[:, 7] - ids[:, 0]


# ------------------------------------------------------------------------------------------------------------ renderer
def sparse_ref(rays, ts_ray, den, rgb, live, head="rgb", order=-1, act="upshifted", bg="black", grid_radius=GR):
    """rays [R,6], ts_ray [R,M] fp32, the grids, live uint8 [S,S,S] -> fine_ref's dict (comp: out [R,3], alpha, weights [M,R], ...) with
    `flags` bool [M,R]; `density` is the DENSE lookup's (the bounds read it), the compositing saw -inf at dead samples"""
    R, M = ts_ray.shape
    pts = F.pts_rayts(rays, ts_ray)
    raw, mag, s, mag_s = F.lookup(head, order, pts.reshape(-1, 3), rays[:, 3:].contiguous(), den, rgb, grid_radius)
    flags = flags_of(pts.reshape(-1, 3), live, grid_radius).reshape(M, R)
    feat = F.colours(head, raw, s, act).reshape(M, R, 3)
    feat = torch.where(flags[..., None], feat, torch.zeros_like(feat))
    dense = raw[:, 0].reshape(M, R)
    d = torch.where(flags, dense, torch.full_like(dense, float("-inf")))
    comp = CR.composite_ref(d, feat, ts_ray.double(), rays[:, 3:].double(), "softplus", bg, None)
    return dict(comp=comp, density=dense, feat=feat, raw=raw, s=s, mag=mag, mag_s=mag_s, pts=pts, head=head, order=order, act=act, bg=bg,
                rand=None, flags=flags)


def sparse_bounds(f):
    """voxel_fine_ref.fine_bounds of a sparse_ref dict: the errors a dead sample does not have are 0 (module docstring)"""
    M, R = f["density"].shape
    raw, mag = f["raw"].detach(), f["mag"].detach()
    s, mag_s = (None, None) if f["s"] is None else (f["s"].detach(), f["mag_s"].detach())
    eps = F.eps_sigma(f["density"].detach(), F.raw_bound(f["head"], f["order"], mag)[:, 0].reshape(M, R))
    eps = torch.where(f["flags"], eps, torch.zeros_like(eps))
    err_c = F.colour_err(f["head"], f["order"], raw, mag, s, mag_s, f["act"]).reshape(M, R, 3)
    err_c = torch.where(f["flags"][..., None], err_c, torch.zeros_like(err_c))
    comp = {k: v.detach() for k, v in f["comp"].items()}
    return CR.forward_bounds(comp, eps, f["feat"].detach(), err_c=err_c, bg=f["bg"], rand=None)


# ------------------------------------------------------------------------------------------------------------ shared inputs
def grids(head, order, S):
    return V.grid_values(S) if head == "rgb" else P.grid_values(S, order) if head == "plv" else H.grid_values(S, order)


def mixed_rays(R, seed=8300):
    """rays through the grid from outside (voxel_ref.generic_rays); every 4th starts INSIDE the grid (origins in +-1, the heads' own
    direction set: un-normalised, the zero direction and an axis among them), every 5th points away from it and never meets it"""
    rays = V.generic_rays((R,), seed + R).clone()
    if R >= 4:
        inside = P.rays_of(H.directions(R, seed + 1), seed + 2)
        rays[::4] = inside[::4]
        rays[1::5, 3:] = -rays[1::5, 3:]
    return rays.contiguous()


def mixed_rows(R, M, seed=8310):
    """[R,M] increasing rows in 2 .. 6 (0 .. 2 for the rays that start inside), a duplicate step where M > 4"""
    rows = torch.sort(2.0 + 4.0 * torch.rand(R, M, generator=torch.Generator().manual_seed(seed + 31 * R + M)), dim=1).values
    if R >= 4:
        rows[::4] = (rows[::4] - 2.0) / 2.0
    if M > 4:
        rows[:, 3] = rows[:, 2]
    return rows.contiguous()


# the edge set: axis-parallel rays, one per (y, z) line of lower ids, so that the table of a line is its own.  A run (c, n) puts n samples
# where the lower id along x is c; `live` names the cells of the line that are live.  M = 65 = 4 chunks of 16 lanes and one step.
EDGE_S, EDGE_M = 6, 65
EDGE_LINES = (
    ("none", ((0, 30), (3, 35)), ()),
    ("all", ((0, 30), (3, 35)), (0, 3)),
    ("first only", ((0, 1), (2, 64)), (0,)),
    ("last only", ((1, 64), (4, 1)), (4,)),
    ("L-1", ((0, 20), (2, 15), (4, 30)), (2,)),
    ("L", ((0, 20), (2, 16), (4, 29)), (2,)),
    ("L+1", ((0, 20), (2, 17), (4, 28)), (2,)),
    ("run over 16", ((0, 10), (2, 11), (4, 44)), (2,)),
    ("runs over 16, 32 and to the end", ((0, 14), (1, 20), (3, 12), (5, 19)), (1, 5)),
    ("alternating", ((0, 5), (1, 5), (2, 5), (3, 5), (4, 5), (5, 40)), (0, 2, 4, 5)),
    ("first L", ((0, 16), (3, 49)), (0,)),
    ("last L", ((1, 49), (4, 16)), (4,)),
    ("second chunk only", ((0, 16), (2, 16), (4, 33)), (2,)),
)
# M = 31: the last chunk holds L - 1 steps, so the queue can hold more than L steps when it is drained (two rounds of phase B)
DRAIN_M = 31
DRAIN_LINES = (
    ("2 L - 2 at the drain", ((0, 1), (2, 30)), (2,)),
    ("L + 1 at the drain", ((0, 14), (2, 17)), (2,)),
    ("all", ((0, 15), (3, 16)), (0, 3)),
    ("none", ((0, 15), (3, 16)), ()),
    ("L at the drain", ((0, 1), (1, 15), (4, 15)), (0, 4)),
)


def edge_set(lines=EDGE_LINES, M=EDGE_M):
    """(rays [R,6], rows [R,M], live uint8 [6,6,6], expected flags bool [M,R]) of EDGE_LINES (or DRAIN_LINES, DRAIN_M)"""
    S = EDGE_S
    vl = GR * 2 / S
    at = lambda c: (c - S / 2 + 0.5) * vl + vl / 2   # the coordinate whose LOWER neighbour is the centre of cell c
    rays, rows, want = [], [], []
    live = torch.zeros(S, S, S, dtype=torch.uint8)
    for k, (_, runs, on) in enumerate(lines):
        yl, zl = k % S, k // S
        x, w = [], []
        for c, n in runs:
            x.append(at(c) + vl * (torch.linspace(-0.3, 0.3, n, dtype=torch.float64) if n > 1 else torch.zeros(1, dtype=torch.float64)))
            w += [c in on] * n
        x = torch.cat(x)
        assert x.numel() == M and bool((x[1:] > x[:-1]).all())
        rays.append([-3.0, at(yl), at(zl), 1.0, 0.0, 0.0])
        rows.append(x + 3.0)
        want.append(w)
        for c in on:
            live[c, yl, zl] = 1
    return (torch.tensor(rays, dtype=torch.float32), torch.stack(rows).float().contiguous(), live,
            torch.tensor(want, dtype=torch.bool).t().contiguous())


def run_stats(flags):
    """flags bool [M,R] -> per ray: live count [R], and whether a live run crosses a multiple of LANES (live at q - 1 and q)"""
    M = flags.shape[0]
    cross = torch.zeros(flags.shape[1], dtype=torch.bool)
    for q in range(LANES, M, LANES):
        cross |= flags[q - 1] & flags[q]
    return flags.sum(dim=0), cross
