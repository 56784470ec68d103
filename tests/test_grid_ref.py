"""The grid operators on the CPU: tests/grid_ref.py against the recorded reference (g24) and against torch itself, the conditions its
bounded cases rest on, and the host side of the feature -- flags, the set_per_run unsetting, --voxel-upsample's argument checks,
utils.randint, NeRFVoxel's state_dict at another resolution."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import grid_ref as G
from oracle.procedural import proc_uniform

G24 = ("462x5", "6x3", "8x1")


# ------------------------------------------------------------------------------------------------------------ total variation
@pytest.mark.parametrize("name", G24)
def test_tv_ref_reproduces_the_recorded_reference(name):
    g = load_golden(f"g24_grid_tv_{name}")
    shape, n = tuple(int(s) for s in g["shape"]), int(g["samples"])
    grid = torch.from_numpy(proc_uniform(shape, int(g["grid_seed"]), 1.0))
    idxs = g["idxs"]
    assert idxs.dtype == torch.int64 and idxs.shape == (n,)
    r64 = G.tv_ref(grid.double(), idxs)
    rel = abs(float(r64["value"]) - float(g["value64"])) / float(g["value64"])
    grel = float((r64["grad"] - g["grad64"]).abs().max() / g["grad64"].abs().max())
    print(f"[g24 {name}] fp64 value {rel:.1e}, gradient {grel:.1e} relative")
    assert rel <= 1e-12 and grel <= 1e-12
    r32 = G.tv_ref(grid, idxs)
    err, bound = abs(float(g["value"]) - float(r32["value"])), G.value_bound(r32["value"], n, shape[3], False)
    print(f"[g24 {name}] the reference's fp32 value is {err:.2e} off, bound {bound:.2e}")
    assert err <= bound


def torch_tv(grid, idxs):
    """the operator as torch operators (what autograd differentiates)"""
    (x, y, z), (ax, ay, az) = G.decode(idxs, grid.shape)
    e = grid[x, y, z]
    dx, dy, dz = e - grid[ax, y, z], e - grid[x, ay, z], e - grid[x, y, az]
    return (dx.square() + dy.square() + dz.square()).clamp(min=1e-10).sqrt().mean()


def test_tv_ref_gradient_is_torch_autograd_including_the_clamp_and_non_finite_voxels():
    grid = G.tv_grid("462x5").double().clone()
    grid[1, 2, 0], grid[3, 5, 1, 2] = float("nan"), float("inf")
    grid[2:4, 1:3] = 0.5                                        # a constant patch: q = 0 at (2, 1, 0), below the clamp
    idxs = torch.arange(4 * 6 * 2, dtype=torch.int64).repeat(2)
    p = grid.clone().requires_grad_(True)
    (3.0 * torch_tv(p, idxs)).backward()
    ref = G.tv_ref(grid, idxs, g=3.0, clean=False)
    assert torch.equal(torch.isnan(ref["grad"]), torch.isnan(p.grad)) and 0 < int(torch.isnan(p.grad).sum()) < p.numel() // 2
    ok = ~torch.isnan(p.grad)
    assert float((ref["grad"][ok] - p.grad[ok]).abs().max()) <= 1e-13
    assert not bool(torch.isfinite(ref["value"]))


def test_every_bounded_gpu_case_is_clear_of_the_clamp():
    """tv_ref(clean=True) asserts q == 0 or q > 1e-8 for every element: run it on every input tests/test_gpu_grid.py bounds"""
    for name in G.TV_GRIDS:
        for n in G.TV_COUNTS:
            r = G.tv_reference(name, n)
            assert bool(torch.isfinite(r["grad"]).all()) and float(r["value"]) > 0.1
    for _, grid, idxs in G.duplicate_cases():
        G.tv_ref(grid, idxs)


def test_decode_takes_x_from_the_fastest_digit():
    (x, y, z), (ax, ay, az) = G.decode(torch.tensor([0, 1, 3, 4, 23, 47]), (4, 6, 2, 5))
    assert x.tolist() == [0, 1, 3, 0, 3, 3] and y.tolist() == [0, 0, 0, 1, 5, 5] and z.tolist() == [0, 0, 0, 0, 0, 1]
    assert ax.tolist() == [1, 2, 2, 1, 2, 2] and ay.tolist() == [1, 1, 1, 2, 4, 4] and az.tolist() == [1, 1, 1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------------------ upsample
@pytest.mark.parametrize("S,R,C", G.UP_CASES)
def test_upsample_chain_against_torch(S, R, C):
    """the restated fp32 coordinate chain with the fp64 blend: within the blend bound of torch's own fp32 F.interpolate, and within the
    whole bound of the float64 reference"""
    grid, ref, bound = G.up_reference(S, R, C)
    val, mag, _ = G.upsample_chain(grid, R)
    assert G.worst_ratio(G.interpolate(grid, R), val, G.BLEND_C * G.U * mag) <= 1.0
    assert G.worst_ratio(val, ref, bound) <= 1.0


def test_upsample_exact_cases_on_the_cpu():
    grid = torch.from_numpy(np.rint(proc_uniform((4, 4, 4, 3), 5410, 8.0)).astype(np.float32))
    assert torch.equal(G.interpolate(grid, 4), grid)
    assert torch.equal(G.upsample_chain(grid, 4)[0], grid.double())
    assert torch.equal(G.interpolate(grid, 8).double(), G.interpolate(grid.double(), 8))
    assert torch.equal(G.upsample_chain(grid, 8)[0], G.interpolate(grid.double(), 8))


# ------------------------------------------------------------------------------------------------------------ host side
def test_the_flags_parse():
    from nerf_atlas_amd import train as T
    a = T.args_from_argv(["--model", "voxel"])
    assert (a.voxel_tv_sigma, a.voxel_tv_rgb, a.voxel_tv_bezier, a.voxel_tv_rigidity, a.voxel_upsample) == (0.0, 0.0, 0.0, 0.0, [])
    a = T.args_from_argv(["--model", "voxel", "--refl-kind", "pos", "--voxel-tv-sigma", "1e-3", "--voxel-tv-rgb", "1e-4", "--voxel-tv-bezier",
                          "0.5", "--voxel-tv-rigidity", "0.25", "--voxel-upsample", "2000:128", "4000:256"])
    assert (a.voxel_tv_sigma, a.voxel_tv_rgb, a.voxel_tv_bezier, a.voxel_tv_rigidity) == (1e-3, 1e-4, 0.5, 0.25)
    assert a.voxel_upsample == [(2000, 128), (4000, 256)]
    assert T.make_args(voxel_upsample=[(5, 8)]).voxel_upsample == [(5, 8)] and T.DEFAULTS["voxel_upsample"] == []


def test_set_per_run_unsets_what_the_model_has_no_grid_for(capsys):
    from nerf_atlas_amd import nerf, train as T
    vox = nerf.NeRFVoxel(resolution=4)
    a = T.make_args(model="voxel", voxel_tv_sigma=0.1, voxel_tv_rgb=0.2, voxel_tv_bezier=0.3, voxel_tv_rigidity=0.4)
    T.unset_voxel_tv(a, vox)
    assert capsys.readouterr().out == "[warn]: model does not have bezier control points or rigidity for static scene\n"
    assert (a.voxel_tv_sigma, a.voxel_tv_rgb, a.voxel_tv_bezier, a.voxel_tv_rigidity) == (0.1, 0.2, 0, 0)
    T.unset_voxel_tv(a, vox)
    assert capsys.readouterr().out == ""
    for k in ("voxel_tv_sigma", "voxel_tv_rgb", "voxel_tv_bezier", "voxel_tv_rigidity"):
        a = T.make_args(**{k: 0.5})
        T.unset_voxel_tv(a, torch.nn.Linear(1, 1))
        assert capsys.readouterr().out == "[warn]: model is not voxel, unsetting total variation\n"
        assert (a.voxel_tv_sigma, a.voxel_tv_rgb, a.voxel_tv_bezier, a.voxel_tv_rigidity) == (0, 0, 0, 0)
    T.unset_voxel_tv(T.make_args(), torch.nn.Linear(1, 1))
    assert capsys.readouterr().out == ""


def test_voxel_upsample_argument_errors():
    from nerf_atlas_amd import nerf, train as T
    for bad, why in ((["6:7"], "even"), (["6:8", "6:16"], "increasing"), (["8:8", "6:16"], "increasing"), (["6"], "ITER:RESO"),
                     (["a:8"], "ITER:RESO"), (["6:0"], "even")):
        with pytest.raises(ValueError, match=why):
            T.args_from_argv(["--model", "voxel", "--voxel-upsample"] + bad)

    class NotVoxel(torch.nn.Linear):
        nerf = property(lambda self: self)
    for kw in (dict(voxel_upsample=[(1, 8)]), dict(voxel_tv_sigma=0.1)):
        with pytest.raises(ValueError, match="--model voxel"):
            T.train(NotVoxel(1, 1), None, None, None, T.make_args(epochs=2, **kw))
    with pytest.raises(ValueError, match="even"):
        nerf.NeRFVoxel(resolution=4).upsample(7)


def test_randint_replays_the_cpu_stream():
    from nerf_atlas_amd import utils
    prev = utils.random_source
    try:
        utils.set_random_source(utils.ReferenceStreamRandom())
        torch.manual_seed(7)
        a, after_a = utils.randint(0, 4 * 6 * 2, (257,), "cpu"), torch.rand(3)
        torch.manual_seed(7)
        b, after_b = torch.randint(0, 4 * 6 * 2, (257,)), torch.rand(3)
        assert a.dtype == torch.int64 and torch.equal(a, b) and torch.equal(after_a, after_b)
    finally:
        utils.set_random_source(prev)
    assert isinstance(utils.random_source, type(prev))
    v = utils.randint(0, 5, (64,), "cpu")
    assert v.dtype == torch.int64 and 0 <= int(v.min()) and int(v.max()) < 5


def test_a_state_dict_decides_the_resolution():
    from nerf_atlas_amd import nerf
    big = nerf.NeRFVoxel(resolution=8, grid_radius=1.3)
    sd = {k: v.clone() for k, v in big.state_dict().items()}
    m = nerf.NeRFVoxel(resolution=4, grid_radius=1.3)
    m.load_state_dict(sd, strict=True)
    assert m.resolution == 8 and m.voxel_len == 1.3 * 2 / 8
    assert torch.equal(m.densities, big.densities) and torch.equal(m.rgb, big.rgb) and isinstance(m.rgb, torch.nn.Parameter)
    assert m.densities.requires_grad and m.rgb.requires_grad
    small = nerf.NeRFVoxel(resolution=8)
    small.load_state_dict(nerf.NeRFVoxel(resolution=2).state_dict())
    assert small.resolution == 2 and tuple(small.rgb.shape) == (2, 2, 2, 3)
    for den, rgb in ((torch.zeros(3, 3, 3, 1), torch.zeros(3, 3, 3, 3)), (torch.zeros(4, 6, 4, 1), torch.zeros(4, 6, 4, 3)),
                     (torch.zeros(8, 8, 8, 1), torch.zeros(6, 6, 6, 3))):
        fresh = nerf.NeRFVoxel(resolution=4)
        with pytest.raises(ValueError, match="cubic"):
            fresh.load_state_dict({"densities": den, "rgb": rgb})
        assert fresh.resolution == 4 and tuple(fresh.densities.shape) == (4, 4, 4, 1)
    with pytest.raises(RuntimeError, match="size mismatch"):    # another channel count stays torch's own refusal
        nerf.NeRFVoxel(resolution=4).load_state_dict({"densities": torch.zeros(8, 8, 8, 1), "rgb": torch.zeros(8, 8, 8, 5)})


def test_upsample_and_total_variation_refuse_a_cpu_model():
    from nerf_atlas_amd import nerf
    m = nerf.NeRFVoxel(resolution=4)
    with pytest.raises(ValueError, match="GPU"):
        m.upsample(8)
    assert m.resolution == 4 and tuple(m.rgb.shape) == (4, 4, 4, 3)
    with pytest.raises(ValueError):
        nerf.total_variation(m.densities, samples=8)
