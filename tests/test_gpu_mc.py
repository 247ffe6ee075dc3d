"""tc_marching_cubes on the device against tests/mc_checker.py: every case of tests/mc_cases.py on both roads (numpy in: the host entry
point; torch device tensors in: the _device one), welded and unwelded, normals on and off.  Vertices, normals, faces and the two counts
are bit-EQUAL to the checker's: no tolerance, nothing left out of a comparison (normals are compared as bits; no NaN occurs: an unusable
corner switches its cubes off, and a NaN gradient gives (0, 0, 1)).
What each family of cases reaches: the 256 one-cube grids every row of the table; the lines the block (256) and scan-tile boundaries of the
per-voxel kernels and of the 16- and 8-lanes-per-cube emit kernels; the non-cubic, anisotropic, shifted grids every axis mix-up of the two
layouts; exact values the 1e-6 branch and vertices on corners; masks and non-finite values the usable rule; the far origins f32
cancellation in the sample coordinates; the 129^3 sphere the two-level scan (3 * 129^3 edge flags are more than 2048 scan tiles)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, synth
from tests import mc_cases as MC
from tests import mc_checker as K

pytestmark = pytest.mark.gpu
HEADER = "threecrate_hip_mc.h"
ROWS = ("mc_classify", "mc_edge_flags", "mc_scan", "mc_emit")
ROADS = ["numpy", "torch"]
MODES = [(weld, normals) for weld in (False, True) for normals in (True, False)]


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _to(a, road):
    return a if a is None or road == "numpy" else torch.from_numpy(a).to("cuda:0")


def _host(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a is not None and a.dtype == np.int32 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(ctx, case, road, weld, normals):
    out = ctx.marching_cubes(_to(case["values"], road), case["dims"], case["voxel_size"], case["origin"], case["iso_level"], normals, weld,
                             _to(case["valid"], road), case["layout"])
    assert all(a is None or isinstance(a, torch.Tensor) == (road == "torch") for a in out)
    return tuple(_host(a) for a in out)


def check(case, weld, normals):
    return K.marching_cubes(case["values"], case["dims"], case["voxel_size"], case["origin"], case["iso_level"], normals, weld, case["valid"], case["layout"])


def assert_equal(got, want, what):
    for key, g, w in zip(("vertices", "normals", "faces"), got, want):
        if w is None:
            assert g is None, (what, key)
            continue
        rows = np.nonzero((g != w).any(axis=1))[0] if g.shape == w.shape and g.size else None
        assert same_bits(g, w), (what, key, g.shape, w.shape, None if rows is None else (rows[:5], g[rows[:3]], w[rows[:3]]))


def all_modes(ctx, case, what, roads=ROADS):
    """every id covers both roads, welded and unwelded, normals on and off"""
    for weld, normals in MODES:
        want = check(case, weld, normals)
        for road in roads:
            assert_equal(run(ctx, case, road, weld, normals), want, (what, road, weld, normals))
    return want


def test_the_scan_tile_is_what_the_cases_assume():
    text = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "grid.hip")).read()
    items, block = (int(re.search(r"constexpr int %s = (\d+);" % k, text).group(1)) for k in ("kScanItems", "kScanBlock"))
    assert items * block == MC.SCAN_TILE


@pytest.mark.parametrize("first", [0, 64, 128, 192])
@pytest.mark.parametrize("layout", ["z_fastest", "x_fastest"])
def test_all_256_cases(ctx, layout, first):
    """a 2 x 2 x 2 grid per case, 64 cases per id, every one on both roads and in all four modes; the expected triangles are the table's
    row, the vertices its crossing edges"""
    rows, masks = K.G.table()
    for c in range(first, first + 64):
        want = all_modes(ctx, MC.one_cube(c, layout), (c, layout))
        assert len(want[2]) == len(rows[c]) and len(want[0]) == bin(masks[c]).count("1")


@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_every_case_equals_the_checker(ctx, name):
    case = MC.CASES[name]()
    want = all_modes(ctx, case, name)
    if name in ("mask_all", "all_above") or name.startswith("dims_with_1"):
        assert len(want[0]) == 0 and len(want[2]) == 0
    else:
        assert len(want[0]) and len(want[2])


@pytest.fixture(scope="module")
def sphere129():
    """the 129^3 sphere and the checker's answer in every mode, computed once"""
    case = MC.sphere(129)
    return case, {mode: check(case, *mode) for mode in MODES}


@pytest.mark.parametrize("road", ROADS)
def test_sphere_129_equals_the_checker_in_every_mode(ctx, sphere129, road):
    case, want = sphere129
    for weld, normals in MODES:
        assert_equal(run(ctx, case, road, weld, normals), want[(weld, normals)], (road, weld, normals))


def test_sphere_129_welded_is_a_closed_surface(sphere129):
    case, want = sphere129
    v, _, f = want[(True, True)]
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = np.minimum(e[:, 0], e[:, 1]) * len(v) + np.maximum(e[:, 0], e[:, 1])
    uniq, counts = np.unique(key, return_counts=True)
    assert (counts == 2).all()                                      # closed: every edge on two faces
    assert len(np.unique(e[:, 0] * len(v) + e[:, 1])) == len(e)     # ... once in each direction
    assert len(v) - len(uniq) + len(f) == 2                         # Euler characteristic of a sphere
    r = np.linalg.norm(v.astype(np.float64) - np.array([0.1, -0.2, 0.3]), axis=1)
    assert np.abs(r - 1.0).max() <= np.linalg.norm(np.array(case["voxel_size"], np.float64))


def test_repeatable(ctx):
    case = MC.CASES["sphere33"]()
    for road in ROADS:
        for weld, normals in MODES:
            a, b = run(ctx, case, road, weld, normals), run(ctx, case, road, weld, normals)
            assert_equal(a, b, (road, weld, normals))


def test_tsdf_volume_extract_mesh(ctx):
    """a 32^3 volume loaded with a plane's signed distance, weight 1 on one half: no vertex in the unobserved half; equal to the checker
    on the downloaded arrays"""
    n, vs = 32, 0.05
    vol = ctx.tsdf_volume(vs, 0.2, (n, n, n), origin=(-0.8, -0.8, 0.1))
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij")
    tsdf = np.clip(((0.3 * x + 0.2 * y + z) * np.float32(vs) - np.float32(1.1)) / np.float32(0.2), -1, 1).astype(np.float32)
    weight = (x < n // 2).astype(np.uint8)
    vol.load(tsdf, weight)
    t, w, _ = vol.voxels()
    assert same_bits(t, tsdf) and same_bits(w, weight)
    for weld, normals in MODES:
        want = K.marching_cubes(t, (n, n, n), (vol.voxel_size,) * 3, vol.origin, 0.0, normals, weld, w, "x_fastest")
        assert len(want[0])
        assert_equal(vol.extract_mesh(0.0, weld, normals), want, (weld, normals))
        got = vol.extract_mesh(0.0, weld, normals, device="cuda:0")
        assert isinstance(got[0], torch.Tensor)
        assert_equal(tuple(_host(a) for a in got), want, (weld, normals, "device"))
        assert want[0][:, 0].max() <= vol.origin[0] + (n // 2 - 1) * vol.voxel_size     # nothing in the unobserved half
    vol.close()


def test_launch_rows(ctx):
    """a Python call is two library calls (the counts, then the mesh): classify and scan twice, the edge flags twice with weld and never
    without, the emit stage once -- and not at all when the counts are zero"""
    def rows():
        r = {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("mc_")}
        return tuple(r.get(k, 0) for k in ROWS), set(r) - set(ROWS)

    ctx.profile_enable(True)
    try:
        for road in ROADS:
            for weld, normals in MODES:
                ctx.profile_reset()
                run(ctx, MC.CASES["random9_z_fastest"](), road, weld, normals)
                assert rows() == ((2, 2 if weld else 0, 2, 1), set()), (road, weld, normals)
                ctx.profile_reset()
                run(ctx, MC.CASES["all_above"](), road, weld, normals)
                assert rows() == ((1, 1 if weld else 0, 1, 0), set()), (road, weld, normals)
                ctx.profile_reset()
                run(ctx, MC.CASES["dims_with_1_a"](), road, weld, normals)
                assert rows() == ((0, 0, 0, 0), set()), (road, weld, normals)
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- the C ABI's calling convention, with a live context ----
def _call(ctx, fn, grid, values, valid, cfg, v, n, f, cap_v, cap_f):
    nv, nf = C.c_size_t(77), C.c_size_t(77)
    p = lambda a: None if a is None else a.ctypes.data
    rc = fn(ctx._h, None if grid is None else C.byref(grid), p(values), p(valid), None if cfg is None else C.byref(cfg), p(v), p(n), p(f), cap_v, cap_f,
            C.byref(nv), C.byref(nf))
    return rc, nv.value, nf.value


def _grid(dims=(9, 9, 9), vs=(0.1, 0.25, 0.5), org=(-3.0, 7.0, 0.5), layout=0):
    return _lib.McGridC((C.c_uint32 * 3)(*dims), (C.c_float * 3)(*vs), (C.c_float * 3)(*org), layout)


def test_count_call_capacities_and_invalid_arguments(ctx):
    L = _lib.load_companion(HEADER)
    case = MC.CASES["random9_z_fastest"]()
    values = case["values"]
    want = check(case, False, True)
    nv, nf = len(want[0]), len(want[2])
    cfg = _lib.McConfigC(0.0, _lib.TC_MC_NORMALS)
    fn = L.tc_marching_cubes
    assert _call(ctx, fn, _grid(), values, None, cfg, None, None, None, 0, 0) == (_lib.TC_OK, nv, nf)           # the count call
    v, n, f = np.full((nv, 3), 7, np.float32), np.full((nv, 3), 7, np.float32), np.full((nf, 3), 7, np.uint32)
    for cap_v, cap_f in ((nv - 1, nf), (nv, nf - 1), (0, 0)):
        assert _call(ctx, fn, _grid(), values, None, cfg, v, n, f, cap_v, cap_f) == (_lib.TC_INVALID_DATA, nv, nf)
        assert (v == 7).all() and (n == 7).all() and (f == 7).all()                                           # untouched
    assert _call(ctx, fn, _grid(), values, None, cfg, v, n, f, nv, nf) == (_lib.TC_OK, nv, nf)
    assert_equal((v, n, f), want, "exact capacity")
    inf, nan = float("inf"), float("nan")
    bad = [(None, values, cfg), (_grid(), None, cfg), (_grid(), values, None), (_grid(layout=2), values, cfg), (_grid(), values, _lib.McConfigC(0.0, 4)),
           (_grid(), values, _lib.McConfigC(nan, 1)), (_grid(), values, _lib.McConfigC(inf, 1)), (_grid(vs=(0.1, 0.0, 0.5)), values, cfg),
           (_grid(vs=(0.1, -0.25, 0.5)), values, cfg), (_grid(vs=(nan, 0.25, 0.5)), values, cfg), (_grid(vs=(0.1, 0.25, inf)), values, cfg),
           (_grid(org=(nan, 7.0, 0.5)), values, cfg), (_grid(org=(-3.0, -inf, 0.5)), values, cfg), (_grid(vs=(3e38, 0.25, 0.5), org=(3e38, 7.0, 0.5)), values, cfg)]
    for fn in (L.tc_marching_cubes, L.tc_marching_cubes_device):
        for grid, vals, c in bad:
            rc, a, b = _call(ctx, fn, grid, vals, None, c, None, None, None, 0, 0)
            assert rc == _lib.TC_INVALID_DATA and (a, b) == (77, 77), (grid, c)
            assert L is not None and ctx._L.tc_last_error_message(ctx._h).decode().startswith("marching_cubes:")
        assert _call(ctx, fn, _grid(dims=(1 << 10, 1 << 10, (1 << 8) + 1)), values, None, cfg, None, None, None, 0, 0)[0] == _lib.TC_UNSUPPORTED
        assert _call(ctx, fn, _grid(dims=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)), values, None, cfg, None, None, None, 0, 0)[0] == _lib.TC_UNSUPPORTED
        assert _call(ctx, fn, _grid(dims=(1, 9, 9)), values, None, cfg, None, None, None, 0, 0) == (_lib.TC_OK, 0, 0)
    nvp, nfp = C.c_size_t(0), C.c_size_t(0)
    assert fn(ctx._h, C.byref(_grid()), values.ctypes.data, None, C.byref(cfg), None, None, None, 0, 0, None, C.byref(nfp)) == _lib.TC_INVALID_DATA
    assert fn(ctx._h, C.byref(_grid()), values.ctypes.data, None, C.byref(cfg), None, None, None, 0, 0, C.byref(nvp), None) == _lib.TC_INVALID_DATA


def test_a_grid_of_zero_voxels_is_empty_on_both_roads(ctx):
    """a zero dim: no voxel, no address to pass; the answer is the header's for a dim below 2, and the checks are still made"""
    for road in ROADS:
        for dims in ((0, 9, 9), (9, 0, 9), (9, 9, 0), (0, 0, 0)):
            empty = np.zeros(0, np.float32)
            for weld, normals in MODES:
                v, n, f = ctx.marching_cubes(_to(empty, road), dims, normals=normals, weld=weld)
                assert len(v) == 0 and len(f) == 0 and (n is None) == (not normals) and isinstance(v, torch.Tensor) == (road == "torch")
            with pytest.raises(tc.InvalidData):
                ctx.marching_cubes(_to(empty, road), dims, voxel_size=(1.0, -1.0, 1.0))
    with pytest.raises(tc.InvalidData):
        threecrate.VolumetricGrid((2, 2), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))


def test_compat_follows_the_reference(ctx):
    v, vs, org = synth.sphere_volume(resolution=(17, 17, 17))
    grid = threecrate.VolumetricGrid((17, 17, 17), vs, org)
    grid.values[...] = v
    assert grid.get_value(1, 2, 3) == float(v[1, 2, 3]) and grid.get_value(17, 0, 0) is None
    with pytest.raises(tc.InvalidData):
        grid.set_value(0, 17, 0, 1.0)
    assert same_bits(grid.grid_to_world(1, 2, 3), np.asarray(org, np.float32) + np.asarray([1, 2, 3], np.float32) * np.asarray(vs, np.float32))
    want = K.marching_cubes(v, (17, 17, 17), vs, org, 0.0, True, False)
    mesh = threecrate.marching_cubes(grid, 0.0)
    assert same_bits(mesh.vertices(), want[0]) and same_bits(mesh.faces(), want[2]) and same_bits(mesh.normals, want[1])
    mesh = threecrate.MarchingCubes(threecrate.MarchingCubesConfig(iso_level=0.0, compute_normals=False)).extract_isosurface(grid)
    assert same_bits(mesh.vertices(), want[0]) and mesh.normals is None
    with pytest.raises(tc.AlgorithmError, match="No isosurface found at specified level"):
        threecrate.marching_cubes(grid, 100.0)
    with pytest.raises(tc.Unsupported):
        threecrate.MarchingCubes(threecrate.MarchingCubesConfig(smooth_mesh=True)).extract_isosurface(grid)


def test_mesh_feeds_smoothing_and_simplification(ctx):
    """depth of the chain: the welded mesh is what smooth_mesh and simplify_mesh_clustering take, without leaving the device"""
    case = MC.CASES["sphere33"]()
    v, _, f = ctx.marching_cubes(_to(case["values"], "torch"), case["dims"], case["voxel_size"], case["origin"], weld=True, normals=False)
    s = ctx.smooth_mesh(v, f, "laplacian", 2, 0.5)
    assert s.shape == v.shape and bool(torch.isfinite(s).all())
    out_v, out_f = ctx.simplify_mesh_clustering(s, f, 0.5)
    assert 0 < len(out_v) < len(v) and len(out_f)
