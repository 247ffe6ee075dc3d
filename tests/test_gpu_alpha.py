"""Alpha-shape reconstruction on the device (include/threecrate_hip_alpha.h, csrc/alpha.hip) against the numpy restatement of its contract
(tests/alpha_checker.py): for every case of tests/alpha_cases.py, in both modes and through both the host and the _device road, the faces
and the stats EQUAL the checker's: the same triples in the same order, the same counts.  No tolerance anywhere: the outputs are indices."""
import numpy as np
import pytest

from tests import alpha_cases as AC
from tests import alpha_checker as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import threecrate_amd as tc
    c = tc.GpuContext(0)
    yield c
    c.close()


def _run(ctx, road, points, alpha, mode, cap):
    import torch
    p = points if road == "host" else torch.from_numpy(points).to("cuda:0")
    faces, stats = ctx.alpha_shape(p, alpha, mode=mode, max_triangles=cap, return_stats=True)
    if road == "device":
        assert isinstance(faces, torch.Tensor) and faces.is_cuda
        faces = faces.cpu().numpy().view(np.uint32)
    return faces, stats


@pytest.mark.parametrize("road", ["host", "device"])
@pytest.mark.parametrize("name", list(AC.CASES))
def test_faces_and_stats_equal_the_checker(ctx, name, road):
    import threecrate_amd as tc
    points, alpha, cap = AC.CASES[name]
    for mode in AC.MODES:
        want = AC.expected(name, mode)
        if isinstance(want, K.AlphaError):
            with pytest.raises(tc.AlgorithmError, match=want.message):
                _run(ctx, road, points, alpha, mode, cap)
            continue
        faces, stats = _run(ctx, road, points, alpha, mode, cap)
        assert faces.dtype == np.uint32 and faces.shape == want["faces"].shape, (mode, faces.shape, want["faces"].shape)
        assert stats == {"candidates": want["candidates"], "boundary_candidates": want["boundary_candidates"], "faces": want["n_faces"],
                         "capped": want["capped"]}, mode
        assert np.array_equal(faces, want["faces"]), mode


def test_no_cap_equals_a_cap_above_the_total(ctx):
    a, sa = _run(ctx, "host", *AC.CASES["sphere300_uncapped"][:2], "full", 0)
    b, sb = _run(ctx, "host", *AC.CASES["sphere300_cap_above"][:2], "full", AC.CASES["sphere300_cap_above"][2])
    assert sa == sb and sa["capped"] == 0 and np.array_equal(a, b)
    c, sc = _run(ctx, "host", *AC.CASES["sphere300_uncapped"][:2], "full", sa["candidates"])        # a cap AT the total cuts nothing off
    assert sc == sa and np.array_equal(a, c)
    d, sd = _run(ctx, "host", *AC.CASES["sphere300_uncapped"][:2], "full", sa["candidates"] - 1)
    assert sd["capped"] == 1 and sd["candidates"] == sa["candidates"] - 1


def test_a_cloud_without_candidates_is_an_algorithm_error_and_writes_nothing(ctx):
    import ctypes as C
    import threecrate_amd as tc
    from threecrate_amd import _lib
    with pytest.raises(tc.AlgorithmError, match="No candidate triangles generated"):
        ctx.alpha_shape(AC.NO_CANDIDATE, 1.0)
    with pytest.raises(tc.AlgorithmError, match="No candidate triangles generated"):
        ctx.alpha_shape(AC.CASES["three_points"][0], 0.9)           # the KAT with a smaller alpha
    L = _lib.load_companion("threecrate_hip_alpha.h")
    cfg, st = _lib.AlphaConfigC(1.0, 0, 1e-8, 50000), _lib.AlphaStatsC(7, 7, 7, 7)
    out = np.full((4, 3), 7, np.uint32)
    rc = L.tc_alpha_shape(ctx._h, AC.NO_CANDIDATE.ctypes.data, len(AC.NO_CANDIDATE), C.byref(cfg), out.ctypes.data, 4, C.byref(st))
    assert rc == _lib.TC_ALGORITHM and (out == 7).all() and (st.candidates, st.boundary_candidates, st.faces, st.capped) == (7, 7, 7, 7)


def test_invalid_input_is_refused(ctx):
    import threecrate_amd as tc
    p = AC.CASES["sphere300_0.35"][0]
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(tc.InvalidData, match="alpha"):
            ctx.alpha_shape(p, alpha)
    with pytest.raises(tc.InvalidData, match="min_triangle_area"):
        ctx.alpha_shape(p, 0.35, min_triangle_area=-1.0)
    bad = p.copy()
    bad[17, 1] = np.nan
    with pytest.raises(tc.InvalidData, match="not finite"):
        ctx.alpha_shape(bad, 0.35)
    with pytest.raises(tc.InvalidData, match="Need at least 3 points"):
        ctx.alpha_shape(p[:2], 0.35)
    with pytest.raises(tc.InvalidData, match="Point cloud is empty"):
        ctx.alpha_shape(p[:0], 0.35)


def test_the_result_feeds_the_mesh_units(ctx):
    """alpha_shape -> mesh_adjacency / smooth_mesh accept the faces over the input points"""
    points, alpha, _ = AC.CASES["sphere300_0.35"]
    faces = ctx.alpha_shape(points, alpha, max_triangles=0)
    offsets, neighbors = ctx.mesh_adjacency(len(points), faces)
    used = np.unique(faces)
    assert offsets[-1] == len(neighbors) and (np.diff(offsets)[used] >= 2).all()
    smooth = ctx.smooth_mesh(points, faces, "laplacian", 2)
    assert smooth.shape == points.shape and np.isfinite(smooth).all() and not np.array_equal(smooth, points)


def test_the_compat_call_gives_the_reference_mesh(ctx):
    import threecrate_amd.compat as threecrate
    points = AC.CASES["sphere700_reference_cap"][0]
    mesh = threecrate.alpha_shape_reconstruct(threecrate.PointCloud.from_numpy(points), 0.6)
    want = AC.expected("sphere700_reference_cap", "boundary")
    assert mesh.vertex_count == 700 and np.array_equal(mesh.vertices(), points) and np.array_equal(mesh.faces(), want["faces"])
    with pytest.raises(RuntimeError, match="No candidate triangles generated"):
        threecrate.alpha_shape_reconstruct(threecrate.PointCloud.from_numpy(AC.NO_CANDIDATE), 1.0)
    for n, k in ((300, 5), (700, 8), (40, 3), (6, 5), (6, 6)):
        p = AC.sphere(n, 11)
        got = threecrate.estimate_optimal_alpha(threecrate.PointCloud.from_numpy(p), k)
        assert np.float32(got) == K.estimate_optimal_alpha(p, k), (n, k)
