"""Ground segmentation on the device (include/threecrate_hip_ground.h, csrc/ground.hip) against the numpy restatement of its contract
(tests/ground_checker.py): for every case of tests/ground_cases.py, through both the host and the _device road, the labels, the statuses
and the counts EQUAL the checker's, with no tolerance and no excused point: tests/test_ground_cpu.py has proven every case at a margin of
1e-6 or more, nine orders of magnitude above what the order of an f64 sum can move.  The float fields of the patch table are held to
1e-5 absolute."""
import ctypes as C

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import ground_cases as GCASES
from tests import ground_checker as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import threecrate_amd as tc
    c = tc.GpuContext(0)
    yield c
    c.close()


def _run(ctx, road, points, cfg, **kw):
    import torch
    import threecrate_amd as tc
    p = points if road == "host" else torch.from_numpy(np.array(points)).to("cuda:0")
    r = ctx.segment_ground(p, config=tc.GpuContext.ground_config(**cfg), **kw)
    if road == "device":
        assert isinstance(r["labels"], torch.Tensor) and r["labels"].is_cuda
        for k in ("labels", "ground", "nonground", "ground_points", "nonground_points"):
            if k in r:
                r[k] = r[k].cpu().numpy()
        for k in ("ground", "nonground"):
            if k in r:
                r[k] = r[k].view(np.uint32)
    return r


def _check(r, want, n):
    assert r["labels"].dtype == bool and r["labels"].shape == (n,)
    assert np.array_equal(r["labels"], want["labels"]), np.flatnonzero(r["labels"] != want["labels"])[:10]
    got, exp = r["patches"], want["patches"]
    assert got.dtype == GC.PATCH_DTYPE and got.shape == exp.shape
    for field in ("count", "status", "n_inliers"):
        assert np.array_equal(got[field], exp[field]), (field, np.flatnonzero(got[field] != exp[field])[:10])
    for field in ("normal", "d", "mean_z", "flatness"):
        worst = float(np.abs(got[field].astype(np.float64) - exp[field].astype(np.float64)).max()) if len(got) else 0.0
        assert worst <= 1e-5, (field, worst)
    # the index lists: ascending, disjoint, adding to n, agreeing with the labels
    g, ng = r["ground"].astype(np.int64), r["nonground"].astype(np.int64)
    assert r["n_ground"] == len(g) == int(want["labels"].sum()) and len(g) + len(ng) == n
    assert np.array_equal(g, np.flatnonzero(want["labels"])) and np.array_equal(ng, np.flatnonzero(~want["labels"]))


@pytest.mark.parametrize("road", ["host", "device"])
@pytest.mark.parametrize("name", list(GCASES.CASES))
def test_labels_and_patch_table_equal_the_checker(ctx, name, road):
    points, cfg = GCASES.case(name)
    _check(_run(ctx, road, points, cfg), GCASES.expected(name), len(points))


@pytest.mark.parametrize("road", ["host", "device"])
def test_two_calls_give_identical_bits(ctx, road):
    for name in ("scene", "sizes_stage", "statuses"):
        points, cfg = GCASES.case(name)
        a, b = _run(ctx, road, points, cfg), _run(ctx, road, points, cfg)
        assert a["labels"].tobytes() == b["labels"].tobytes() and a["patches"].tobytes() == b["patches"].tobytes()
        assert a["ground"].tobytes() == b["ground"].tobytes() and a["nonground"].tobytes() == b["nonground"].tobytes()


@pytest.mark.parametrize("name", ["scene", "kitti16", "statuses", "data_edges"])
def test_a_permutation_of_the_input_gives_every_point_the_same_label(ctx, name):
    points, cfg = GCASES.case(name)
    perm = np.random.default_rng(1).permutation(len(points))
    want = GCASES.expected(name)
    r = _run(ctx, "host", np.ascontiguousarray(points[perm]), cfg)
    assert np.array_equal(r["labels"], want["labels"][perm])
    assert np.array_equal(r["patches"]["status"], want["patches"]["status"]) and np.array_equal(r["patches"]["n_inliers"], want["patches"]["n_inliers"])


def test_the_empty_cloud(ctx):
    import torch
    for p in (np.zeros((0, 3), np.float32), torch.zeros((0, 3), device="cuda:0")):
        r = ctx.segment_ground(p, sensor_height=1.8)
        assert len(r["labels"]) == 0 and r["n_ground"] == 0 and len(r["ground"]) == 0 and len(r["nonground"]) == 0
        assert len(r["patches"]) == 504 and not r["patches"].tobytes().strip(b"\0")


def test_compat_returns_the_references_result_shape(ctx):
    import threecrate_amd.compat as threecrate
    points, _ = GCASES.case("scene")
    want = GCASES.expected("scene")
    cloud = threecrate.PointCloud.from_numpy(np.array(points))
    for r in (threecrate.segment_ground(cloud, 1.8), threecrate.patchwork_plus_plus(cloud, threecrate.PatchworkConfig(sensor_height=1.8))):
        assert isinstance(r, threecrate.GroundSegmentationResult) and isinstance(r.ground, threecrate.PointCloud) and isinstance(r.nonground, threecrate.PointCloud)
        assert isinstance(r.labels, list) and r.labels == want["labels"].tolist()
        assert np.array_equal(r.ground.to_numpy(), points[want["labels"]]) and np.array_equal(r.nonground.to_numpy(), points[~want["labels"]])
        assert len(r.ground) + len(r.nonground) == len(cloud)
    empty = threecrate.segment_ground(threecrate.PointCloud(), 1.8)
    assert len(empty.ground) == 0 and len(empty.nonground) == 0 and empty.labels == []
    bad = threecrate.PatchworkConfig(zone_radii=[0.0, 10.0], num_rings_per_zone=[2, 2], num_sectors_per_zone=[8, 8])
    with pytest.raises(RuntimeError, match="zone_radii"):
        threecrate.patchwork_plus_plus(cloud, bad)
    with pytest.raises(RuntimeError, match="dist_threshold must be positive"):
        threecrate.patchwork_plus_plus(cloud, threecrate.PatchworkConfig(dist_threshold=0.0))


@pytest.mark.parametrize("road", ["host", "device"])
def test_the_outputs_that_may_be_null(ctx, road):
    import torch
    import threecrate_amd as tc
    points, cfg = GCASES.case("statuses")
    want = GCASES.expected("statuses")
    n, n_patches = len(points), len(want["patches"])
    L = _lib.load_companion("threecrate_hip_ground.h")
    fn = L.tc_segment_ground if road == "host" else L.tc_segment_ground_device
    c = tc.GpuContext.ground_config(**cfg)
    dev = road == "device"
    new = lambda shape, dtype: torch.full(shape, 7, dtype=getattr(torch, {np.uint8: "uint8", np.uint32: "int32"}[dtype]), device="cuda:0") if dev else np.full(shape, 7, dtype)
    ptr = lambda a: a.data_ptr() if dev else a.ctypes.data
    host = lambda a: a.cpu().numpy() if dev else a
    p = torch.from_numpy(np.array(points)).to("cuda:0") if dev else points
    for mask in range(8):
        labels = new((n,), np.uint8)
        g = new((n,), np.uint32) if mask & 1 else None
        ng = new((n,), np.uint32) if mask & 2 else None
        pt = new((n_patches * GC.PATCH_DTYPE.itemsize,), np.uint8) if mask & 4 else None
        count = C.c_size_t(7)
        if dev:
            torch.cuda.synchronize()
        rc = fn(ctx._h, ptr(p), n, C.byref(c), ptr(labels), None if g is None else ptr(g), None if ng is None else ptr(ng), None if pt is None else ptr(pt),
                C.byref(count))
        assert rc == _lib.TC_OK, mask
        k = int(want["labels"].sum())
        assert count.value == k and np.array_equal(host(labels) != 0, want["labels"]) and set(np.unique(host(labels))) <= {0, 1}
        if g is not None:
            assert np.array_equal(host(g).view(np.uint32)[:k], np.flatnonzero(want["labels"])) and (host(g).view(np.uint32)[k:] == (7 if not dev else 7)).all()
        if ng is not None:
            assert np.array_equal(host(ng).view(np.uint32)[:n - k], np.flatnonzero(~want["labels"])) and (host(ng).view(np.uint32)[n - k:] == 7).all()
        if pt is not None:
            got = np.ascontiguousarray(host(pt)).view(GC.PATCH_DTYPE)
            assert np.array_equal(got["status"], want["patches"]["status"]) and np.array_equal(got["count"], want["patches"]["count"])


def test_one_context_serves_this_companion_and_the_main_library_in_turn(ctx):
    from threecrate_amd import synth
    points, cfg = GCASES.case("scene")
    want = GCASES.expected("scene")
    cloud = synth.uniform_cloud(3000, seed=2)
    before = ctx.estimate_normals(cloud, 8)
    for _ in range(2):
        r = _run(ctx, "host", points, cfg)
        assert np.array_equal(r["labels"], want["labels"])
        filtered = ctx.voxel_grid_filter(points[r["nonground"].astype(np.int64)], 0.5)
        assert 0 < len(filtered) <= len(r["nonground"])
        assert ctx.estimate_normals(cloud, 8).tobytes() == before.tobytes()


def test_too_many_patches_is_unsupported(ctx):
    import threecrate_amd as tc
    points, _ = GCASES.case("n2")
    with pytest.raises(tc.Unsupported, match="65536"):
        _run(ctx, "host", points, GCASES.too_many_patches())
