"""Euclidean cluster extraction on the MI355X: the reference's unit tests restated (segmentation.rs:890-1015), exact
partition equality with the checker (labels and member lists equal), edge cases, the device entry point, errors."""
import ctypes as C

import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, synth
from tests import cluster_checker as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _exact(ctx, pts, tol, mn, mx):
    labels, members, offsets = ctx.extract_euclidean_clusters_labels(pts, tol, mn, mx)
    el, em, eo = K.clusters(pts, tol, mn, mx)
    assert len(offsets) == len(eo), (len(offsets), len(eo))
    assert np.array_equal(offsets, eo)
    assert np.array_equal(labels, el), int(np.count_nonzero(labels != el))
    assert np.array_equal(members, em)
    return labels, members, offsets


# ---- the reference's unit tests (segmentation.rs:890-1015) ----
def test_two_blobs(ctx):
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.3, 200, 1), K.sphere_cloud((10, 0, 0), 0.3, 150, 2)])
    cl = ctx.extract_euclidean_clusters(pts, 0.5, 50, 10000)
    assert len(cl) == 2 and len(cl[0]) >= len(cl[1])
    assert cl[0].tolist() == list(range(200)) and cl[1].tolist() == list(range(200, 350))


def test_three_blobs(ctx):
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.4, 300, 1), K.sphere_cloud((5, 0, 0), 0.4, 200, 2),
                          K.sphere_cloud((0, 5, 0), 0.4, 100, 3)])
    assert [len(c) for c in ctx.extract_euclidean_clusters(pts, 0.6, 50, 10000)] == [300, 200, 100]


def test_min_and_max_size_filters(ctx):
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.4, 300, 1), K.sphere_cloud((10, 0, 0), 0.2, 5, 2)])
    assert len(ctx.extract_euclidean_clusters(pts, 0.5, 50, 10000)) == 1
    big = K.sphere_cloud((0, 0, 0), 0.5, 500, 3)
    assert len(ctx.extract_euclidean_clusters(big, 0.6, 1, 100)) == 0


def test_get_cluster_cloud_and_compat(ctx):
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.3, 200, 1), K.sphere_cloud((10, 0, 0), 0.3, 100, 2)])
    clouds = threecrate.extract_clusters(threecrate.PointCloud(pts), 0.5, 50, 10000)
    assert [len(c) for c in clouds] == [200, 100]
    assert np.array_equal(clouds[1].to_numpy(), pts[200:])
    dense = K.sphere_cloud((0, 0, 0), 0.05, 3000, 3)                               # the wheel's defaults: 0.02, 100, 25000
    want = K.cluster_lists(*K.clusters(dense, 0.02, 100, 25000))
    got = threecrate.extract_clusters(threecrate.PointCloud(dense))
    assert len(got) == len(want) >= 1
    assert all(np.array_equal(g.to_numpy(), dense[w]) for g, w in zip(got, want))


def test_invalid_configs(ctx):
    one = np.zeros((1, 3), np.float32)
    for args, msg in [((np.zeros((0, 3), np.float32), 0.1, 1, 100), "Point cloud is empty"), ((one, -1.0, 1, 100), "Tolerance must be positive"),
                      ((one, 0.0, 1, 100), "Tolerance must be positive"), ((one, 0.1, 0, 100), "min_cluster_size must be at least 1"),
                      ((one, 0.1, 10, 5), "min_cluster_size must not exceed max_cluster_size")]:
        with pytest.raises(tc.InvalidData, match=msg):
            ctx.extract_euclidean_clusters(*args)
        with pytest.raises(RuntimeError, match=msg):
            threecrate.extract_clusters(threecrate.PointCloud(args[0]), *args[1:])
    with pytest.raises(tc.Unsupported):
        ctx.extract_euclidean_clusters(one, 1e20, 1, 10)           # tol * tol overflows
    with pytest.raises(tc.Unsupported):
        ctx.extract_euclidean_clusters(one, float("inf"), 1, 10)


# ---- exact partitions ----
def test_exact_uniform_near_percolation(ctx):
    _exact(ctx, synth.uniform_cloud(100_000, seed=5), 0.0185, 1, 100_000)
    _exact(ctx, synth.uniform_cloud(100_000, seed=6), 0.0185, 10, 500)


def test_exact_kitti_shaped(ctx):
    _exact(ctx, synth.kitti_shaped_cloud(), 0.5, 10, 25000)


def test_exact_tum_shaped(ctx):
    _exact(ctx, synth.tum_shaped_cloud(step=2), 0.02, 1, 10**6)


def test_exact_blobs_with_far_outliers(ctx):
    rng = np.random.default_rng(11)
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 1.0, 20000, 1), K.sphere_cloud((3, 0, 0), 0.5, 5000, 2),
                          rng.uniform(-1e5, 1e5, (50, 3)).astype(np.float32)])
    pts = pts[rng.permutation(len(pts))]
    _exact(ctx, pts, 0.05, 1, len(pts))


def test_exact_duplicates(ctx):
    rng = np.random.default_rng(12)
    base = rng.random((3000, 3)).astype(np.float32)
    pts = np.concatenate([base, base[:1000], base[:1000], np.repeat(base[:1], 500, axis=0)])
    pts = pts[rng.permutation(len(pts))]
    _exact(ctx, pts, 0.02, 1, len(pts))
    _exact(ctx, pts, 1e-7, 2, len(pts))          # only the exact duplicates connect


def test_exact_lattice_ties(ctx):
    pts = K.lattice((40, 30, 20), 0.5)
    pts = pts[np.random.default_rng(13).permutation(len(pts))]
    labels, _, offsets = _exact(ctx, pts, 0.5, 1, len(pts))
    assert len(offsets) == 2                              # ties connect: one component
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    labels, _, offsets = _exact(ctx, pts, below, 1, len(pts))
    assert len(offsets) == len(pts) + 1                   # just below: all singletons


def test_exact_long_chain(ctx):
    n, tol = 200_000, 0.01
    x = np.arange(n, dtype=np.float64) * (0.9 * tol)
    pts = np.stack([x, np.zeros(n), np.zeros(n)], 1).astype(np.float32)
    pts = pts[np.random.default_rng(14).permutation(n)]
    labels, members, offsets = _exact(ctx, pts, tol, 1, n)
    assert len(offsets) == 2 and int(offsets[1]) == n


def test_exact_one_million(ctx):
    pts = synth.uniform_cloud(10**6, seed=2)
    _, _, offsets = _exact(ctx, pts, 0.02, 1, 10**6)
    assert int(offsets[1] - offsets[0]) > 900_000        # one giant component
    _exact(ctx, pts, 0.0086, 1, 10**6)


# ---- edge cases ----
def test_nan_tolerance_gives_singletons_in_index_order(ctx):
    pts = synth.uniform_cloud(5000, seed=3)
    labels, members, offsets = _exact(ctx, pts, float("nan"), 1, 10)
    assert labels.tolist() == list(range(5000)) and members.tolist() == list(range(5000))


def test_non_finite_points_are_singletons(ctx):
    pts = synth.uniform_cloud(20000, seed=4)
    pts[::97, 0] = np.nan
    pts[5::101, 2] = np.inf
    pts[7::103, 1] = -np.inf
    labels, _, _ = _exact(ctx, pts, 0.03, 1, len(pts))
    bad = ~np.all(np.isfinite(pts), axis=1)
    assert np.all(np.bincount(labels[bad], minlength=1)[labels[bad]] == 1)


def test_max_filters_the_giant_component_and_n_equals_one(ctx):
    pts = synth.uniform_cloud(50000, seed=8)
    labels, _, offsets = _exact(ctx, pts, 0.05, 1, 1000)
    assert np.count_nonzero(labels == K.NONE) > 40000
    labels, members, offsets = ctx.extract_euclidean_clusters_labels(np.ones((1, 3), np.float32), 0.1, 1, 1)
    assert labels.tolist() == [0] and members.tolist() == [0] and offsets.tolist() == [0, 1]
    assert ctx.extract_euclidean_clusters(np.ones((1, 3), np.float32), 0.1, 2, 5) == []


# ---- device entry point ----
def test_device_entry_point_equals_host_and_is_deterministic(ctx):
    torch = pytest.importorskip("torch")
    pts = synth.uniform_cloud(300_000, seed=9)
    hl, hm, ho = ctx.extract_euclidean_clusters_labels(pts, 0.012, 5, 50000)
    x = torch.from_numpy(pts).to("cuda:0")
    dl, dm, do = ctx.extract_euclidean_clusters_labels(x, 0.012, 5, 50000)
    torch.cuda.synchronize()
    assert np.array_equal(dl.cpu().numpy().view(np.uint32), hl)
    assert np.array_equal(dm.cpu().numpy().view(np.uint32), hm)
    assert np.array_equal(do.cpu().numpy().astype(np.uint64), ho)
    dl2, _, _ = ctx.extract_euclidean_clusters_labels(x, 0.012, 5, 50000)
    assert torch.equal(dl, dl2)
    cl = ctx.extract_euclidean_clusters(x, 0.012, 5, 50000)
    assert len(cl) == len(ho) - 1 and all(c.is_cuda for c in cl)


def test_c_abi_status_and_message(ctx):
    L = _lib.load()
    one = np.zeros((1, 3), np.float32)
    n_cl = C.c_size_t(7)
    lab = np.zeros(1, np.uint32)
    rc = L.tc_extract_euclidean_clusters(ctx._h, one.ctypes.data, 1, 0.0, 1, 10, lab.ctypes.data, None, None, C.byref(n_cl))
    assert rc == _lib.TC_INVALID_DATA and n_cl.value == 0
    rc = L.tc_extract_euclidean_clusters(ctx._h, one.ctypes.data, 1, 1.0, 1, 10, lab.ctypes.data, lab.ctypes.data, None, C.byref(n_cl))
    assert rc == _lib.TC_INVALID_DATA                      # members without offsets
    rc = L.tc_extract_euclidean_clusters(ctx._h, one.ctypes.data, 1, 1.0, 1, 10, lab.ctypes.data, None, None, C.byref(n_cl))
    assert rc == _lib.TC_OK and n_cl.value == 1 and lab.tolist() == [0]
