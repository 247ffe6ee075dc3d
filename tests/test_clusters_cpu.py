"""Euclidean cluster extraction, device-free: the checker against a plain restatement of the reference's BFS, and the
binding surfaces (Rust shim, compat module)."""
import os
import re
from collections import deque

import numpy as np
import pytest

from tests import cluster_checker as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def reference_bfs(pts, tol, min_size, max_size):
    """segmentation.rs:420-458 with a brute-force f32 find_radius_neighbors (nearest_neighbor.rs:254-298)."""
    pts = np.asarray(pts, np.float32)
    n = len(pts)
    r2 = np.float32(tol) * np.float32(tol)
    visited = np.zeros(n, bool)
    out = []
    for seed in range(n):
        if visited[seed]:
            continue
        cluster, queue = [], deque([seed])
        visited[seed] = True
        while queue:
            cur = queue.popleft()
            cluster.append(cur)
            d2 = K._d2(pts[cur][None, :], pts)
            for nb in np.nonzero(d2 <= r2)[0]:
                if not visited[nb]:
                    visited[nb] = True
                    queue.append(int(nb))
        if min_size <= len(cluster) <= max_size:
            out.append(cluster)
    out.sort(key=len, reverse=True)          # stable, like sort_by
    return out


def _same(pts, tol, mn, mx):
    ref = reference_bfs(pts, tol, mn, mx)
    got = K.cluster_lists(*K.clusters(pts, tol, mn, mx))
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.tolist() == sorted(r)            # same set, same rank; ascending inside the cluster
    return got


def test_checker_matches_reference_bfs_on_blobs():
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.3, 200, 1), K.sphere_cloud((10, 0, 0), 0.3, 150, 2),
                          K.sphere_cloud((0, 5, 0), 0.2, 40, 3), np.random.default_rng(4).uniform(-20, 20, (60, 3)).astype(np.float32)])
    got = _same(pts, 0.5, 1, 10000)
    assert len(got[0]) >= 200 and len(got[1]) >= 150
    _same(pts, 0.5, 50, 10000)
    _same(pts, 0.5, 1, 199)


def test_checker_matches_reference_bfs_on_random_clouds():
    rng = np.random.default_rng(7)
    for n, tol in [(300, 0.08), (500, 0.06), (800, 0.05)]:
        _same(rng.random((n, 3)).astype(np.float32), tol, 1, n)
        _same(rng.random((n, 3)).astype(np.float32), tol, 3, 50)


def test_checker_lattice_ties_connect_at_tol_and_not_below():
    pts = K.lattice((6, 5, 4), 0.5)
    got = _same(pts, 0.5, 1, len(pts))
    assert len(got) == 1 and len(got[0]) == len(pts)          # d2 == tol^2 exactly: adjacent
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    got = _same(pts, below, 1, len(pts))
    assert len(got) == len(pts)                               # just below: singletons, in index order
    assert [int(c[0]) for c in got] == list(range(len(pts)))


def test_checker_duplicates_nan_tolerance_and_non_finite_points():
    pts = np.array([[0, 0, 0], [0, 0, 0], [1, 1, 1], [np.nan, 0, 0], [1, 1, 1], [np.inf, 0, 0], [1, 1, 1.01]], np.float32)
    got = _same(pts, 0.05, 1, 10)
    assert [c.tolist() for c in got] == [[2, 4, 6], [0, 1], [3], [5]]
    labels, _, offsets = K.clusters(pts, float("nan"), 1, 10)
    assert labels.tolist() == list(range(len(pts))) and len(offsets) == len(pts) + 1


def test_checker_large_path_equals_all_pairs_path():
    rng = np.random.default_rng(3)
    pts = rng.random((21000, 3)).astype(np.float32)
    tol = 0.03
    i, j = K.f32_pairs(pts, tol)                       # cKDTree route (n > 20 k)
    sub = pts[:20000]
    a, b = K.f32_pairs(sub, tol)                       # all-pairs route
    m = (i < 20000) & (j < 20000)
    assert sorted(zip(i[m].tolist(), j[m].tolist())) == sorted(zip(a.tolist(), b.tolist()))


def test_rust_shim_has_the_cluster_functions_and_structs():
    src = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ["extract_euclidean_clusters", "extract_euclidean_clusters_parallel", "gpu_extract_euclidean_clusters", "gpu_extract_clusters"]:
        assert re.search(r"pub fn %s\s*\(" % fn, src), fn
    for st in ["GpuEuclideanClusterConfig", "GpuClusterExtractionResult"]:
        assert re.search(r"pub struct %s\b" % st, src), st
    m = re.search(r"pub struct GpuEuclideanClusterConfig\s*\{([^}]*)\}", src)
    assert [f.split(":")[0].replace("pub", "").strip() for f in m.group(1).split(",") if f.strip()] == \
        ["tolerance", "min_cluster_size", "max_cluster_size", "max_neighbors"]
    assert "tolerance: 0.02, min_cluster_size: 100, max_cluster_size: 25_000, max_neighbors: 64" in src
    ffi = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "ffi.rs")).read()
    assert "pub fn tc_extract_euclidean_clusters(" in ffi and "pub fn tc_extract_euclidean_clusters_device(" in ffi


def test_compat_names_extract_clusters():
    import inspect
    import threecrate_amd.compat as threecrate
    assert "extract_clusters" in threecrate.__all__
    sig = inspect.signature(threecrate.extract_clusters)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("cloud", inspect.Parameter.empty), ("tolerance", 0.02), ("min_cluster_size", 100), ("max_cluster_size", 25000)]


def test_header_declares_the_cluster_entry_points():
    hdr = open(os.path.join(ROOT, "include", "threecrate_hip.h")).read()
    assert "#define TC_CLUSTER_NONE 0xFFFFFFFFu" in hdr
    from threecrate_amd import _lib
    assert {"tc_extract_euclidean_clusters", "tc_extract_euclidean_clusters_device"} <= set(_lib.EXPORTS)
