#!/usr/bin/env python3
"""Euclidean cluster extraction: one JSON line per workload.

  host_ms / device_ms   steady-state call through host buffers / through the _device entry point (torch tensors), median of
                        --iters calls after --warmup, device-synchronised
  phases_ms             per-phase kernel time of one device call (tc_profile_read; index build phases included)
  radius_host_ms        what a caller can do without this entry point: tc_search_index_create + tc_search_index_radius_count/fill
                        on the device, scipy.sparse.csgraph.connected_components on the host, then the same filter and order
  ckdtree_ms            a CPU route: scipy cKDTree.query_pairs + connected_components (+ filter and order)

    python tools/cluster_bench.py [--iters 10] [--warmup 3] [--no-baselines]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: see tests/conftest.py)
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import _lib, synth  # noqa: E402


def _rank(n, i, j, mn, mx):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ncomp, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)
    size = np.bincount(comp, minlength=ncomp)
    _, first = np.unique(comp, return_index=True)
    keep = np.nonzero((size >= mn) & (size <= mx))[0]
    return keep[np.lexsort((first[keep], -size[keep]))]


def radius_route(ctx, pts, tol, mn, mx):
    L = _lib.load()
    n = len(pts)
    h = C.c_void_p()
    if L.tc_search_index_create(ctx._h, pts.ctypes.data, n, 16, C.byref(h)) != 0:
        raise RuntimeError("tc_search_index_create failed")
    try:
        cnt = np.zeros(n, np.uint32)
        ctx._check(L.tc_search_index_radius_count(h, pts.ctypes.data, n, tol, cnt.ctypes.data))
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        total = int(off[-1])
        idx = np.zeros(max(total, 1), np.uint32)
        dist = np.zeros(max(total, 1), np.float32)
        ctx._check(L.tc_search_index_radius_fill(h, pts.ctypes.data, n, tol, off.ctypes.data, total, idx.ctypes.data, dist.ctypes.data))
    finally:
        L.tc_search_index_destroy(h)
    rows = np.repeat(np.arange(n, dtype=np.int64), cnt.astype(np.int64))
    return _rank(n, rows, idx[:total].astype(np.int64), mn, mx)


def ckdtree_route(pts, tol, mn, mx):
    from scipy.spatial import cKDTree
    pr = cKDTree(pts.astype(np.float64)).query_pairs(tol, output_type="ndarray")
    return _rank(len(pts), pr[:, 0], pr[:, 1], mn, mx)


def timed(fn, iters, warmup, sync=None):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-baselines", action="store_true")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    work = [("kitti_shaped", synth.kitti_shaped_cloud(), 0.5, 10, 25000),
            ("uniform_1M_tol0.0086", synth.uniform_cloud(10**6), 0.0086, 10, 25000),
            ("uniform_1M_tol0.02", synth.uniform_cloud(10**6), 0.02, 1, 10**6),
            ("tum_shaped", synth.tum_shaped_cloud(), 0.02, 100, 25000)]
    sync = torch.cuda.synchronize
    for name, pts, tol, mn, mx in work:
        pts = np.ascontiguousarray(pts, np.float32)
        host_med, host_min = timed(lambda: ctx.extract_euclidean_clusters_labels(pts, tol, mn, mx), a.iters, a.warmup)
        x = torch.from_numpy(pts).to("cuda:0")
        dev_med, dev_min = timed(lambda: ctx.extract_euclidean_clusters_labels(x, tol, mn, mx), a.iters, a.warmup, sync)
        ctx.profile_enable(1)
        ctx.profile_reset()
        _, _, offsets = ctx.extract_euclidean_clusters_labels(x, tol, mn, mx)
        sync()
        phases = {k: round(v[1], 4) for k, v in ctx.profile_read().items() if v[0]}
        ctx.profile_enable(0)
        ctx.profile_reset()
        row = {"workload": name, "n": len(pts), "tol": tol, "min": mn, "max": mx, "clusters": int(len(offsets) - 1),
               "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3), "device_ms": round(dev_med, 3),
               "device_min_ms": round(dev_min, 3), "phases_ms": phases}
        if not a.no_baselines:
            t0 = time.perf_counter()
            order_r = radius_route(ctx, pts, tol, mn, mx)
            row["radius_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            ckdtree_route(pts, tol, mn, mx)
            row["ckdtree_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["radius_route_clusters"] = int(len(order_r))
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
