#!/usr/bin/env python3
"""FPFH descriptors: one JSON line per workload.

  host_ms / device_ms   steady-state tc_extract_fpfh_features_with_normals through host buffers / through the _device entry point
                        (torch tensors), median of --iters calls after --warmup, device-synchronised
  phases_ms             per-phase kernel time of one device call (tc_profile_read; index build phases included)
  search_route_ms       what a caller can do without this entry point: tc_search_index radius count / fill on the device (the
                        k-NN fallback through the same index), then the histograms in numpy on the host (tests/fpfh_checker.py's
                        pair features over the fetched lists)
  cpu_ms                a CPU route: the checker itself (cKDTree + numpy)

    python tools/fpfh_bench.py [--iters 10] [--warmup 3] [--no-baselines]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (first: see tests/conftest.py)
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import _lib, synth  # noqa: E402
from tests import fpfh_checker as F  # noqa: E402


def search_route(ctx, pos, nrm, radius, k):
    """radius lists (+ k-NN fallback) from the search index on the device, SPFH / FPFH in numpy on the host"""
    L = _lib.load()
    n = len(pos)
    h = C.c_void_p()
    if L.tc_search_index_create(ctx._h, pos.ctypes.data, n, 16, C.byref(h)) != 0:
        raise RuntimeError("tc_search_index_create failed")
    try:
        cnt = np.zeros(n, np.uint32)
        ctx._check(L.tc_search_index_radius_count(h, pos.ctypes.data, n, radius, cnt.ctypes.data))
        off = np.zeros(n + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        total = int(off[-1])
        idx = np.zeros(max(total, 1), np.uint32)
        dist = np.zeros(max(total, 1), np.float32)
        ctx._check(L.tc_search_index_radius_fill(h, pos.ctypes.data, n, radius, off.ctypes.data, total, idx.ctypes.data, dist.ctypes.data))
        rows = np.repeat(np.arange(n), cnt.astype(np.int64))
        cols = idx[:total].astype(np.int64)
        keep = rows != cols
        rows, cols = rows[keep], cols[keep]
        nl = np.bincount(rows, minlength=n)
        fb = np.nonzero(nl < k)[0]
        if len(fb):
            q = np.ascontiguousarray(pos[fb])
            ki = np.zeros((len(fb), k + 1), np.uint32)
            kd = np.zeros((len(fb), k + 1), np.float32)
            kc = np.zeros(len(fb), np.uint32)
            ctx._check(L.tc_search_index_query(h, q.ctypes.data, len(fb), k + 1, C.c_float(-1.0), ki.ctypes.data, kd.ctypes.data, kc.ctypes.data))
            drop = np.isin(rows, fb)
            rows, cols = rows[~drop], cols[~drop]
            fr, fc = [], []
            for s, i in enumerate(fb):
                lst = ki[s, :kc[s]].astype(np.int64)
                lst = lst[lst != i][:k]
                fr.append(np.full(len(lst), i)); fc.append(lst)
            rows, cols = np.concatenate([rows] + fr), np.concatenate([cols] + fc)
    finally:
        L.tc_search_index_destroy(h)
    o = np.argsort(rows, kind="stable")
    rows, cols = rows[o], cols[o]
    valid, bins, _ = F.pair_bins(pos[rows], nrm[rows], pos[cols], nrm[cols])
    counts = np.zeros((n, F.DIM), np.float32)
    for c in range(3):
        np.add.at(counts, (rows[valid], bins[valid, c]), 1)
    nv = np.bincount(rows[valid], minlength=n).astype(np.float32)
    spfh = counts * np.where(nv > 0, np.float32(1) / np.maximum(nv, 1), 0).astype(np.float32)[:, None]
    w = np.float32(1) / np.sqrt(F.d2_f32(pos[cols], pos[rows]))
    w[~np.isfinite(w)] = 0
    acc = np.zeros((n, F.DIM), np.float32)
    np.add.at(acc, rows, w[:, None] * spfh[cols])
    ws = np.bincount(rows, weights=w, minlength=n).astype(np.float32)
    desc = spfh + np.where(ws > 0, 1 / np.maximum(ws, 1e-30), 0)[:, None].astype(np.float32) * acc
    for p in range(3):
        s = desc[:, 11 * p:11 * p + 11].sum(1, keepdims=True)
        desc[:, 11 * p:11 * p + 11] = np.where(s > 0, desc[:, 11 * p:11 * p + 11] / np.where(s > 0, s, 1), desc[:, 11 * p:11 * p + 11])
    return desc


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
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    work = [("kitti_shaped_r0.5", lambda: synth.kitti_shaped_cloud(), 0.5, 10),
            ("kitti_shaped_r1.0", lambda: synth.kitti_shaped_cloud(), 1.0, 10),
            ("uniform_1M_r0.023", lambda: synth.uniform_cloud(10**6), 0.023, 10),
            ("uniform_100k_defaults", lambda: synth.uniform_cloud(10**5), 0.1, 10),
            ("tum_shaped_r0.02", lambda: synth.tum_shaped_cloud(), 0.02, 10)]
    if a.only:
        keep = set(a.only.split(","))
        work = [w for w in work if w[0] in keep]
    sync = torch.cuda.synchronize
    for name, make, radius, k in work:
        pts = np.ascontiguousarray(make(), np.float32)
        c6 = np.ascontiguousarray(ctx.estimate_normals(pts, 10), np.float32)
        host_med, host_min = timed(lambda: ctx.extract_fpfh_features_with_normals(c6, radius, k), a.iters, a.warmup)
        x = torch.from_numpy(c6).to("cuda:0")
        dev_med, dev_min = timed(lambda: ctx.extract_fpfh_features_with_normals(x, radius, k), a.iters, a.warmup, sync)
        xyz = torch.from_numpy(pts).to("cuda:0")
        xyz_med, _ = timed(lambda: ctx.extract_fpfh_features(xyz, radius, k), a.iters, a.warmup, sync)
        ctx.profile_enable(1)
        ctx.profile_reset()
        ctx.extract_fpfh_features_with_normals(x, radius, k)
        sync()
        phases = {kk: round(v[1], 4) for kk, v in ctx.profile_read().items() if v[0]}
        ctx.profile_enable(0)
        ctx.profile_reset()
        row = {"workload": name, "n": len(pts), "radius": radius, "k": k, "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3),
               "device_ms": round(dev_med, 3), "device_min_ms": round(dev_min, 3), "xyz_device_ms": round(xyz_med, 3), "phases_ms": phases}
        if not a.no_baselines:
            pos, nrm = c6[:, :3].copy(), c6[:, 3:].copy()
            t0 = time.perf_counter()
            search_route(ctx, pos, nrm, radius, k)
            row["search_route_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            t0 = time.perf_counter()
            rows = None if len(pos) <= 200000 else np.random.default_rng(0).choice(len(pos), 20000, replace=False)
            F.fpfh(pos, nrm, radius, k, rows)
            ms = (time.perf_counter() - t0) * 1e3
            row["cpu_ms"] = round(ms if rows is None else ms * len(pos) / len(rows), 1)
            row["cpu_extrapolated"] = rows is not None
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
