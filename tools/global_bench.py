#!/usr/bin/env python3
"""Descriptor matching and RANSAC over correspondences: one JSON line per workload.

  host_ms / device_ms   steady-state call through host buffers / through the _device entry point (torch tensors), median and
                        minimum of --iters calls after --warmup, device-synchronised
  phases_ms             kernel time per phase from the library's own events (tc_profile_read), summed over the launches of one call,
                        minimum over --iters profiled device calls: match_features; ransac_gather, ransac_models, ransac_score,
                        ransac_fold

Matching runs on random descriptors of --match x --match rows; RANSAC runs the default configuration (50 000 candidates, inlier ratio
0.25, threshold 0.05) on synth.registration_pair(--points), first with the identity correspondences (the exit comes in the first
chunk), then with the early exit out of reach (every chunk is scored).

    python tools/global_bench.py [--iters 10] [--warmup 3] [--match 100000] [--points 100000]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: see tests/conftest.py)
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import synth  # noqa: E402


def timed(fn, iters, warmup, sync):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def phases(ctx, fn, iters, sync, prefix):
    ctx.profile_enable(1)
    out = {}
    for _ in range(iters):
        ctx.profile_reset()
        fn()
        sync()
        for k, v in ctx.profile_read().items():
            if v[0] and k.startswith(prefix):
                out[k] = min(out.get(k, 1e30), v[1])
    ctx.profile_enable(0)
    ctx.profile_reset()
    return {k: round(v, 4) for k, v in sorted(out.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--match", type=int, default=100_000)
    ap.add_argument("--points", type=int, default=100_000)
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(0)
    sd, td = rng.random((a.match, 33), np.float32), rng.random((a.match, 33), np.float32)
    dsd, dtd = torch.from_numpy(sd).to("cuda:0"), torch.from_numpy(td).to("cuda:0")
    host_med, host_min = timed(lambda: ctx.match_features(sd, td), a.iters, a.warmup, sync)
    dev_med, dev_min = timed(lambda: ctx.match_features(dsd, dtd), a.iters, a.warmup, sync)
    print(json.dumps({"step": "match_features", "ns": a.match, "nt": a.match, "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3),
                      "device_ms": round(dev_med, 3), "device_min_ms": round(dev_min, 3),
                      "phases_ms": phases(ctx, lambda: ctx.match_features(dsd, dtd), a.iters, sync, "match_")}), flush=True)
    src, tgt, _ = synth.registration_pair(a.points, seed=3)
    corr = np.arange(a.points, dtype=np.uint32)
    dsrc, dtgt = torch.from_numpy(src).to("cuda:0"), torch.from_numpy(tgt).to("cuda:0")
    dcorr = torch.from_numpy(corr.view(np.int32)).to("cuda:0")
    for name, ratio in (("exit in the first chunk", 0.25), ("every chunk scored", 2.0)):
        host = lambda: ctx.ransac_correspondences(src, tgt, corr, corr, 0.05, ratio)
        dev = lambda: ctx.ransac_correspondences(dsrc, dtgt, dcorr, dcorr, 0.05, ratio)
        host_med, host_min = timed(host, a.iters, a.warmup, sync)
        dev_med, dev_min = timed(dev, a.iters, a.warmup, sync)
        r = dev()
        print(json.dumps({"step": "ransac_correspondences", "case": name, "m": a.points, "candidates": 50_000, "inlier_ratio": ratio,
                          "inliers": r.inlier_count, "iterations_run": r.iterations_run, "host_ms": round(host_med, 3),
                          "host_min_ms": round(host_min, 3), "device_ms": round(dev_med, 3), "device_min_ms": round(dev_min, 3),
                          "phases_ms": phases(ctx, dev, a.iters, sync, "ransac_")}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
