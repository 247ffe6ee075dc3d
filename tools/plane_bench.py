#!/usr/bin/env python3
"""RANSAC plane segmentation: one JSON line per workload.

  host_ms / device_ms   steady-state call through host buffers / through the _device entry point (torch tensors), median and
                        minimum of --iters calls after --warmup, device-synchronised
  phases_ms             kernel time per phase from the library's own events (tc_profile_read), minimum over --iters profiled
                        device calls on an otherwise idle stream: plane_model, plane_score, plane_winner, plane_inliers
  no_index_ms           the device call without the inlier list

    python tools/plane_bench.py [--iters 10] [--warmup 3] [--points 1000000] [--candidates 1000]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=10**6)
    ap.add_argument("--candidates", type=int, default=1000)
    ap.add_argument("--threshold", type=float, default=0.02)
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    sync = torch.cuda.synchronize
    for n, iters in sorted({(a.points, a.candidates), (max(3, a.points // 8), a.candidates)}, reverse=True):
        pts = synth.plane_clutter_cloud(n)
        x = torch.from_numpy(pts).to("cuda:0")
        host_med, host_min = timed(lambda: ctx.segment_plane(pts, a.threshold, iters), a.iters, a.warmup, sync)
        dev_med, dev_min = timed(lambda: ctx.segment_plane(x, a.threshold, iters), a.iters, a.warmup, sync)
        noidx_med, _ = timed(lambda: ctx.segment_plane(x, a.threshold, iters, return_index=False), a.iters, a.warmup, sync)
        ctx.profile_enable(1)
        phases = {}
        for _ in range(a.iters):
            ctx.profile_reset()
            r = ctx.segment_plane(x, a.threshold, iters)
            sync()
            for k, v in ctx.profile_read().items():
                if v[0] and k.startswith("plane_"):
                    phases[k] = min(phases.get(k, 1e30), v[1])
        ctx.profile_enable(0)
        ctx.profile_reset()
        print(json.dumps({"n": n, "candidates": iters, "threshold": a.threshold, "inliers": r.num_inliers, "best_iteration": r.best_iteration,
                          "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3), "device_ms": round(dev_med, 3),
                          "device_min_ms": round(dev_min, 3), "no_index_ms": round(noidx_med, 3),
                          "phases_ms": {k: round(v, 4) for k, v in sorted(phases.items())}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
