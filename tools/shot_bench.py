#!/usr/bin/env python3
"""SHOT and USC descriptors (tc_extract_shot_features_with_normals, include/threecrate_hip_shot.h): one JSON line per workload and variant,
on tools/fpfh_bench.py's workloads, with the FPFH call on the same cloud beside it (the nearest existing cost).

  host_ms / device_ms   the whole call through host buffers / through the _device entry point (torch tensors), median of --iters calls
                        after --warmup, device-synchronised
  descriptors_per_s     points over device_ms
  phases_ms             per-stage kernel time of one device call (tc_profile_read: shot_index, shot_ball, shot_knn_fallback, shot_fallback,
                        and the index build's rows)
  fpfh_device_ms        tc_extract_fpfh_features_with_normals_device on the same cloud, radius and k

    python tools/shot_bench.py [--iters 10] [--warmup 3] [--only name,...]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import synth  # noqa: E402


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
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    work = [("kitti_shaped_r0.5", lambda: synth.kitti_shaped_cloud(), 0.5, 10),
            ("kitti_shaped_r1.0", lambda: synth.kitti_shaped_cloud(), 1.0, 10),
            ("uniform_100k_r0.1", lambda: synth.uniform_cloud(10**5), 0.1, 10)]
    if a.only:
        keep = set(a.only.split(","))
        work = [w for w in work if w[0] in keep]
    sync = torch.cuda.synchronize
    for name, make, radius, k in work:
        pts = np.ascontiguousarray(make(), np.float32)
        c6 = np.ascontiguousarray(ctx.estimate_normals(pts, 10), np.float32)
        x = torch.from_numpy(c6).to("cuda:0")
        fpfh_ms = timed(lambda: ctx.extract_fpfh_features_with_normals(x, radius, k), a.iters, a.warmup, sync)
        for variant in ("shot", "usc"):
            host_ms = timed(lambda: ctx.extract_shot_features(c6, radius, k, variant), a.iters, a.warmup)
            dev_ms = timed(lambda: ctx.extract_shot_features(x, radius, k, variant), a.iters, a.warmup, sync)
            ctx.profile_enable(1)
            ctx.profile_reset()
            _, _, flags = ctx.extract_shot_features(x, radius, k, variant, return_frames=True)
            sync()
            phases = {kk: round(v[1], 4) for kk, v in ctx.profile_read().items() if v[0]}
            ctx.profile_enable(0)
            ctx.profile_reset()
            fl = flags.cpu().numpy().view(np.uint32)
            row = {"workload": name, "variant": variant, "n": len(pts), "radius": radius, "k": k, "host_ms": round(host_ms, 3),
                   "device_ms": round(dev_ms, 3), "descriptors_per_s": round(len(pts) / dev_ms * 1e3), "fpfh_device_ms": round(fpfh_ms, 3),
                   "fallback_share": round(float((fl & 3 == 1).mean()), 4), "x_tie_share": round(float((fl & 4 != 0).mean()), 4), "phases_ms": phases}
            print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
