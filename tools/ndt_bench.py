#!/usr/bin/env python3
"""NDT registration: one JSON line per workload.

  host_ms / device_ms   steady-state call through host buffers / through the _device entry point (torch tensors), median and
                        minimum of --iters calls after --warmup, device-synchronised
  phases_ms             kernel time per phase from the library's own events (tc_profile_read), minimum per launch over --iters
                        profiled device calls: ndt_voxel_keys, ndt_voxel_stats, ndt_table, ndt_evaluate, ndt_finalize
  evaluate              the hot path: microseconds per launch, the bytes of its model (per source point 12 B of source, 4 B of table
                        and, for a hit, the 48-byte record; nothing else is counted) and their fraction of the 8 TB/s roof

Workloads: the synthetic 64-beam LiDAR frame (120 k points) against itself moved a little, resolution 1.0; a uniform 1 M-point pair.

    python tools/ndt_bench.py [--iters 10] [--warmup 3] [--points 1000000] [--steps 10]
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

ROOF_BYTES_PER_S = 8e12


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
    ap.add_argument("--steps", type=int, default=10, help="NDT iterations per call (epsilon 0: every one runs)")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    sync = torch.cuda.synchronize
    move = synth.yaw_isometry((0.05, -0.04, 0.02), 0.01)
    frame = synth.kitti_shaped_cloud()
    src_u, tgt_u, _ = synth.registration_pair(a.points, seed=1)
    side = round(a.points ** (1.0 / 3.0)) / 8.0                 # the uniform pair scaled to ~8 points per voxel of resolution 1 / 4
    workloads = [("lidar_frame", synth.apply_isometry(move, frame).astype(np.float32), frame, 1.0),
                 ("uniform_pair", (src_u * side).astype(np.float32), (tgt_u * side).astype(np.float32), 0.25)]
    for name, src, tgt, res in workloads:
        kw = dict(resolution=res, max_iterations=a.steps, epsilon=0.0)
        ds, dt = torch.from_numpy(src).to("cuda:0"), torch.from_numpy(tgt).to("cuda:0")
        host_med, host_min = timed(lambda: ctx.ndt_registration(src, tgt, None, **kw), a.iters, a.warmup, sync)
        dev_med, dev_min = timed(lambda: ctx.ndt_registration(ds, dt, None, **kw), a.iters, a.warmup, sync)
        ctx.profile_enable(1)
        phases = {}
        for _ in range(a.iters):
            ctx.profile_reset()
            r = ctx.ndt_registration(ds, dt, None, **kw)
            sync()
            for k, v in ctx.profile_read(minmax=True).items():
                if v[0] and k.startswith("ndt_"):
                    phases[k] = min(phases.get(k, 1e30), v[2])     # the fastest launch of the phase
        ctx.profile_enable(0)
        ctx.profile_reset()
        bytes_per_launch = 16 * len(src) + 48 * r.n_hits
        ev_ms = phases.get("ndt_evaluate", float("nan"))
        print(json.dumps({"workload": name, "n_source": len(src), "n_target": len(tgt), "resolution": res, "steps": a.steps,
                          "iterations": r.iterations, "n_voxels": r.n_voxels, "n_hits": r.n_hits,
                          "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3), "device_ms": round(dev_med, 3),
                          "device_min_ms": round(dev_min, 3), "phases_ms": {k: round(v, 4) for k, v in sorted(phases.items())},
                          "evaluate": {"us_per_launch": round(ev_ms * 1e3, 2), "bytes_per_launch": bytes_per_launch,
                                       "roof_fraction": round(bytes_per_launch / (ev_ms * 1e-3) / ROOF_BYTES_PER_S, 4)}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
