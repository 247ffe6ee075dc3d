#!/usr/bin/env python3
"""Poisson reconstruction's field (tc_poisson_field_device, include/threecrate_hip_poisson.h): one JSON line per workload and depth, on a
200 k-point sphere and tools/shot_bench.py's clouds (their normals from estimate_normals), at depth 6, 7 and 8.

  device_ms        the whole field call through the _device entry point (torch tensors), median of --iters calls after --warmup
  iterations       the loop's iterations of that call
  iteration_us     (poisson_stencil + poisson_update kernel time) / iterations, from one profiled call (tc_profile_read): the launched
                   rounds after the stop return at once and count as no iteration.  The two one-block fold launches of a round and
                   the gaps between launches are not in it: what a round costs on the stream is (device_ms - the other phases) / iterations
  achieved_TBps    the two passes' minimum traffic, 10 arrays of 4 N^3 bytes an iteration (stencil: r, p in, p', q out; update: p', q,
                   chi, r in, chi, r out), 11 with --point-weight > 0 (the stencil then reads the density), over iteration_us;
                   hbm_share = that over the 6.3 TB/s a copy achieves on the MI355X.  At depth 6 the arrays fit the caches
  phases_ms        every profile row of that call

    python tools/poisson_bench.py [--iters 5] [--warmup 2] [--only name,...] [--depths 6,7,8] [--max-iterations 200] [--point-weight 0]
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

HBM_ACHIEVABLE_TBPS = 6.3


def sphere(n):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1).astype(np.float32)
    return (0.5 * d).astype(np.float32), d


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
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    ap.add_argument("--depths", default="6,7,8")
    ap.add_argument("--max-iterations", type=int, default=200)
    ap.add_argument("--point-weight", type=float, default=0.0)
    a = ap.parse_args()
    ctx = tc.GpuContext(0)

    def with_normals(make):
        c6 = np.ascontiguousarray(ctx.estimate_normals(np.ascontiguousarray(make(), np.float32), 10), np.float32)
        return np.ascontiguousarray(c6[:, :3]), np.ascontiguousarray(c6[:, 3:])

    work = [("sphere_200k", lambda: sphere(200000)), ("kitti_shaped", lambda: with_normals(synth.kitti_shaped_cloud)),
            ("uniform_100k", lambda: with_normals(lambda: synth.uniform_cloud(10**5)))]
    if a.only:
        keep = set(a.only.split(","))
        work = [w for w in work if w[0] in keep]
    sync = torch.cuda.synchronize
    for name, make in work:
        p, q = make()
        P, Q = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(q).to("cuda:0")
        for depth in (int(d) for d in a.depths.split(",")):
            cfg = {"depth": depth, "max_iterations": a.max_iterations, "point_weight": a.point_weight}
            call = lambda: ctx.poisson_field(P, Q, cfg, want_density=False)
            dev_ms = timed(call, a.iters, a.warmup, sync)
            ctx.profile_enable(1)
            ctx.profile_reset()
            out = call()
            sync()
            rows = {k: v for k, v in ctx.profile_read().items() if v[0]}
            ctx.profile_enable(0)
            ctx.profile_reset()
            rounds = rows["poisson_stencil"][0]
            it_us = (rows["poisson_stencil"][1] + rows["poisson_update"][1]) / max(out["iterations"], 1) * 1e3
            arrays = 10 + (1 if a.point_weight > 0 else 0)
            tbps = arrays * 4 * (1 << (3 * depth)) / (it_us * 1e-6) / 1e12
            print(json.dumps({"workload": name, "n": len(p), "depth": depth, "device_ms": round(dev_ms, 3), "iterations": out["iterations"],
                              "launched_rounds": rounds, "rel_residual": out["rel_residual"], "iteration_us": round(it_us, 2),
                              "achieved_TBps": round(tbps, 3), "hbm_share": round(tbps / HBM_ACHIEVABLE_TBPS, 3),
                              "phases_ms": {k: round(v[1], 4) for k, v in rows.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
