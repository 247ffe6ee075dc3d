#!/usr/bin/env python3
"""TSDF fusion and surface extraction: one JSON line per workload.

  host_ms / device_ms   steady-state integrate call through host images / through the _device entry point (torch tensors), median and
                        minimum of --iters calls after --warmup, device-synchronised
  counted_ms            the same _device call with count=True: the kernel's counting instantiation (one integer atomic per block on one
                        word) + the read-back of n_updated -- the A/B of that atomic
  extract_ms            whole extract_surface call into torch device arrays (the count call, then the points: two count passes, a scan
                        each, one fill pass, two read-backs, the scratch allocated and freed per call)
  kernels               time per launch from the library's own events (tc_profile_read), median and minimum over --iters profiled
                        calls: tsdf_integrate, tsdf_count, tsdf_fill; each next to the bytes of its model and their fraction of the
                        8 TB/s roof (the achievable streaming figure is about 6.3 TB/s = 0.79)
  models                integration: 16 B per updated voxel (one 8-byte load, one 8-byte store) + the depth image once;
                        extraction: 8 B per voxel per pass (corner re-reads are expected to hit in cache) + 15 B per point written

Workloads, on a --resolution^3 volume of 0.004 m voxels under a 640 x 480 camera: `full`, the camera on the axis far enough back that
every voxel is in view (n_updated == voxels proves it); `corner`, the camera moved aside so that it sees one corner only -- what the
wave-level skip is worth.  Run it several times for medians over fresh processes.

    python tools/tsdf_bench.py [--iters 10] [--warmup 3] [--resolution 512]
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

ROOF_BYTES_PER_S = 8e12
VOXEL = 0.004


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


def kernel_row(samples, nbytes):
    if not samples:
        return None
    med = statistics.median(samples)
    return {"ms_per_launch": round(med, 4), "min_ms": round(min(samples), 4), "model_bytes": int(nbytes),
            "roof_fraction": round(nbytes / (med * 1e-3) / ROOF_BYTES_PER_S, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resolution", type=int, default=512)
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    sync = torch.cuda.synchronize
    r = a.resolution
    side = r * VOXEL
    k = tc.CameraIntrinsics(525.0, 525.0, 319.5, 239.5, 640, 480)
    near = 1.1 * (side / 2) / (239.5 / 525.0)                   # the near face fills the image's height with a margin
    vol = ctx.tsdf_volume(VOXEL, 0.04, (r, r, r), (-side / 2, -side / 2, near))
    depth = np.full((480, 640), near + 0.4 * side, np.float32)      # a plane inside the volume
    d_depth = torch.from_numpy(depth).to("cuda:0")
    nvox = r ** 3
    for name, t in (("full", (0.0, 0.0, 0.0)), ("corner", (1.45 * side, 1.15 * side, 0.0))):
        pose = np.eye(4)
        pose[:3, 3] = t
        vol.reset()
        n_updated = vol.integrate(d_depth, k, camera_pose=pose, count=True)
        host_med, host_min = timed(lambda: vol.integrate(depth, k, camera_pose=pose), a.iters, a.warmup, sync)
        dev_med, dev_min = timed(lambda: vol.integrate(d_depth, k, camera_pose=pose), a.iters, a.warmup, sync)
        cnt_med, cnt_min = timed(lambda: vol.integrate(d_depth, k, camera_pose=pose, count=True), a.iters, a.warmup, sync)
        ext_med, ext_min = timed(lambda: vol.extract_surface(0.0, device="cuda:0"), a.iters, a.warmup, sync)
        ctx.profile_enable(1)
        samples = {"tsdf_integrate": [], "tsdf_count": [], "tsdf_fill": []}
        n_points = 0
        for _ in range(a.iters):
            ctx.profile_reset()
            vol.integrate(d_depth, k, camera_pose=pose)
            xyz, _ = vol.extract_surface(0.0, device="cuda:0")
            sync()
            n_points = len(xyz)
            for key, v in ctx.profile_read(minmax=True).items():
                if key in samples and v[0]:
                    samples[key].append(v[2])                   # (the count kernel runs twice per extract_surface: the faster launch)
        ctx.profile_enable(0)
        ctx.profile_reset()
        print(json.dumps({"workload": name, "resolution": r, "voxels": nvox, "state_bytes": 8 * nvox, "n_updated": n_updated,
                          "all_in_view": n_updated == nvox, "n_points": n_points,
                          "host_ms": round(host_med, 3), "host_min_ms": round(host_min, 3), "device_ms": round(dev_med, 3),
                          "device_min_ms": round(dev_min, 3), "counted_ms": round(cnt_med, 3), "counted_min_ms": round(cnt_min, 3),
                          "extract_ms": round(ext_med, 3), "extract_min_ms": round(ext_min, 3),
                          "kernels": {"tsdf_integrate": kernel_row(samples["tsdf_integrate"], 16 * n_updated + depth.nbytes),
                                      "tsdf_count": kernel_row(samples["tsdf_count"], 8 * nvox),
                                      "tsdf_fill": kernel_row(samples["tsdf_fill"], 8 * nvox + 15 * n_points)}}), flush=True)
    vol.close()
    ctx.close()


if __name__ == "__main__":
    main()
