#!/usr/bin/env python3
"""Streaming voxel map: one JSON line per voxel size.

  insert_device_ms / insert_host_ms   whole tc_voxel_map_insert(_device) call per frame over --frames KITTI-shaped frames (synth's 120 k-point
                        frame, a forward ego-motion of 1 m and a yaw of 0.01 rad per frame applied), median and minimum, device-synchronised
  extract_ms            one whole extract call at the end (the count call, then keys, counts, sums and centroids into host arrays)
  kernels               time per launch from the library's own events (tc_profile_read) over a second, profiled pass of the same frames:
                        voxel_map_sort (key kernel + radix sort + run detection + long-run list), voxel_map_insert, voxel_map_insert_long,
                        voxel_map_rehash, voxel_map_extract
  yardstick_ms          tc_voxel_grid_filter_device on ONE frame of the same sequence (median and minimum over the first 20 frames): the
                        single-shot filter the map cannot be replaced by, as the nearest existing cost.  With --yardstick-lib PATH (another
                        build of libthreecrate_hip.so, the parent commit's say) it is measured in a child process that loads THAT library
                        through TC_HIP_LIB, in the same session; yardstick_lib in the row says which library ran.  Without the option it is
                        the library under test -- the same figure as long as voxel.hip's device assembly is the parent's.
  voxels, points        the map's final size and the points inserted

    python tools/voxelmap_bench.py [--frames 100] [--voxel-sizes 0.5 1.0] [--yardstick-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: see tests/conftest.py)
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import synth  # noqa: E402


def frames(count):
    """the same scan seen from a moving vehicle: frame f in world coordinates"""
    base = synth.kitti_shaped_cloud(seed=0).astype(np.float64)
    out = []
    for f in range(count):
        a = 0.01 * f
        c, s = np.cos(a), np.sin(a)
        r = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        out.append(np.ascontiguousarray((base @ r.T + np.array([1.0 * f, 0.0, 0.0])).astype(np.float32)))
    return out


def timed_inserts(m, chunks, sync):
    ts = []
    for ch in chunks:
        sync()
        t0 = time.perf_counter()
        m.insert(ch)
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4), round(min(ts), 4)


def yardstick(ctx, dev, vs, sync):
    """the single-shot voxel filter on one frame, through the _device entry point: median and minimum over the frames given"""
    ctx.voxel_grid_filter(dev[0], vs)
    ys = []
    for f in dev:
        sync()
        t0 = time.perf_counter()
        ctx.voxel_grid_filter(f, vs)
        sync()
        ys.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ys), 4), round(min(ys), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--voxel-sizes", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--yardstick-lib", default=None, help="another build of libthreecrate_hip.so for the yardstick (a child process loads it)")
    ap.add_argument("--yardstick-only", action="store_true", help="print {voxel size: yardstick} of the loaded library and leave")
    args = ap.parse_args()
    ctx = tc.GpuContext(0)
    sync = torch.cuda.synchronize
    if args.yardstick_only:
        dev = [torch.from_numpy(f).to("cuda:0") for f in frames(20)]
        print(json.dumps({str(vs): yardstick(ctx, dev, vs, sync) for vs in args.voxel_sizes}), flush=True)
        ctx.close()
        return
    other = None
    if args.yardstick_lib:          # before this process has much on the device; a fresh child, its own library
        out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--yardstick-only", "--voxel-sizes"] + [str(v) for v in args.voxel_sizes],
                                      env=dict(os.environ, TC_HIP_LIB=os.path.abspath(args.yardstick_lib)), text=True, timeout=240)
        other = json.loads(out.strip().splitlines()[-1])
    host = frames(args.frames)
    dev = [torch.from_numpy(f).to("cuda:0") for f in host]
    sync()
    for vs in args.voxel_sizes:
        row = {"voxel_size": vs, "frames": args.frames, "points_per_frame": len(host[0])}
        warm = ctx.voxel_map(vs)
        warm.insert(dev[0])
        warm.insert(host[0])
        warm.close()
        m = ctx.voxel_map(vs)
        row["insert_device_ms"] = timed_inserts(m, dev, sync)
        row["voxels"], row["points"] = len(m), m.points_inserted
        t0 = time.perf_counter()
        m.extract(keys=True, counts=True, sums=True)
        row["extract_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        m.reset()
        row["insert_host_ms"] = timed_inserts(m, host, sync)
        m.reset()
        ctx.profile_enable(True)
        ctx.profile_reset()
        for f in dev:
            m.insert(f)
        m.extract()
        row["kernels"] = {k: {"launches": v[0], "ms_per_launch": round(v[1] / max(v[0], 1), 4), "min_ms": round(v[2], 4), "max_ms": round(v[3], 4)}
                          for k, v in ctx.profile_read(minmax=True).items() if k.startswith("voxel_map") and v[0]}
        ctx.profile_enable(False)
        m.close()
        row["yardstick_ms"] = tuple(other[str(vs)]) if other else yardstick(ctx, dev[:20], vs, sync)
        row["yardstick_lib"] = args.yardstick_lib if other else "the library under test"
        print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
