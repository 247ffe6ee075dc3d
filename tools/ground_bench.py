"""Ground segmentation (tc_segment_ground / tc_segment_ground_device, include/threecrate_hip_ground.h) timed on synth.kitti_shaped_cloud()
(120 000 points) with the default configuration: milliseconds per call through host buffers and through device pointers, the split of
the kernel time among the key pass, the sort, the work lists, the fit and the compaction from the library's events (tc_profile_read: the
rows `ground_keys`, `ground_sort`, `ground_lists`, `ground_fit`, `ground_compact`), and the ground fraction.

    python tools/ground_bench.py [--reps 20] [--sensor-height 1.73] [--json out.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import threecrate_amd as tc  # noqa: E402
from threecrate_amd import synth  # noqa: E402

ROWS = ("ground_keys", "ground_sort", "ground_lists", "ground_fit", "ground_compact")


def timed(call, reps):
    call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sensor-height", type=float, default=1.73)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    points = synth.kitti_shaped_cloud()
    d = torch.from_numpy(points).to("cuda:0")
    cfg = tc.GpuContext.ground_config(a.sensor_height)
    r = ctx.segment_ground(points, config=cfg)
    status = np.bincount(r["patches"]["status"], minlength=9)
    row = dict(points=len(points), patches=len(r["patches"]), ground_fraction=round(float(r["labels"].mean()), 4),
               patches_by_status={name: int(c) for name, c in zip(tc._lib.TC_GROUND_STATUS, status)},
               largest_patch=int(r["patches"]["count"].max()),
               host_ms=round(timed(lambda: ctx.segment_ground(points, config=cfg), a.reps), 3),
               device_ms=round(timed(lambda: ctx.segment_ground(d, config=cfg), a.reps), 3),
               device_labels_only_ms=round(timed(lambda: ctx.segment_ground(d, config=cfg, return_index=False, return_patches=False), a.reps), 3))
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(a.reps):
        ctx.segment_ground(d, config=cfg)
    torch.cuda.synchronize()
    stat = ctx.profile_read()
    ctx.profile_enable(False)
    for name in ROWS:
        if name in stat:
            row[name + "_ms_per_call"] = round(stat[name][1] / a.reps, 4)
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(row, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
