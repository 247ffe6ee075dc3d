"""Marching cubes (tc_marching_cubes, include/threecrate_hip_mc.h) timed on the device road: the Python call (two library calls: the counts,
then the mesh) and the stages alone from the library's events (tc_profile_read: `mc_classify`, `mc_edge_flags`, `mc_scan`, `mc_emit`), for
the res^3 sphere of synth.sphere_volume (z-fastest, no mask) and for a res^3 TSDF-shaped volume (x-fastest, a truncated plane distance,
a weight mask on three quarters of it), welded and unwelded, with and without normals.  Beside each figure the plain estimate: the volume
read once plus the outputs written, at the HBM rate DESIGN.md uses.

    python tools/mc_bench.py [--res 256] [--reps 10] [--json out.json]
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

ROWS = ("mc_classify", "mc_edge_flags", "mc_scan", "mc_emit")
HBM_GBPS = 8000.0       # the MI355X's HBM3E rate, as in DESIGN.md's rooflines


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def measure(ctx, label, values, dims, vs, org, valid, layout, weld, normals, reps):
    d_v = torch.from_numpy(values).to("cuda:0")
    d_m = None if valid is None else torch.from_numpy(valid).to("cuda:0")
    call = lambda: ctx.marching_cubes(d_v, dims, vs, org, 0.0, normals, weld, d_m, layout)
    v, n, f = call()
    row = dict(volume=label, voxels=int(values.size), weld=weld, normals=normals, vertices=int(v.shape[0]), faces=int(f.shape[0]))
    row["device_call_ms"], row["device_call_min_ms"], row["device_call_max_ms"] = (round(x, 3) for x in timed(call, reps))
    ctx.profile_reset()
    ctx.profile_enable(True)
    k = max(3, reps // 2)
    for _ in range(k):
        call()
    torch.cuda.synchronize()
    stat = ctx.profile_read()
    ctx.profile_enable(False)
    for name in ROWS:
        if name in stat and stat[name][0]:
            row[name + "_us"] = round(stat[name][1] / stat[name][0] * 1e3, 1)
    # one library call of the two: classify + flags + scan; the second adds the emit stage
    row["kernels_one_pass_us"] = round(sum(row.get(r + "_us", 0.0) for r in ROWS), 1)
    bytes_moved = values.size * (4 + (1 if valid is not None else 0)) + v.shape[0] * 12 * (2 if normals else 1) + f.shape[0] * 12
    row["estimate_us"] = round(bytes_moved / (HBM_GBPS * 1e3), 1)
    row["fraction_of_estimate"] = round(row["estimate_us"] / row["kernels_one_pass_us"], 3) if row["kernels_one_pass_us"] else None
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    res = a.res
    rows = []
    sv, svs, sorg = synth.sphere_volume((0.0, 0.0, 0.0), 1.0, (res,) * 3, (3.0, 3.0, 3.0))
    z, y, x = np.meshgrid(*[np.arange(res, dtype=np.float32)] * 3, indexing="ij")
    vs = np.float32(3.0 / (res - 1))
    tsdf = np.clip(((np.float32(0.3) * x + np.float32(0.2) * y + z) * vs - np.float32(2.0)) / (np.float32(4.0) * vs), -1, 1).astype(np.float32)
    weight = (x < 3 * res // 4).astype(np.uint8)
    for weld in (False, True):
        for normals in (False, True):
            rows.append(measure(ctx, f"sphere_{res}", np.ascontiguousarray(sv).reshape(-1), (res,) * 3, svs, sorg, None, "z_fastest", weld, normals, a.reps))
            rows.append(measure(ctx, f"tsdf_{res}", tsdf.reshape(-1), (res,) * 3, (float(vs),) * 3, (0.0, 0.0, 0.0), weight.reshape(-1), "x_fastest", weld,
                                normals, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
