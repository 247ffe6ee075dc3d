"""Mesh simplification (tc_simplify_clustering, include/threecrate_hip_simplify.h) timed: the whole call on both roads (numpy in: staging
included; torch device tensors in) and the stages alone from the library's events (tc_profile_read: `simplify_classes`,
`simplify_clusters`, `simplify_faces`, `simplify_write`), for synth.grid_mesh(side, side) at ratios 0.5 / 0.9 / 0.99 and both strategies.

With --ab: the meshes that bear on kSimplifyLongCluster -- a flat grid at ratios that give clusters of about 4, 16, 64, 256 and 1 024
members -- as the time of the cluster stage.  --cluster N loads the A/B build of the library with that threshold
(`make -C threecrate_amd/csrc simplify-ab`; 4294967295: every cluster on one lane) instead of the product.

    python tools/simplify_bench.py [--side 1000] [--reps 10] [--json out.json] [--cluster N] [--ab]
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
from threecrate_amd import _lib, synth  # noqa: E402

ROWS = ("simplify_classes", "simplify_clusters", "simplify_faces", "simplify_write")


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def measure(ctx, label, v, f, ratio, strategy, reps, whole=True):
    d_v, d_f = torch.from_numpy(v).to("cuda:0"), torch.from_numpy(f.view(np.int32)).to("cuda:0")
    out_v, out_f = ctx.simplify_mesh_clustering(d_v, d_f, ratio, strategy)
    row = dict(mesh=label, vertices=len(v), faces=len(f), ratio=ratio, strategy=strategy, out_vertices=int(out_v.shape[0]), out_faces=int(out_f.shape[0]))
    if whole:
        row["host_call_ms"] = round(timed(lambda: ctx.simplify_mesh_clustering(v, f, ratio, strategy), reps), 3)
        row["device_call_ms"] = round(timed(lambda: ctx.simplify_mesh_clustering(d_v, d_f, ratio, strategy), reps), 3)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(max(3, reps // 2)):
        ctx.simplify_mesh_clustering(d_v, d_f, ratio, strategy)
    torch.cuda.synchronize()
    stat = ctx.profile_read()
    ctx.profile_enable(False)
    for name in ROWS:
        if name in stat and stat[name][0]:
            row[name + "_us"] = round(stat[name][1] / stat[name][0] * 1e3, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    ap.add_argument("--cluster", type=int, help="load variants/libthreecrate_hip_simplify_cluster<N>.so instead of the product")
    ap.add_argument("--ab", action="store_true")
    a = ap.parse_args()
    if a.cluster is not None:
        _lib.load_companion("threecrate_hip_simplify.h", variant=f"libthreecrate_hip_simplify_cluster{a.cluster}.so")
    ctx = tc.GpuContext(0)
    rows = []
    if a.ab:
        v, f = synth.grid_mesh(a.side, a.side, 0.0)
        for members in (4, 16, 64, 256, 1024):
            # a flat unit lattice: cell^2 = members, so 1 - ratio = 1 / members
            rows.append(dict(measure(ctx, f"grid_{a.side}", v, f, 1.0 - 1.0 / members, "centroid", a.reps, whole=False), members=members, threshold=a.cluster))
    else:
        v, f = synth.grid_mesh(a.side, a.side, 0.5)
        for ratio in (0.5, 0.9, 0.99):
            for strategy in ("centroid", "weighted_average"):
                rows.append(measure(ctx, f"grid_{a.side}", v, f, ratio, strategy, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
