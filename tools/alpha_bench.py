"""Alpha-shape reconstruction (tc_alpha_shape_device, include/threecrate_hip_alpha.h) timed on the device road with the cap lifted
(max_triangles = 0): the whole call (the counts call and the faces call of GpuContext.alpha_shape together), the candidates, and the
split of the kernel time among index, lists, triples, edges and write-out from the library's events (tc_profile_read: the rows
`alpha_lists`, `alpha_triples`, `alpha_edges`, `alpha_write`; every other row of the call is the index build).  The triples tested are
counted on the host from an f64 k-d tree (the pairs j > i within alpha per point): a figure for the rate, not for the result.
Clouds: synth.sphere_cloud (random order) and the vertices of synth.bumpy_grid_mesh (row order), alpha = --spacings mean spacings.
--small adds the time of the numpy restatement (tests/alpha_checker.py) on a 700-point sphere next to the device's, for scale.

    python tools/alpha_bench.py [--points 100000 1000000] [--spacings 2.5] [--reps 3] [--small] [--json out.json]
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

ROWS = ("alpha_lists", "alpha_triples", "alpha_edges", "alpha_write")


def triples_tested(points, alpha):
    from scipy.spatial import cKDTree
    pairs = cKDTree(points.astype(np.float64)).query_pairs(float(alpha), output_type="ndarray")           # i < j
    m = np.bincount(pairs[:, 0], minlength=len(points)).astype(np.int64)
    return int(len(pairs)), int((m * (m - 1) // 2).sum())


def measure(ctx, label, points, alpha, reps):
    d = torch.from_numpy(points).to("cuda:0")
    call = lambda: ctx.alpha_shape(d, alpha, mode="boundary", max_triangles=0, return_stats=True)
    faces, stats = call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    stat = ctx.profile_read()
    ctx.profile_enable(False)
    calls = 2 * reps                                            # alpha_shape calls the library twice: the counts, then the faces
    pairs, triples = triples_tested(points, alpha)
    row = dict(cloud=label, points=len(points), alpha=round(float(alpha), 6), pairs=pairs, triples=triples, candidates=stats["candidates"],
               faces=stats["faces"], two_calls_ms=round(float(np.median(t)), 3))
    split = {name: stat[name][1] / calls for name in ROWS if name in stat}
    split["index"] = sum(v[1] for k, v in stat.items() if k not in ROWS) / calls
    for name, ms in split.items():
        row[name + "_ms_per_call"] = round(ms, 3)
    if split.get("alpha_triples"):
        # a library call enumerates the triples twice (the count pass and the emit pass)
        row["triples_tested_per_s"] = float(f"{2 * triples / (split['alpha_triples'] * 1e-3):.4g}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--spacings", type=float, default=2.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    rows = []
    for n in a.points:
        rows.append(measure(ctx, "sphere", synth.sphere_cloud(n), a.spacings * np.sqrt(4 * np.pi / n), a.reps))
        print(json.dumps(rows[-1]), flush=True)
        side = int(round(np.sqrt(n)))
        v, _ = synth.bumpy_grid_mesh(side, side, amplitude=0.05, waves=8.0)
        spacing = float(np.linalg.norm(v[1] - v[0]))
        rows.append(measure(ctx, "bumpy_grid", np.ascontiguousarray(v, np.float32), a.spacings * spacing, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    if a.small:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from tests import alpha_checker as K
        p = synth.sphere_cloud(700)
        t0 = time.perf_counter()
        want = K.alpha_shape(p, 0.6, K.BOUNDARY, 1e-8, 0)
        checker_ms = (time.perf_counter() - t0) * 1e3
        row = measure(ctx, "sphere_small", p, 0.6, a.reps)
        row["checker_ms"] = round(checker_ms, 1)
        row["equal_to_checker"] = bool(row["candidates"] == want["candidates"] and row["faces"] == want["n_faces"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
