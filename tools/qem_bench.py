"""Quadric-error simplification (tc_simplify_quadric, include/threecrate_hip_qem.h) timed on the device road (torch device tensors in): the
whole call, the number of rounds, and the rounds alone from the library's events (tc_profile_read: `qem_setup`, `qem_round`, `qem_write`)
as kernel ms per round, for synth.bumpy_grid_mesh(side, side) -- 10^6 vertices at the default side -- at ratios 0.5 and 0.9.

With --ab: the meshes that bear on kQemLongRing -- closed double cones whose two apexes have 64, 256, 1 024 and 4 096 faces, many of them in
one mesh -- as the time of the set-up stage, which holds the quadric fold.  --ring N loads the A/B build of the library with that threshold
(`make -C threecrate_amd/csrc qem-ab`; 4294967295: every ring on one lane) instead of the product.

    python tools/qem_bench.py [--side 1000] [--reps 5] [--json out.json] [--ring N] [--ab]
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

ROWS = ("qem_setup", "qem_round", "qem_write")


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


def cones(faces_per_apex, copies):
    """`copies` closed double cones side by side, each apex with faces_per_apex faces"""
    k = faces_per_apex
    a = np.arange(k) * (2 * np.pi / k)
    ring = np.stack([np.cos(a), np.sin(a), 0.05 * np.sin(3 * a)], axis=1)
    one_v = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, -0.7]], ring])
    i = np.arange(k)
    one_f = np.concatenate([np.stack([0 * i, 2 + i, 2 + (i + 1) % k], axis=1), np.stack([0 * i + 1, 2 + (i + 1) % k, 2 + i], axis=1)])
    v = np.concatenate([one_v + [3.0 * c, 0.0, 0.0] for c in range(copies)]).astype(np.float32)
    f = np.concatenate([one_f + c * len(one_v) for c in range(copies)]).astype(np.uint32)
    return v, f


def measure(ctx, label, v, f, ratio, reps, whole=True):
    d_v, d_f = torch.from_numpy(v).to("cuda:0"), torch.from_numpy(f.view(np.int32)).to("cuda:0")
    out_v, out_f = ctx.simplify_mesh_quadric(d_v, d_f, ratio)
    rounds = ctx.last_qem_rounds
    row = dict(mesh=label, vertices=len(v), faces=len(f), ratio=ratio, out_vertices=int(out_v.shape[0]), out_faces=int(out_f.shape[0]), rounds=rounds)
    if whole:
        row["device_call_ms"] = round(timed(lambda: ctx.simplify_mesh_quadric(d_v, d_f, ratio), reps), 3)
    ctx.profile_reset()
    ctx.profile_enable(True)
    calls = max(2, reps // 2)
    for _ in range(calls):
        ctx.simplify_mesh_quadric(d_v, d_f, ratio)
    torch.cuda.synchronize()
    stat = ctx.profile_read()
    ctx.profile_enable(False)
    for name in ROWS:
        if name in stat and stat[name][0]:
            row[name + "_ms_per_call"] = round(stat[name][1] / calls, 3)
    if "qem_round" in stat and stat["qem_round"][0]:
        row["kernel_ms_per_round"] = round(stat["qem_round"][1] / stat["qem_round"][0], 4)          # (the round that takes nothing counts as one)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json")
    ap.add_argument("--ring", type=int, help="load variants/libthreecrate_hip_qem_ring<N>.so instead of the product")
    ap.add_argument("--ab", action="store_true")
    a = ap.parse_args()
    if a.ring is not None:
        _lib.load_companion("threecrate_hip_qem.h", variant=f"libthreecrate_hip_qem_ring{a.ring}.so")
    ctx = tc.GpuContext(0)
    rows = []
    if a.ab:
        for per_apex in (64, 256, 1024, 4096):
            v, f = cones(per_apex, max(1, (1 << 20) // (2 * per_apex)))
            rows.append(dict(measure(ctx, f"cones_{per_apex}", v, f, 0.01, a.reps, whole=False), ring=per_apex, threshold=a.ring))
    else:
        v, f = synth.bumpy_grid_mesh(a.side, a.side, amplitude=0.05, waves=8.0)
        for ratio in (0.5, 0.9):
            rows.append(measure(ctx, f"field_{a.side}", v, f, ratio, a.reps))
    for r in rows:
        print(json.dumps(r))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
