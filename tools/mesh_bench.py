"""Mesh smoothing (tc_mesh_smooth, include/threecrate_hip_mesh.h) timed: the whole call on both roads (numpy in: staging included; torch
device tensors in) and the kernels alone from the library's events (tc_profile_read: `mesh_adjacency`, one row per kind of sweep,
`mesh_sweep_long`), for synth.grid_mesh(side, side) in row-major order and with the vertex indices randomly permuted (what locality is
worth to the gather), all three methods at the defaults; and a hub mesh: one vertex of a side x side grid joined to `--hub` others.
Next to each sweep: the model bytes -- per vertex 32 (its own 16-byte record in, one 16-byte record out) + 4 deg (the neighbour
indices) + 4 (the offset), every neighbour RECORD counted as a cache hit once the working set is streamed; HC's sweeps move one record
more (p in, or b out) and the model adds those 16 bytes -- and a device-to-device copy of as many bytes taken in the same process.

With --ab: only the meshes that bear on kMeshLongRing -- the hub, and `--fans` fans of one ring size each, for ring sizes either side
of the candidates -- as the time of one whole sweep (the one-lane launch + the long-ring launch).  --ring N loads the A/B build of the
library with that threshold (`make -C threecrate_amd/csrc mesh-ab`; 4294967295: every ring on one lane) instead of the product.

    python tools/mesh_bench.py [--side 1000] [--hub 100000] [--reps 20] [--json out.json] [--ring N] [--ab]
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

STREAM_BYTES_PER_S = 6.3e12
SWEEPS = {"laplacian": ["mesh_sweep_step"], "taubin": ["mesh_sweep_step"], "hc": ["mesh_sweep_hc_b", "mesh_sweep_hc_q"]}
EXTRA_RECORDS = {"mesh_sweep_step": 0, "mesh_sweep_hc_b": 2, "mesh_sweep_hc_q": 1}     # hc_b: p in, b out; hc_q: qbar in


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


def copy_us(nbytes, reps):
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0"), torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst.copy_(src)
    e0.record()
    for _ in range(reps):
        dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def measure(ctx, label, v, f, reps, rows):
    n = len(v)
    off, _ = ctx.mesh_adjacency(n, f)
    entries = int(off[-1])
    d_v, d_f = torch.from_numpy(v).to("cuda:0"), torch.from_numpy(f.view(np.int32)).to("cuda:0")
    for method, names in SWEEPS.items():
        host_ms = timed(lambda: ctx.smooth_mesh(v, f, method), reps)
        dev_ms = timed(lambda: ctx.smooth_mesh(d_v, d_f, method), reps)
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(max(3, reps // 4)):
            ctx.smooth_mesh(d_v, d_f, method)
        torch.cuda.synchronize()
        stat = ctx.profile_read(minmax=True)
        ctx.profile_enable(False)
        row = dict(mesh=label, vertices=n, faces=len(f), entries=entries, method=method, host_call_ms=round(host_ms, 3), device_call_ms=round(dev_ms, 3),
                   adjacency_us=round(stat["mesh_adjacency"][1] / stat["mesh_adjacency"][0] * 1e3, 1))
        if "mesh_sweep_long" in stat and stat["mesh_sweep_long"][0]:
            row["sweep_long_us"] = round(stat["mesh_sweep_long"][1] / stat["mesh_sweep_long"][0] * 1e3, 1)
        for name in names:
            us = stat[name][1] / stat[name][0] * 1e3
            model = n * (32 + 4 + 16 * EXTRA_RECORDS[name]) + 4 * entries
            row[name] = dict(kernel_us=round(us, 1), model_bytes=model, stream_fraction=round(model / (us * 1e-6) / STREAM_BYTES_PER_S, 3),
                             d2d_copy_us=round(copy_us(model, reps), 1))
        rows.append(row)
        print(json.dumps(row), flush=True)


def hub_mesh(side, hub):
    """vertex 0 of a side x side grid joined to `hub` other vertices by a fan of faces (0, k, k + 1)"""
    v, f = synth.grid_mesh(side, side, 0.5, seed=2)
    ring = min(hub, len(v) - 2)
    k = np.arange(1, ring, dtype=np.uint32)
    return ring, v, np.concatenate([f, np.stack([np.zeros_like(k), k, k + 1], axis=1)])


def fans_mesh(count, ring):
    """`count` closed fans of `ring` rim vertices each, one behind the other: hub c * (ring + 1), its rim behind it"""
    base = (np.arange(count, dtype=np.uint32) * np.uint32(ring + 1))[:, None]
    k = np.arange(ring, dtype=np.uint32)[None, :]
    f = np.stack([np.broadcast_to(base, (count, ring)), base + 1 + k, base + 1 + (k + 1) % ring], axis=2).reshape(-1, 3)
    return synth.uniform_cloud(count * (ring + 1), seed=ring), np.ascontiguousarray(f, np.uint32)


def sweep_us(ctx, v, f, reps):
    """one whole Laplacian sweep: the one-lane launch + the long-ring launch, per launch from the library's events"""
    d_v, d_f = torch.from_numpy(v).to("cuda:0"), torch.from_numpy(f.view(np.int32)).to("cuda:0")
    ctx.smooth_mesh(d_v, d_f, "laplacian")
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(max(3, reps // 4)):
        ctx.smooth_mesh(d_v, d_f, "laplacian")
    torch.cuda.synchronize()
    stat = ctx.profile_read(minmax=True)
    ctx.profile_enable(False)
    per = lambda name: stat[name][1] / stat[name][0] * 1e3 if name in stat and stat[name][0] else 0.0
    return per("mesh_sweep_step"), per("mesh_sweep_long")


def ab(ctx, a, rows):
    ring, hv, hf = hub_mesh(a.hub_side, a.hub)
    meshes = [(f"hub ring {ring}", hv, hf)] + [(f"{a.fans} fans of ring {r}", *fans_mesh(a.fans, r)) for r in (12, 24, 48, 96, 192, 384, 1024)]
    for label, v, f in meshes:
        one, long_ = sweep_us(ctx, v, f, a.reps)
        row = dict(threshold=a.ring, mesh=label, vertices=len(v), one_lane_us=round(one, 1), long_us=round(long_, 1), sweep_us=round(one + long_, 1))
        rows.append(row)
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--hub", type=int, default=100_000)
    ap.add_argument("--hub-side", type=int, default=317)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--ring", type=int, help="load variants/libthreecrate_hip_mesh_ring<N>.so instead of the product's mesh library")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--fans", type=int, default=2000)
    a = ap.parse_args()
    if a.ring is not None:
        _lib.load_companion("threecrate_hip_mesh.h", variant=f"libthreecrate_hip_mesh_ring{a.ring}.so")
    ctx = tc.GpuContext(0)
    rows = []
    if a.ab:
        ab(ctx, a, rows)
        if a.json:
            with open(a.json, "w") as fh:
                json.dump(dict(ring=a.ring, rows=rows), fh, indent=1)
        ctx.close()
        return
    v, f = synth.grid_mesh(a.side, a.side, 0.5, seed=1)
    measure(ctx, "row-major", v, f, a.reps, rows)
    perm = np.random.default_rng(0).permutation(len(v)).astype(np.uint32)       # old index -> new index
    pv = np.empty_like(v)
    pv[perm] = v
    measure(ctx, "permuted", pv, perm[f], a.reps, rows)
    ring, hv, hf = hub_mesh(a.hub_side, a.hub)
    measure(ctx, f"hub ring {ring}", hv, hf, a.reps, rows)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(side=a.side, hub=a.hub, reps=a.reps, rows=rows), fh, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
