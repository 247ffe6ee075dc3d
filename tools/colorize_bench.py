"""Colorization (tc_colorize, include/threecrate_hip_color.h) timed: the whole call on both roads (numpy in: staging included; torch
device tensors in) and the kernel alone from the library's events (tc_profile_read, rows `colorize` / `colorize_counted`), for n points of synth.uniform_cloud
in front of one and of six 640 x 480 cameras; bilinear and nearest; with and without the count; with and without depth images.  Next to
each kernel time: the model bytes (12 in + 3 out [+ 4 index] per point + the texels and depths touched), the fraction of the 6.3 TB/s
streaming rate STATE.md uses, and a device-to-device copy of the same number of bytes taken in the same process.

    python tools/colorize_bench.py [--points 1000000] [--reps 20] [--json out.json]
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

W, H, FOCAL, STREAM_BYTES_PER_S = 640, 480, 400.0, 6.3e12


def cameras(k, rng):
    """k cameras on a ring around the unit cube's centre, 2.5 away, looking at it: (image, intrinsics, world_to_camera, depth)"""
    out = []
    for s in range(k):
        a = 2 * np.pi * s / max(k, 1)
        eye = np.array([0.5 + 2.5 * np.sin(a), 0.5, 0.5 - 2.5 * np.cos(a)])
        fwd = (np.array([0.5, 0.5, 0.5]) - eye) / 2.5
        right = np.cross([0.0, 1.0, 0.0], fwd)
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        rot = np.stack([right, down, fwd])
        m = np.concatenate([rot, (-rot @ eye)[:, None]], axis=1).astype(np.float32)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        depth = np.full((H, W), 2.5, np.float32)                # with a tolerance of 1: every point of the cube passes
        out.append((img, (FOCAL, FOCAL, W / 2, H / 2), m, depth))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json")
    a = ap.parse_args()
    ctx = tc.GpuContext(0)
    rng = np.random.default_rng(0)
    xyz = synth.uniform_cloud(a.points, seed=1)
    d_xyz = torch.from_numpy(xyz).to("cuda:0")
    rows = []
    for k in (1, 6):
        cams = cameras(k, rng)
        d_cams = [(torch.from_numpy(i).to("cuda:0"), kk, m, torch.from_numpy(d).to("cuda:0")) for i, kk, m, d in cams]
        for mode in ("bilinear", "nearest"):
            for count in (False, True):
                for depth in (False, True):
                    for index in (False, True):
                        pick = lambda cs: [c if depth else c[:3] for c in cs]
                        kw = dict(interpolation=mode, count=count, return_index=index, depth_tolerance=1.0)
                        host_ms = timed(lambda: ctx.colorize(xyz, pick(cams), **kw), max(3, a.reps // 4))
                        dev_ms = timed(lambda: ctx.colorize(d_xyz, pick(d_cams), **kw), a.reps)
                        ctx.profile_reset()
                        ctx.profile_enable(True)
                        for _ in range(a.reps):
                            ctx.colorize(d_xyz, pick(d_cams), **kw)
                        torch.cuda.synchronize()
                        stat = ctx.profile_read(minmax=True)["colorize_counted" if count else "colorize"]
                        ctx.profile_enable(False)
                        kernel_us = stat[1] / stat[0] * 1e3
                        texels = (12 if mode == "bilinear" else 3) + (4 if depth else 0)
                        model = a.points * (15 + (4 if index else 0) + texels)
                        src, dst = torch.empty(model, dtype=torch.uint8, device="cuda:0"), torch.empty(model, dtype=torch.uint8, device="cuda:0")
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        dst.copy_(src)
                        e0.record()
                        for _ in range(a.reps):
                            dst.copy_(src)
                        e1.record()
                        torch.cuda.synchronize()
                        copy_us = e0.elapsed_time(e1) / a.reps * 1e3
                        row = dict(cameras=k, mode=mode, count=count, depth=depth, index=index, host_call_ms=round(host_ms, 3), device_call_ms=round(dev_ms, 3),
                                   kernel_us=round(kernel_us, 2), model_bytes=model, stream_fraction=round(model / (kernel_us * 1e-6) / STREAM_BYTES_PER_S, 3),
                                   d2d_copy_us=round(copy_us, 2))
                        rows.append(row)
                        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(dict(points=a.points, reps=a.reps, rows=rows), f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
