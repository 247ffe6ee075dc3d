"""The calls that share regions of a context's pinned host block leave each other alone (tc_internal.h: PinnedBlock).

One word of the block is the first chunk flag of the ICP loop AND the count word of the voxel filter, of cluster extraction and of
FPFH; the registrations stage their initial state in one IcpState slot and read their result from another.  The suite shares one
session context, but no other test states that a call's result does not depend on what the context ran before it.  Here seven calls
run in a row on ONE context, and each result is compared, bit for bit, with the same call made alone on a fresh context.

Inputs: two disjoint random subsets, 2 000 points each, of one synth.tum_shaped_cloud surface (100 x 80 samples), the source moved by a
small isometry.  2 000 points keep the small-source exact-sums kernel in play; 20 iterations with threshold 0 (the unchecked entry
point accepts it) never converge, so the loop runs all of its chunks 6, 2, 4, 4, 4 and the host polls flags 0..2 -- the smallest call
that reaches the flag polling."""
import numpy as np
import pytest

import threecrate_amd as tc
from threecrate_amd import synth

pytestmark = pytest.mark.gpu

N = 2000
ITERS = 20


def _inputs():
    surface = synth.tum_shaped_cloud(width=100, height=80, seed=3)
    order = np.argsort(synth.splitmix_u01(17, np.arange(len(surface), dtype=np.uint64)), kind="stable")
    tgt = np.ascontiguousarray(surface[order[:N]])
    offset = synth.yaw_isometry((0.02, -0.015, 0.01), 0.03)
    src = np.ascontiguousarray(synth.apply_isometry(offset, surface[order[N:2 * N]]))
    return src, tgt


def _registration(r):
    return [np.asarray(r.transformation), np.float32(r.mse), np.int64(r.iterations), np.asarray(r.corr_target)]


def _steps(src, tgt):
    """name -> call(ctx, normals of step 5 or None) -> list of arrays"""
    p2p = lambda c, _: _registration(c.icp_detailed(src, tgt, None, ITERS, None, 0.0))
    return [
        ("voxel_grid_filter", lambda c, _: [np.asarray(c.voxel_grid_filter(tgt, 0.1))]),
        ("icp_detailed", p2p),
        ("extract_euclidean_clusters_labels", lambda c, _: [np.asarray(a) for a in c.extract_euclidean_clusters_labels(tgt, 0.08, 5, N)]),
        ("extract_fpfh_features", lambda c, _: [np.asarray(c.extract_fpfh_features(tgt, 0.1, 10))]),
        ("estimate_normals", lambda c, _: [np.asarray(c.estimate_normals(tgt, 16))]),
        ("icp_point_to_plane_detailed", lambda c, nrm: _registration(c.icp_point_to_plane_detailed(src, tgt, nrm, None, ITERS, None, 0.0))),
        ("icp_detailed again", p2p),
    ]


def test_calls_sharing_the_pinned_block_give_the_results_they_give_alone():
    src, tgt = _inputs()
    assert src.shape == tgt.shape == (N, 3)
    steps = _steps(src, tgt)
    ctx = tc.GpuContext(0)
    try:
        together, normals = [], None
        for name, call in steps:
            together.append(call(ctx, normals))
            if name == "estimate_normals":
                normals = together[-1][0]
    finally:
        ctx.close()
    assert together[1][2] == ITERS and together[5][2] == ITERS          # every chunk ran: flags 0..2 were polled
    assert together[0][0].shape[0] > 1 and together[2][2].shape[0] > 1  # several voxels, at least one cluster: the count word carried a number
    for (name, call), got in zip(steps, together):
        fresh = tc.GpuContext(0)
        try:
            alone = call(fresh, normals)
        finally:
            fresh.close()
        assert len(alone) == len(got)
        for k, (a, b) in enumerate(zip(alone, got)):
            assert np.array_equal(a, b), f"{name}: output {k} differs from the same call on a fresh context"
    for k, (a, b) in enumerate(zip(together[1], together[6])):
        assert np.array_equal(a, b), f"icp_detailed: output {k} of the second run differs from the first"
