"""The steps the voxel filter's sort path, the NDT voxel map and cluster extraction share (csrc/grid.hip: sort_pairs, key_runs), at the
sizes where they can go wrong: runs of 9, 96, 97 (either side of voxel.hip's kLongVoxel) and 300 points (a run across two 256-thread
blocks), n around one block (256), one scan tile (2048) and two (4097), 1 / 255 / 256 / 257 / 2049 runs, the two-level scan, and a
member sort whose unlabelled points carry the key behind the last cluster.  The wave road of the voxel filter (csrc/run_fold.h:
fold_run_wave, 64 points per trip) also gets runs of 192, 193, 256, 257 and 4097 points -- a last trip of exactly 64 points and of one --
a cloud of five long voxels among forty short ones, and one of 4 100 long voxels: more than the wave kernel's grid has waves, so
that they stride over the list of long runs (csrc/run_fold.h: for_each_listed_run).

Inputs: points on a line along x (y = z = 0), voxel v = [v * EDGE, (v + 1) * EDGE) with EDGE a power of two, the first point at x = 0
exactly (the voxel filter's keys are relative to the box's minimum) and every other point 0.1 .. 0.9 of an edge into its voxel, in
shuffled order.  Every input has a twin without the `gpu` mark that proves on the oracle / the checkers alone that it has the runs it
is meant to have.  References: the oracle for the voxel filter (bit equality), tests/ndt_checker.py with the budgets of
tests/test_gpu_ndt.py for the voxel map, tests/cluster_checker.py for the clusters (equality)."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import cluster_checker as K
from tests import ndt_checker as NC

F = np.float32
EDGE = 0.5
LONG_VOXEL = 96         # kLongVoxel of csrc/voxel.hip: voxels of more points get a wave each
SIZES = (255, 256, 257, 2047, 2048, 2049, 4097)
WAVE_LENGTHS = (192, 193, 256, 257, 4097)   # all above LONG_VOXEL: always a wave; the last trip has 64, 1, 64, 1 and 1 points


@functools.lru_cache(maxsize=None)
def line_cloud(m, runs, alternate=False):
    """`runs` consecutive voxels along x of m points each (alternate: m, m - 1, m, ...), shuffled with a fixed seed"""
    return cloud_of(tuple(m - (v % 2 if alternate else 0) for v in range(runs)), 1000 * m + runs)


@functools.lru_cache(maxsize=None)
def mixed_cloud(m):
    """45 consecutive voxels: voxels 4, 13, 22, 31 and 40 have m points, the forty others 9"""
    return cloud_of(tuple(m if v % 9 == 4 else 9 for v in range(45)), 77 * m)


def cloud_of(counts, seed):
    rng = np.random.default_rng(seed)
    x = np.concatenate([(v + rng.uniform(0.1, 0.9, c)) * EDGE for v, c in enumerate(counts)])
    x[0] = 0.0
    cloud = np.zeros((len(x), 3), F)
    cloud[:, 0] = rng.permutation(x)
    cloud.setflags(write=False)
    return cloud


def voxel_cases():
    """(m, V): n = m V takes every size of SIZES where m divides it, else the multiples of m either side; and V = 1, 2"""
    out = []
    for m in (9, LONG_VOXEL, LONG_VOXEL + 1, 300):
        vs = {1, 2}
        for n in SIZES:
            vs |= {n // m} if n % m == 0 else {n // m, n // m + 1}
        out += [(m, v) for v in sorted(vs - {0})]
    # (the last: more long voxels than the wave kernel's 1 024 blocks have waves, so its waves stride over their list)
    return out + [(m, v) for m in WAVE_LENGTHS for v in (1, 2)] + [(LONG_VOXEL + 1, 4 * 1024 + 4)]


@functools.lru_cache(maxsize=None)
def voxel_reference(m, v):
    return O.voxel_grid_filter(line_cloud(m, v), EDGE)


def sorted_path_call(ctx, cloud):
    """the filter's result, after asserting that the sort path served it, once"""
    ctx.profile_enable(1)
    ctx.profile_reset()
    try:
        out = ctx.voxel_grid_filter(cloud, EDGE)
        rows = ctx.profile_read()
    finally:
        ctx.profile_enable(0)
    assert rows["voxel_grid_filter_sorted"][0] == 1 and rows.get("voxel_grid_filter", (0, 0))[0] == 0, rows
    return out


@functools.lru_cache(maxsize=None)
def mixed_reference(m):
    return O.voxel_grid_filter(mixed_cloud(m), EDGE)


def check_voxel_filter(ctx, m, v, mixed=False):
    cloud, ref = (mixed_cloud(m), mixed_reference(m)) if mixed else (line_cloud(m, v), voxel_reference(m, v))
    assert len(cloud) > 8 * v                                   # more than 8 points per voxel of the box: the sort path
    host = sorted_path_call(ctx, cloud)
    assert host.shape == ref.shape and np.array_equal(host.view(np.uint32), ref.view(np.uint32))
    dev = sorted_path_call(ctx, torch.from_numpy(np.array(cloud)).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ---- voxel filter, sort path ----
@pytest.mark.parametrize("m,v", voxel_cases())
def test_line_cloud_has_v_voxels_of_m_points(m, v):
    cloud, ref = line_cloud(m, v), voxel_reference(m, v)
    keys = np.floor((cloud[:, 0] - cloud[:, 0].min()) / F(EDGE)).astype(np.int64)
    assert cloud.dtype == F and cloud[:, 0].min() == 0 and np.array_equal(np.bincount(keys), np.full(v, m))
    assert ref.shape == (v, 3) and np.array_equal(np.floor(ref[:, 0] / F(EDGE)), np.arange(v)) and not ref[:, 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("m,v", voxel_cases())
def test_voxel_filter_sort_path_at_run_and_tile_boundaries(ctx, m, v):
    check_voxel_filter(ctx, m, v)


@pytest.mark.parametrize("m", [193, 256])
def test_mixed_cloud_has_five_long_voxels_among_forty_short_ones(m):
    cloud, ref = mixed_cloud(m), mixed_reference(m)
    keys = np.floor((cloud[:, 0] - cloud[:, 0].min()) / F(EDGE)).astype(np.int64)
    counts = np.bincount(keys)
    assert cloud[:, 0].min() == 0 and len(counts) == 45 and np.array_equal(np.flatnonzero(counts == m), [4, 13, 22, 31, 40])
    assert m > LONG_VOXEL and (np.delete(counts, [4, 13, 22, 31, 40]) == 9).all() and len(cloud) > 8 * 45
    assert ref.shape == (45, 3) and np.array_equal(np.floor(ref[:, 0] / F(EDGE)), np.arange(45)) and not ref[:, 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("m", [193, 256])
def test_voxel_filter_sort_path_with_several_long_voxels_among_short_ones(ctx, m):
    """five listed voxels for the wave kernel's fixed grid, between voxels the lane kernel folds: every centroid has the oracle's bits"""
    check_voxel_filter(ctx, m, 45, mixed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [9, LONG_VOXEL, LONG_VOXEL + 1, 300])
def test_voxel_filter_sort_path_with_the_two_level_scan(ctx, monkeypatch, m):
    """n just above 2049: two scan tiles, and TC_SCAN_FUSED_MAX=1 (read per call) sends them through the two-level scan inside key_runs"""
    v = 2049 // m + 1
    assert len(line_cloud(m, v)) > 2048
    monkeypatch.setenv("TC_SCAN_FUSED_MAX", "1")
    check_voxel_filter(ctx, m, v)


# ---- NDT voxel map ----
NDT_CASES = [(9, r) for r in (1, 255, 256, 257, 2049)] + [(129, 256), (300, 1), (300, 257)]


@functools.lru_cache(maxsize=None)
def ndt_reference(m, runs):
    """the checker's map in f64 and the budgets of tests/test_gpu_ndt.py (voxel_budget): 4 x the checker's own f32-to-f64 distance"""
    cloud = line_cloud(m, runs, alternate=True)
    g32, g64 = NC.build(cloud, EDGE, m, np.float32), NC.build(cloud, EDGE, m, np.float64)
    assert np.array_equal(g32[0], g64[0])
    scale = np.linalg.norm(g64[3], axis=(1, 2))
    d_inv = (np.linalg.norm(g32[3].astype(np.float64) - g64[3], axis=(1, 2)) / scale).max()
    d_mean = np.abs(g32[2].astype(np.float64) - g64[2]).max()
    return g64, 4 * max(d_inv, np.finfo(F).eps), 4 * max(d_mean, np.finfo(F).eps * np.abs(g64[2]).max())


@pytest.mark.parametrize("m,runs", NDT_CASES)
def test_line_cloud_alternates_runs_of_m_and_one_less(m, runs):
    cloud = line_cloud(m, runs, alternate=True)
    keys, counts, _, _ = NC.build(cloud, EDGE, 1, np.float32)
    assert np.array_equal(keys, np.c_[np.arange(runs), np.zeros((runs, 2), np.int64)])
    assert np.array_equal(counts, [m - r % 2 for r in range(runs)])
    g64 = ndt_reference(m, runs)[0]
    assert np.array_equal(g64[0][:, 0], np.arange(0, runs, 2)) and (g64[1] == m).all()         # min_points = m drops every second run


@pytest.mark.gpu
@pytest.mark.parametrize("m,runs", NDT_CASES)
def test_ndt_map_at_run_boundaries(ctx, m, runs):
    g64, b_inv, b_mean = ndt_reference(m, runs)
    keys, counts, mean, inv = ctx.ndt_voxels(line_cloud(m, runs, alternate=True), EDGE, m)
    assert keys.dtype == np.int32 and np.array_equal(keys, g64[0]) and np.array_equal(counts, g64[1])
    full = np.zeros((len(keys), 3, 3))
    for c, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        full[:, i, j] = full[:, j, i] = inv[:, c]
    d_inv = (np.linalg.norm(full - g64[3], axis=(1, 2)) / np.linalg.norm(g64[3], axis=(1, 2))).max()
    d_mean = np.abs(mean.astype(np.float64) - g64[2]).max()
    print(f"m = {m}, R = {runs}: V = {len(keys)}, inv_cov {d_inv:.2e} (budget {b_inv:.2e}), mean {d_mean:.2e} (budget {b_mean:.2e})")
    assert d_inv <= b_inv and d_mean <= b_mean


# ---- cluster extraction, member sort ----
CLUSTERS, ISOLATED, TOL = 257, 40, 0.25


@functools.lru_cache(maxsize=None)
def cluster_cloud():
    """257 cubes of 8 points (edge 0.2) ten apart on a 17-wide lattice and 40 points far from everything, shuffled"""
    corners = np.array([[i, j, k] for i in (-0.1, 0.1) for j in (-0.1, 0.1) for k in (-0.1, 0.1)])
    centres = np.array([[10.0 * (c % 17), 10.0 * (c // 17), 0.0] for c in range(CLUSTERS)])
    lone = np.array([[5.0 + 10.0 * i, 5.0, 50.0] for i in range(ISOLATED)])
    pts = np.concatenate([(centres[:, None, :] + corners).reshape(-1, 3), lone])
    pts = pts[np.random.default_rng(7).permutation(len(pts))].astype(F)
    pts.setflags(write=False)
    return pts, K.clusters(pts, TOL, 2, len(pts))


def check_members(labels, members, offsets):
    assert len(offsets) == CLUSTERS + 1 and np.array_equal(np.diff(offsets.astype(np.int64)), np.full(CLUSTERS, 8))
    assert np.count_nonzero(labels == K.NONE) == ISOLATED                      # (in the member sort they carry the key 257)
    groups = members[: int(offsets[-1])].astype(np.int64).reshape(CLUSTERS, 8)
    assert (np.diff(groups, axis=1) > 0).all()                                 # ascending inside every cluster
    assert (np.diff(groups[:, 0]) > 0).all()                                   # equal sizes: ranked by smallest original index
    assert all((labels[g] == k).all() for k, g in enumerate(groups))


def test_cluster_cloud_has_257_clusters_of_8_and_40_unlabelled_points():
    check_members(*cluster_cloud()[1])


@pytest.mark.gpu
def test_member_sort_with_unlabelled_points_behind_the_last_cluster(ctx):
    pts, (el, em, eo) = cluster_cloud()
    labels, members, offsets = ctx.extract_euclidean_clusters_labels(np.array(pts), TOL, 2, len(pts))
    check_members(labels, members, offsets)
    assert np.array_equal(offsets, eo) and np.array_equal(labels, el) and np.array_equal(members[: int(eo[-1])], em[: int(eo[-1])])
