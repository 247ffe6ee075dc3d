"""The three roads that share compact_flagged / store_compacted (grid.hip, tc_internal.h) -- the statistical outlier filter with a
threshold, the radius outlier filter and plane segmentation's inlier list -- on clouds whose kept set is known by construction:
nothing, everything, only the first point, only the last point, every second point, at every size around the compaction block
(256) and the scan tile (8 x 256 = 2048), with the fused and with the two-level scan (TC_SCAN_FUSED_MAX=1, read per call),
through the numpy and through the torch input.  Kept points and indices are compared exactly.

The constructions (unit spacing `tight`, 64 x that `coarse`, the two regions 64 apart at the least):
  statistical, k = 2   a kept point has its two nearest at distance ~1, a dropped one its second nearest at >= 64; "only the
                       first / last": P between Q1 and Q2 on a line, mean(P) = 1 against mean(Q) = 1.5, the narrowest gap of all.
                       The threshold is the geometric mean of the two classes' extreme means (checker values of the constructed
                       cloud), so each class is at least sqrt(1.5) = 1.22 x away from it: ~2^21 ulps, never a rounding question.
                       A lone point has mean 0 <= any positive threshold (filtering.rs:291), so "nothing" at n = 1 is a point
                       with a NaN coordinate: inert, mean NaN, never kept.
  radius, r = 1.5      squared distances are the integers 1 and 2 (inside) against 3, 4 or >= 4096 (outside r * r = 2.25);
                       min_neighbors is 2 for "first / last / everything" (P sees Q1 and Q2, they see only P) and 1 for "every
                       second" (n = 3 keeps a pair).
  plane, one triple    the kept points lie on z = 0 (the triple: the first three of them, (0,0) (1,0) (0,1)), the others on
                       z = 1, threshold 0.25: distances are exactly 0 and 1.
What the filters' definitions rule out, and what stands in for it (NOT_CONSTRUCTIBLE names every such case):
  radius, n = 1        a lone point has no neighbour and min_neighbors >= 1: only "nothing" exists.
  plane                an inlier set holds the three points that define the plane: "first" is {0, 1, 2}, "last" {n-3, n-2, n-1},
                       "every second" needs n >= 5, and "nothing" is the call's error (no candidate with a model: the list
                       stays unwritten).  n < 3 is an argument error and left out.
test_constructed_inputs_give_the_intended_kept_sets checks every construction with tests/outlier_checker.py /
tests/plane_checker.py without a device; the device tests build their inputs through the same (cached, checked) function."""
import functools
import math

import numpy as np
import pytest

import threecrate_amd as tc
from tests import outlier_checker as OC
from tests import plane_checker as PC

SIZES = [1, 3, 255, 256, 257, 2047, 2048, 2049, 4097]
PATTERNS = ["nothing", "everything", "first", "last", "every_second"]
ROADS = ["sor", "radius", "plane"]
K, RADIUS, PLANE_THR = 2, 1.5, 0.25
NO_MODEL = "Failed to find valid plane model"

NOT_CONSTRUCTIBLE = {("radius", 1, p) for p in PATTERNS if p != "nothing"} | {("plane", 3, "every_second")}


def kept_set(n, pattern, road):
    if pattern == "nothing":
        return np.zeros(0, np.int64)
    if pattern == "everything":
        return np.arange(n)
    if pattern == "every_second":
        return np.arange(0, n, 2)
    width = min(n, 3) if road == "plane" else 1
    return np.arange(width) if pattern == "first" else np.arange(n - width, n)


def tight(m):
    """m points of the unit lattice in a 2 x 2 column: from m = 3 on every point has two others within sqrt(2)"""
    i = np.arange(m)
    return np.stack([i % 2, (i // 2) % 2, i // 4], 1).astype(np.float32)


def flat(m):
    """m distinct points of the unit lattice in the plane, two wide: the first three are not collinear"""
    i = np.arange(m)
    return np.stack([i % 2, i // 2], 1).astype(np.float32)


def coarse(m):
    """m points 64 apart, the nearest of them 64 from everything `tight` can reach"""
    i = np.arange(m)
    return (np.stack([i % 8, (i // 8) % 8, i // 64], 1).astype(np.float32) + np.float32(1.0)) * np.float32(-64.0)


def neighbour_cloud(n, pattern):
    """the cloud of the two outlier roads"""
    p = np.empty((n, 3), np.float32)
    if pattern == "nothing":
        p[:] = coarse(n)
    elif pattern == "everything":
        p[:] = tight(n)
    elif pattern == "every_second":
        p[0::2] = tight((n + 1) // 2)
        p[1::2] = coarse(n // 2)
    else:                                                       # P between Q1 and Q2 on a line, the rest far away
        trio = np.array([[0, 0, 0], [-1, 0, 0], [1, 0, 0]], np.float32)[:n]
        rest = coarse(n - len(trio))
        p[:] = np.concatenate([trio, rest]) if pattern == "first" else np.concatenate([rest, trio[::-1]])
    return p


@functools.lru_cache(None)
def case(road, n, pattern):
    """-> (cloud, parameter, kept indices) with the checker's confirmation, or None (NOT_CONSTRUCTIBLE)"""
    if (road, n, pattern) in NOT_CONSTRUCTIBLE:
        return None
    keep = kept_set(n, pattern, road)
    if road == "plane":
        if pattern == "nothing":                               # every point off z = 0 and a collinear triple: no model
            p = np.concatenate([flat(n), np.ones((n, 1), np.float32)], 1)
            triple = np.array([[0, 0, 1]], np.uint32)
            assert PC.segment(p, PLANE_THR, triple)[0] is None
            return p, triple, keep
        p = np.empty((n, 3), np.float32)
        drop = np.setdiff1d(np.arange(n), keep)
        p[keep] = np.concatenate([flat(len(keep)), np.zeros((len(keep), 1), np.float32)], 1)
        p[drop] = np.concatenate([flat(len(drop)), np.ones((len(drop), 1), np.float32)], 1)
        triple = keep[:3].astype(np.uint32).reshape(1, 3)
        coeff, inl, best, counts = PC.segment(p, PLANE_THR, triple)
        assert best == 0 and np.array_equal(inl, keep) and counts[0] == len(keep)
        d = PC.distances(p, coeff)
        assert np.all(d[keep] == 0.0) and np.all(d[drop] == 1.0)
        return p, triple, keep
    p = neighbour_cloud(n, pattern)
    if road == "sor":
        if n == 1 and pattern == "nothing":
            p[0, 1] = np.nan
        mean = OC.mean_distances(p, K)
        inside, outside = mean[keep], np.delete(mean, keep)
        outside = outside[~np.isnan(outside)]
        hi = float(inside.max()) if len(inside) else 0.0
        lo = float(outside.min()) if len(outside) else math.inf
        assert lo >= 1.45 * hi, (n, pattern, hi, lo)            # the narrowest gap by construction: 1 against 1.5
        thr = math.sqrt(hi * lo) if hi > 0.0 and lo < math.inf else 2.0 * hi if hi > 0.0 else 0.5 * lo if lo < math.inf else 1.0
        assert hi * 1.2 <= thr <= lo / 1.2
        assert np.array_equal(OC.sor_keep(mean, thr), keep)
        return p, thr, keep
    min_neighbors = 1 if pattern == "every_second" else 2
    # (squared distances are the integers 1, 2 | 3, 4, ... against r * r = 2.25; the same set from sqrt(2) to sqrt(3))
    for r in (1.45, RADIUS, 1.7):
        assert np.array_equal(OC.radius_keep(p, r, min_neighbors), keep), (n, pattern, r)
    return p, min_neighbors, keep


def test_constructed_inputs_give_the_intended_kept_sets():
    built = 0
    for road in ROADS:
        for n in SIZES:
            for pattern in PATTERNS:
                if road == "plane" and n < 3:
                    continue
                c = case(road, n, pattern)
                assert (c is None) == ((road, n, pattern) in NOT_CONSTRUCTIBLE)
                if c is not None:
                    built += 1
                    assert np.array_equal(c[2], kept_set(n, pattern, road)) and len(c[0]) == n
    assert built == 3 * len(SIZES) * len(PATTERNS) - len(PATTERNS) - len(NOT_CONSTRUCTIBLE)       # (the plane has no n = 1)


# ---- on the device --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _check(p, keep, points, index):
    idx = _host(index).astype(np.int64) & 0xFFFFFFFF
    assert np.array_equal(idx, keep), (len(idx), len(keep))
    if points is not None:
        got = np.ascontiguousarray(_host(points), np.float32).reshape(-1, 3)
        assert got.shape == (len(keep), 3) and np.array_equal(got.view(np.uint32), p[keep].view(np.uint32))


def _scan(monkeypatch, two_level):
    if two_level:
        monkeypatch.setenv("TC_SCAN_FUSED_MAX", "1")


scan_modes = pytest.mark.parametrize("two_level", [False, True], ids=["fused", "two_level"])
sizes = pytest.mark.parametrize("n", SIZES)


@pytest.mark.gpu
@scan_modes
@sizes
def test_statistical_threshold_road(ctx, monkeypatch, n, two_level):
    _scan(monkeypatch, two_level)
    for pattern in PATTERNS:
        p, thr, keep = case("sor", n, pattern)
        for arr in (p, _dev(p)):
            pts, idx = ctx.statistical_outlier_removal_with_threshold(arr, K, thr, return_index=True)
            _check(p, keep, pts, idx)


@pytest.mark.gpu
@scan_modes
@sizes
def test_radius_road(ctx, monkeypatch, n, two_level):
    _scan(monkeypatch, two_level)
    for pattern in PATTERNS:
        c = case("radius", n, pattern)
        if c is None:
            continue                                            # (NOT_CONSTRUCTIBLE: a lone point keeps nothing, which "nothing" checks)
        p, min_neighbors, keep = c
        for arr in (p, _dev(p)):
            pts, idx = ctx.radius_outlier_removal(arr, RADIUS, min_neighbors, return_index=True)
            _check(p, keep, pts, idx)


@pytest.mark.gpu
@scan_modes
@pytest.mark.parametrize("n", [n for n in SIZES if n >= 3])
def test_plane_inlier_road(ctx, monkeypatch, n, two_level):
    _scan(monkeypatch, two_level)
    for pattern in PATTERNS:
        c = case("plane", n, pattern)
        if c is None:
            continue                                            # (NOT_CONSTRUCTIBLE: two points define no plane)
        p, triple, keep = c
        for arr, smp in ((p, triple), (_dev(p), _dev(triple))):
            if pattern == "nothing":
                with pytest.raises(tc.AlgorithmError, match=NO_MODEL):
                    ctx.segment_plane_samples(arr, PLANE_THR, smp)
                continue
            r = ctx.segment_plane_samples(arr, PLANE_THR, smp)
            assert r.num_inliers == len(keep) and r.best_iteration == 0
            _check(p, keep, None, r.inlier_indices)
