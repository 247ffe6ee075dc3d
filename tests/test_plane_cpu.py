"""RANSAC plane segmentation without a GPU: the checker (tests/plane_checker.py) against the reference's doc example and unit tests
(segmentation.rs:285-291, :546-604), the sampler, the tie rule, the names and the null-context behaviour of its surface
(include/threecrate_hip_segmentation.h) and the precondition of the GPU boundary test."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import plane_checker as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the reference's doc example and unit tests ----
def test_doc_example_three_points():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    coeff, inl, best, counts = PC.segment(pts, 0.01, PC.samples(3, 1000))
    assert inl.tolist() == [0, 1, 2] and best == 0 and counts.tolist() == [3] * 1000
    assert coeff[0] == 0 and coeff[1] == 0 and abs(coeff[2]) == 1 and coeff[3] == 0


def test_plane_model_from_points():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    m = PC.model(pts, (0, 1, 2))
    assert abs(m[2]) > 0.9
    assert (PC.distances(pts, m) < 1e-6).all()


def test_collinear_and_repeated_points_give_no_model():
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0]], F)
    assert PC.model(pts, (0, 1, 2)) is None
    assert PC.model(pts, (0, 0, 3)) is None and PC.model(pts, (3, 1, 3)) is None and PC.model(pts, (1, 1, 1)) is None
    assert PC.model(pts, (0, 1, 4)) is None          # an index past the cloud
    assert PC.model(pts, (0, 1, 3)) is not None


def test_plane_distance_calculation():
    m = np.array([0, 0, 1, -1], F)
    d = PC.distances(np.array([[0, 0, 1], [0, 0, 2], [0, 0, 0]], F), m)
    assert d.tolist() == [0.0, 1.0, 1.0]
    assert np.isinf(PC.distances(np.zeros((2, 3), F), np.array([0, 0, 0, 1], F))).all()      # :63-65


def _grid_cloud(side, extra=()):
    return np.array([[i, j, 0] for i in range(side) for j in range(side)] + list(extra), F)


def test_segment_plane_simple():
    pts = _grid_cloud(10, [[5, 5, 10], [5, 5, -10]])
    coeff, inl, _, _ = PC.segment(pts, 0.1, PC.samples(len(pts), 100))
    assert len(inl) >= 95 and abs(coeff[2]) > 0.9
    assert 100 not in inl and 101 not in inl


def test_segment_plane_tilted():
    rng = np.random.default_rng(0)
    pts = np.array([[i, j, -(i + j)] for i in range(15) for j in range(15)], np.float64) + rng.uniform(-0.02, 0.02, (225, 3))
    pts = np.concatenate([pts, np.column_stack([rng.uniform(0, 15, 30), rng.uniform(0, 15, 30), rng.uniform(5, 10, 30)])]).astype(F)
    coeff, inl, _, _ = PC.segment(pts, 0.1, PC.samples(len(pts), 1000))
    assert len(inl) >= 200
    assert abs(float(coeff[:3] @ (np.ones(3) / np.sqrt(3.0)))) > 0.8


# ---- the sampler ----
@pytest.mark.parametrize("n", [3, 4, 5, 1000])
def test_sampler_triples_are_distinct_and_in_range(n):
    s = PC.samples(n, 300)
    assert s.shape == (300, 3) and s.dtype == np.uint32 and (s < n).all()
    assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()


def test_sampler_takes_the_fallback_at_three_points():
    """three draws from {0, 1, 2} collide 7 times in 9: the closed form (it % n, (37 it + 1) % n, (101 it + 2) % n, then bumped
    until distinct) must show up, and it is a different rule from the draws"""
    n, iters = 3, 60
    s = PC.samples(n, iters)
    state = ((n << 32) ^ iters ^ PC.GOLDEN) & PC.M64
    taken = 0
    for it in range(iters):
        d = []
        for _ in range(3):
            state = (state * PC.LCG_MUL + PC.LCG_INC) & PC.M64
            d.append((state >> 32) % n)
        if len(set(d)) < 3:
            taken += 1
            a = it % 3
            b = (it * 37 + 1) % 3
            b = b if b != a else (b + 1) % 3
            c = (it * 101 + 2) % 3
            while c in (a, b):
                c = (c + 1) % 3
            assert s[it].tolist() == [a, b, c]
        else:
            assert s[it].tolist() == d
    assert taken >= 30


def test_sampler_literals():
    """n = 1000, max_iters = 3, seed 0, by hand from the recurrence: state0 = (1000 << 32) ^ 3 ^ 0x9E3779B97F4A7C15 =
    0x9e377a517f4a7c16; state <- state * 6364136223846793005 + 1442695040888963407 mod 2^64 gives 0xfe0065070bdc3b2d,
    0x002f50471baa3b38, 0x84d94b395f4cb227, ...; the high words 4261438727, 3100743, 2228833081, ... modulo 1000"""
    assert PC.samples(1000, 3).tolist() == [[727, 743, 81], [606, 343, 462], [546, 788, 906]]
    assert PC.samples(1000, 3, seed=1).tolist() != PC.samples(1000, 3).tolist()
    # the seed is XORed into the initial state: seed == state0 starts the recurrence from 0, whose first state is the increment
    first = (PC.LCG_INC >> 32) % 1000
    assert PC.samples(1000, 3, seed=0x9e377a517f4a7c16)[0, 0] == first


# ---- the tie rule ----
def tie_cloud():
    """two parallel planes, z = 0 and z = 1, five points each; rows 0 and 1 of the samples lie in one each"""
    lo = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0]]
    return np.array(lo + [[x, y, 1] for x, y, _ in lo], F)


def test_equal_scores_go_to_the_lower_index():
    pts = tie_cloud()
    for first, second, z in (((0, 1, 2), (5, 6, 7), 0.0), ((5, 6, 7), (0, 1, 2), 1.0)):
        coeff, inl, best, counts = PC.segment(pts, 0.1, [first, second])
        assert counts.tolist() == [5, 5] and best == 0
        assert -coeff[3] / coeff[2] == z and (pts[inl, 2] == z).all()
    # a candidate without a model, or with no inlier, never wins
    assert PC.segment(pts, 0.1, [(0, 1, 10), (0, 0, 1)])[2] is None
    assert PC.segment(pts, np.nan, [(0, 1, 2)])[2] is None


# ---- what is this feature's own of the surface (tests/test_abi_surfaces.py holds header, table, Rust file and library together) ----
def test_rust_facade_has_the_reference_names():
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ("segment_plane", "segment_plane_ransac", "plane_segmentation_ransac", "gpu_segment_plane", "gpu_segment_plane_ransac"):
        assert re.search(r"pub fn " + fn + r"\(", lib_rs), fn
    for st in ("PlaneModel", "PlaneSegmentationResult", "GpuPlaneSegmentationResult", "GpuPlaneSegmentationConfig"):
        assert re.search(r"pub struct " + st + r"\b", lib_rs), st


def test_every_segmentation_export_returns_a_status_and_writes_nothing_without_a_context():
    L = _lib.load()
    pts = np.zeros((4, 3), F)
    smp = np.array([[0, 1, 2]], np.uint32)
    coeff, n_in, best = (C.c_float * 4)(7, 7, 7, 7), C.c_size_t(7), C.c_uint32(7)
    tail = (coeff, None, C.byref(n_in), C.byref(best))
    assert L.tc_segment_plane(None, pts.ctypes.data, 4, 0.1, 10, 0, *tail) == _lib.TC_INVALID_DATA
    assert L.tc_segment_plane_device(None, pts.ctypes.data, 4, 0.1, 10, 0, *tail) == _lib.TC_INVALID_DATA
    assert L.tc_segment_plane_samples(None, pts.ctypes.data, 4, 0.1, smp.ctypes.data, 1, *tail) == _lib.TC_INVALID_DATA
    assert L.tc_segment_plane_samples_device(None, pts.ctypes.data, 4, 0.1, smp.ctypes.data, 1, *tail) == _lib.TC_INVALID_DATA
    assert n_in.value == 7 and best.value == 7 and list(coeff) == [7.0] * 4       # nothing is written without a context


def test_python_surface():
    import threecrate_amd as tc
    import threecrate_amd.compat as threecrate
    for name in ("segment_plane", "segment_plane_samples"):
        assert callable(getattr(tc.GpuContext, name))
    for name in ("segment_plane", "segment_plane_ransac", "plane_segmentation_ransac", "gpu_segment_plane", "gpu_segment_plane_ransac"):
        assert callable(getattr(tc, name))
    sig = inspect.signature(tc.GpuContext.segment_plane)
    assert list(sig.parameters)[1:] == ["cloud", "threshold", "max_iters", "seed", "return_index"]
    assert sig.parameters["seed"].default == 0 and sig.parameters["return_index"].default is True
    assert list(inspect.signature(tc.segment_plane_ransac).parameters)[:3] == ["cloud", "max_iters", "threshold"]       # :297-301
    assert list(inspect.signature(tc.plane_segmentation_ransac).parameters)[:3] == ["cloud", "max_iters", "threshold"]
    cfg = tc.GpuPlaneSegmentationConfig()
    assert (cfg.max_iterations, cfg.distance_threshold, cfg.min_inliers) == (1000, 0.02, 1)
    r = tc.PlaneSegmentationResult(np.zeros(4, F), np.zeros(0, np.uint32), 5)
    assert r.iterations == 5 and hasattr(r, "plane_coefficients") and hasattr(r, "inlier_indices")
    assert "segment_plane" in threecrate.__all__ and "PlaneSegmentationResult" in threecrate.__all__
    sig = inspect.signature(threecrate.segment_plane)                       # threecrate-python/src/lib.rs:1262
    assert list(sig.parameters) == ["cloud", "threshold", "max_iterations"]
    assert sig.parameters["threshold"].default == 0.01 and sig.parameters["max_iterations"].default == 1000
    cr = threecrate.PlaneSegmentationResult(np.array([0, 0, 1, 0], F), np.array([0, 2], np.uint32))
    assert cr.num_inliers == 2 and cr.inlier_indices() == [0, 2] and cr.plane_coefficients().dtype == np.float32
    cloud = threecrate.PointCloud(np.arange(9, dtype=F).reshape(3, 3))
    assert cr.inlier_cloud(cloud).to_numpy().tolist() == [[0, 1, 2], [6, 7, 8]]
    assert repr(cr) == "PlaneSegmentationResult(inliers=2, normal=[0.000, 0.000, 1.000])"


# ---- precondition of test_gpu_plane.py::test_boundary_tilted ----
def test_the_band_cloud_straddles_the_threshold_ulp_by_ulp():
    """The stored normal of the band cloud's plane is not of length 1, at least 50 points lie within 4 ulps of the threshold on each
    side of it and at least one exactly on it -- by the checker alone.  A score that skips the division (|s| <= t) decides hundreds
    of these points differently, which is what the GPU test catches.  A score that multiplies instead (|s| <= fl(t * m)) decides
    none of them differently, here or anywhere a search has looked: a normalised triple's m is one of 1 - 3 * 2^-24 ... 1 + 2^-23,
    and for those no threshold and no |s| separates the two tests (test_multiply_and_divide_agree_for_every_normal_length_a_triple_gives)."""
    pts, triple = PC.tilted_band_cloud()
    coeff = PC.model(pts, triple)
    m, t = PC.normal_length(coeff), PC.BAND_THRESHOLD
    assert m != 1.0
    d = PC.distances(pts, coeff)
    k = np.rint((d.astype(np.float64) - float(t)) / float(np.spacing(t)))
    below, above, on = int(((k < 0) & (k >= -4)).sum()), int(((k > 0) & (k <= 4)).sum()), int((d == t).sum())
    undivided = int(((np.abs(PC.signed_offsets(pts, coeff)) <= t) != (d <= t)).sum())
    print(f"m = {m!r}: {below} within 4 ulps below, {above} within 4 ulps above, {on} on the threshold; {undivided} decided differently without the division")
    multiplied = int(((np.abs(PC.signed_offsets(pts, coeff)) <= t * m) != (d <= t)).sum())
    assert below >= 50 and above >= 50 and on >= 1
    assert undivided >= 100 and multiplied == 0


def test_multiply_and_divide_agree_for_every_normal_length_a_triple_gives():
    """Why no test can tell `|s| <= fl(t * m)` from `fl(|s| / m) <= t`: the normal lengths of 200 000 random triples take five values,
    1 - 3 * 2^-24 ... 1 + 2^-23, and for each of them, 200 000 thresholds over nine decades and |s| within 4 ulps of fl(t * m), the two
    decisions are the same.  (Further from 1 they are not: m = 1 + 3 * 2^-23, t = 0.5833333, |s| one ulp above fl(t * m).)"""
    rng = np.random.default_rng(1)
    p = rng.uniform(-1, 1, (600000, 3)).astype(F)
    v1, v2 = p[1::3] - p[0::3], p[2::3] - p[0::3]
    cx = v1[:, 1] * v2[:, 2] - v1[:, 2] * v2[:, 1]
    cy = v1[:, 2] * v2[:, 0] - v1[:, 0] * v2[:, 2]
    cz = v1[:, 0] * v2[:, 1] - v1[:, 1] * v2[:, 0]
    ln = np.sqrt(cx * cx + cy * cy + cz * cz)
    a, b, c = cx / ln, cy / ln, cz / ln
    lengths = np.unique(np.sqrt(a * a + b * b + c * c))
    print("normal lengths - 1:", [float(v) - 1.0 for v in lengths])
    assert len(lengths) <= 6 and lengths.min() >= F(1) - F(4 * 2.0 ** -24) and lengths.max() <= F(1) + F(2.0 ** -23)
    ts = (10.0 ** rng.uniform(-6, 3, 200000)).astype(F)

    def differing(m):
        prod, n = ts * m, 0
        for k in range(-4, 5):
            s = prod.copy()
            for _ in range(abs(k)):
                s = np.nextafter(s, F(np.inf) if k > 0 else F(0))
            n += int((((s / m) <= ts) != (s <= prod)).sum())
        return n
    for m in lengths:
        assert differing(m) == 0, m
    ts = np.array([0.5833333134651184], F)
    assert differing(F(1) + F(3 * 2.0 ** -23)) == 1


WINNER_CASES = [(5, 64, 0, 7, True), (5, 64, 0, 5, False), (7, 64, 0, 28, True), (7, 64, 0, 34, False), (7, 64, 0xDEADBEEFCAFEF00D, 13, True),
                (7, 64, 0xDEADBEEFCAFEF00D, 28, False), (40, 300, 0, 22, True), (40, 300, 0, 119, False), (40, 300, 5, 37, True),
                (40, 300, 5, 144, False)]


@pytest.mark.parametrize("n,iters,seed,target,fallback", WINNER_CASES)
def test_winner_clouds_single_out_one_iteration(n, iters, seed, target, fallback):
    """precondition of test_gpu_plane.py::test_seeded_call_draws_a_late_iterations_triple: in the checker, iteration `target` is the
    first with four inliers, every earlier one has three, and its triple is (is not) the collision fallback"""
    t = PC.samples(n, iters, seed)
    assert bool(PC.collisions(n, iters, seed)[target]) is fallback
    p = PC.winner_cloud(n, t, target)
    _, inl, best, counts = PC.segment(p, PC.WINNER_THRESHOLD, t)
    assert best == target and counts[target] == 4 and (counts[:target] == 3).all() and counts.max() == 4
    assert inl.tolist() == np.nonzero(p[:, 2] == 0)[0].tolist()
