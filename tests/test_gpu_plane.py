"""RANSAC plane segmentation on the MI355X against tests/plane_checker.py: coefficients to the bit, the winner's index, the inlier
list and every candidate's count; the seeded generator against the checker's triples; the threshold's boundary ulp by ulp; ties,
candidates without a model, non-finite points, errors through every road, both roads and two runs bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib
from tests import plane_checker as PC

pytestmark = pytest.mark.gpu
F = np.float32
NO_MODEL = "Failed to find valid plane model"


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


def _bits(a):
    return np.ascontiguousarray(_host(a), F).view(np.uint32)


@functools.lru_cache(None)
def cloud(kind, n):
    return {"clutter": PC.plane_clutter_cloud, "two": PC.two_plane_cloud}[kind](n)


@functools.lru_cache(None)
def triples(n, iters, seed=0):
    return PC.samples(n, iters, seed)


@functools.lru_cache(None)
def reference(kind, n, iters, thr, seed=0):
    """the checker's answer, computed once per case"""
    return PC.segment(cloud(kind, n), thr, triples(n, iters, seed))


def assert_result(r, ref, iters):
    coeff, inl, best, _ = ref
    assert np.array_equal(_bits(r.plane_coefficients), coeff.view(np.uint32)), (r.plane_coefficients, coeff)
    assert r.best_iteration == best and r.iterations == iters
    got = _host(r.inlier_indices).astype(np.int64)
    assert np.array_equal(got, inl) and r.num_inliers == len(got)


# The scoring kernel (csrc/plane.hip) walks point tiles of kPlanePointsPerBlock = 1024 and candidate chunks of kPlaneCandChunk = 128:
# n and max_iters one below, at and one above each, next to the sizes around a wave (64) and the odd large ones.
SIZES = [3, 4, 63, 64, 65, 1000, 1023, 1024, 1025, 4097, 20011]
ITERS = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 1025]
CASES = sorted({(n, 129 if n > 65 else 65) for n in SIZES} | {(1025, it) for it in ITERS} | {(65, it) for it in ITERS if it <= 65} |
               {(4097, 1000), (20011, 1025)})
THR = 0.02


@pytest.mark.parametrize("kind", ["clutter", "two"])
@pytest.mark.parametrize("n,iters", CASES)
def test_samples_against_the_checker(ctx, kind, n, iters):
    p, t = cloud(kind, n), triples(n, iters)
    ref = reference(kind, n, iters, THR)
    assert ref[2] is not None
    assert_result(ctx.segment_plane_samples(p, THR, t), ref, iters)
    if n <= 65 and iters <= 65:         # every candidate's count: a call per triple, whose n_inliers is that candidate's score
        counts = []
        for row in t:
            try:
                counts.append(ctx.segment_plane_samples(p, THR, row[None, :], return_index=False).num_inliers)
            except tc.AlgorithmError:
                counts.append(0)
        assert counts == ref[3].tolist()


@pytest.mark.parametrize("seed", [0, 0xDEADBEEFCAFEF00D])
@pytest.mark.parametrize("n,iters", [(3, 65), (4, 129), (5, 64), (1000, 1025), (4097, 1000)])
def test_seeded_call_draws_the_checkers_triples(ctx, n, iters, seed):
    """the device's jump-ahead generator, the collision fallback included (n = 3, 4, 5), against the sequential recurrence"""
    p = cloud("clutter", n)
    ref = reference("clutter", n, iters, THR, seed)
    r = ctx.segment_plane(p, THR, iters, seed)
    assert_result(r, ref, iters)
    s = ctx.segment_plane_samples(p, THR, triples(n, iters, seed))
    assert np.array_equal(_bits(s.plane_coefficients), _bits(r.plane_coefficients)) and s.best_iteration == r.best_iteration
    assert np.array_equal(_host(s.inlier_indices), _host(r.inlier_indices))
    # each iteration's triple alone: a one-candidate call over the checker's row gives the count the seeded winner has
    if iters <= 129:
        one = ctx.segment_plane_samples(p, THR, triples(n, iters, seed)[r.best_iteration][None, :])
        assert one.num_inliers == r.num_inliers


# (n, max_iters, seed, iteration): tests/test_plane_cpu.py::test_winner_clouds_single_out_one_iteration holds the checker to each
WINNER_CASES = [(5, 64, 0, 7), (5, 64, 0, 5), (7, 64, 0, 28), (7, 64, 0, 34), (7, 64, 0xDEADBEEFCAFEF00D, 13),
                (7, 64, 0xDEADBEEFCAFEF00D, 28), (40, 300, 0, 22), (40, 300, 0, 119), (40, 300, 5, 37), (40, 300, 5, 144)]


@pytest.mark.parametrize("n,iters,seed,target", WINNER_CASES)
def test_seeded_call_draws_a_late_iterations_triple(ctx, n, iters, seed, target):
    """A cloud in which only the triple of iteration `target` (half of the cases a collision fallback, half three plain draws) lies
    in a plane with a fourth point: the seeded call must name that iteration, which it can only with that iteration's own triple."""
    t = triples(n, iters, seed)
    p = PC.winner_cloud(n, t, target)
    for arr in (p, _dev(p)):
        r = ctx.segment_plane(arr, float(PC.WINNER_THRESHOLD), iters, seed)
        assert r.best_iteration == target and r.num_inliers == 4
        assert sorted(_host(r.inlier_indices).tolist()) == sorted(np.nonzero(p[:, 2] == 0)[0].tolist())
        assert set(t[target].tolist()) <= set(_host(r.inlier_indices).tolist())


def test_samples_on_the_host_with_a_device_cloud(ctx):
    """a CPU tensor of samples beside a device cloud is moved to the cloud's device, not handed over as a host pointer"""
    import torch
    p, t = cloud("clutter", 1000), triples(1000, 64)
    r = ctx.segment_plane_samples(_dev(p), THR, torch.from_numpy(t.view(np.int32)))
    assert_result(r, reference("clutter", 1000, 64, THR), 64)


def test_boundary_unit_normal(ctx):
    """plane z = 0 from (0,0,0), (1,0,0), (0,1,0): the stored normal is (0, 0, 1), m == 1 exactly; threshold 0.25"""
    q = F(0.25)
    up, down = np.nextafter(q, F(1)), np.nextafter(q, F(0))
    zs = [0, 0, 0, q, -q, up, -up, down, -down, np.nextafter(up, F(1)), -np.nextafter(down, F(0))]
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]] + [[0.5, 0.25, z] for z in zs[3:]], F)
    r = ctx.segment_plane_samples(p, 0.25, np.array([[0, 1, 2]], np.uint32))
    assert r.plane_coefficients.tolist() == [0.0, 0.0, 1.0, 0.0] or r.plane_coefficients.tolist() == [0.0, 0.0, 1.0, -0.0]
    assert _host(r.inlier_indices).tolist() == [0, 1, 2, 3, 4, 7, 8, 10]
    assert np.array_equal(_host(r.inlier_indices), PC.inliers(p, PC.model(p, (0, 1, 2)), 0.25))


def test_boundary_tilted(ctx):
    """The band cloud of tests/test_plane_cpu.py::test_the_band_cloud_straddles_the_threshold_ulp_by_ulp: m != 1, hundreds of points
    within 4 ulps of the threshold on either side and on it.  The inlier set is the checker's, point for point, as one candidate
    and among others (the band's points as further triples), on both roads.  A score that skips the division (|s| <= t) decides
    300 of these points differently and fails here; one that compares |s| with fl(t * m) does not differ from the division for
    any m a normalised triple can have and no input can tell the two apart."""
    p, triple = PC.tilted_band_cloud()
    t = np.array([triple], np.uint32)
    coeff = PC.model(p, triple)
    want = PC.inliers(p, coeff, PC.BAND_THRESHOLD)
    for arr, smp in ((p, t), (_dev(p), _dev(t))):
        r = ctx.segment_plane_samples(arr, float(PC.BAND_THRESHOLD), smp)
        assert np.array_equal(_bits(r.plane_coefficients), coeff.view(np.uint32))
        assert r.num_inliers == len(want) and np.array_equal(_host(r.inlier_indices).astype(np.int64), want)
    many = np.concatenate([PC.samples(len(p), 200), t])
    ref = PC.segment(p, PC.BAND_THRESHOLD, many)
    assert_result(ctx.segment_plane_samples(p, float(PC.BAND_THRESHOLD), many), ref, len(many))


def parallel_planes(per_plane=1500):
    """z = 0 and z = 1 over the same xy lattice: any non-collinear triple of one plane scores per_plane"""
    xy = np.array([[i % 50, i // 50] for i in range(per_plane)], F)
    return np.concatenate([np.column_stack([xy, np.zeros(per_plane, F)]), np.column_stack([xy, np.ones(per_plane, F)])]).astype(F)


@pytest.mark.parametrize("rows", [(5, 90), (5, 200), (127, 128), (0, 299)])        # one candidate chunk (128), and two
def test_equal_scores_go_to_the_lower_index(ctx, rows):
    p = parallel_planes()                # 3000 points: three point tiles
    n0 = len(p) // 2
    lower, upper = (0, 1, 50), (n0, n0 + 1, n0 + 50)
    for first, second, z in ((lower, upper, 0.0), (upper, lower, 1.0)):
        t = np.zeros((300, 3), np.uint32)                      # every other row repeats point 0: no model
        t[rows[0]], t[rows[1]] = first, second
        r = ctx.segment_plane_samples(p, 0.1, t)
        assert r.best_iteration == rows[0] and r.num_inliers == n0
        assert (p[_host(r.inlier_indices), 2] == z).all()
        assert_result(r, PC.segment(p, 0.1, t), 300)


def test_no_winner(ctx):
    p = np.array([[i, 2 * i, 3 * i] for i in range(70)], F)                      # a line
    for arr in (p, _dev(p)):
        with pytest.raises(tc.AlgorithmError, match=NO_MODEL):
            ctx.segment_plane(arr, 0.1, 200)
    with pytest.raises(tc.AlgorithmError, match=NO_MODEL):
        ctx.segment_plane_samples(p, 0.1, np.array([[0, 0, 1], [3, 3, 3]], np.uint32))
    q = cloud("clutter", 1000)
    for arr in (q, _dev(q)):
        with pytest.raises(tc.AlgorithmError, match=NO_MODEL):                    # `d <= NaN` holds for nothing
            ctx.segment_plane(arr, float("nan"), 100)


def test_sample_index_past_the_cloud_is_a_candidate_without_a_model(ctx):
    n = 1000
    p = cloud("clutter", n)
    t = triples(n, 64).copy()
    t[0] = (n, 1, 2)
    t[5] = (1, 0xFFFFFFFF, 2)
    t[63] = (1, 2, n + 7)
    ref = PC.segment(p, THR, t)
    for arr, smp in ((p, t), (_dev(p), _dev(t))):
        assert_result(ctx.segment_plane_samples(arr, THR, smp), ref, 64)
    with pytest.raises(tc.AlgorithmError, match=NO_MODEL):
        ctx.segment_plane_samples(p, THR, t[[0, 5, 63]])


def test_non_finite_points(ctx):
    n = 1100
    p = cloud("clutter", n).copy()
    p[[7, 300, 1050], 0] = np.nan
    p[[8, 1099], 1] = np.inf
    p[9, 2] = -np.inf
    t = triples(n, 129).copy()
    t[0] = (7, 1, 2)            # a NaN model: it has no inlier and cannot win
    t[1] = (3, 8, 4)
    t[2] = (9, 5, 6)
    ref = PC.segment(p, THR, t)
    assert ref[3][:3].tolist() == [0, 0, 0] and not set(ref[1].tolist()) & {7, 8, 9, 300, 1050, 1099}
    for arr, smp in ((p, t), (_dev(p), _dev(t))):
        assert_result(ctx.segment_plane_samples(arr, THR, smp), ref, 129)
    with pytest.raises(tc.AlgorithmError, match=NO_MODEL):
        ctx.segment_plane_samples(p, THR, t[:3])


def test_null_outputs_at_the_entry_points(ctx):
    """inlier_index NULL skips the list, best_iteration NULL is not written; an over-allocated list keeps its tail"""
    import torch
    L, n, iters = ctx._L, 1025, 129
    p, t = cloud("clutter", n), triples(n, iters)
    coeff_ref, inl, best, _ = reference("clutter", n, iters, THR)
    dp, dt = _dev(p), _dev(t)
    for road in ("host", "device"):
        x, s = (dp, dt) if road == "device" else (p, t)
        ptr = lambda a: a.data_ptr() if road == "device" else a.ctypes.data
        seeded = L.tc_segment_plane_device if road == "device" else L.tc_segment_plane
        sampled = L.tc_segment_plane_samples_device if road == "device" else L.tc_segment_plane_samples
        for want_index in (True, False):
            for want_best in (True, False):
                idx = np.full(n + 5, -7, np.int32)
                idx = _dev(idx) if road == "device" else idx
                torch.cuda.synchronize()        # filled on torch's stream, read on the library's own
                coeff, n_in, b = (C.c_float * 4)(), C.c_size_t(0), C.c_uint32(77)
                tail = (coeff, ptr(idx) if want_index else None, C.byref(n_in), C.byref(b) if want_best else None)
                assert sampled(ctx._h, ptr(x), n, THR, ptr(s), iters, *tail) == 0
                assert np.array_equal(np.array(coeff[:], F).view(np.uint32), coeff_ref.view(np.uint32)) and n_in.value == len(inl)
                assert b.value == (best if want_best else 77)
                i = _host(idx)
                assert np.array_equal(i[:len(inl)], inl) and (i[len(inl):] == -7).all() if want_index else (i == -7).all()
                n_in.value = 0
                assert seeded(ctx._h, ptr(x), n, THR, iters, 0, *tail) == 0 and n_in.value == len(inl)
    r = ctx.segment_plane(p, THR, iters, return_index=False)
    assert r.inlier_indices is None and r.num_inliers == len(inl) and r.best_iteration == best


def _raises(fn, exc, msg):
    with pytest.raises(exc) as e:
        fn()
    assert str(e.value) == msg


ERRORS = [                  # cloud size, threshold, max_iters: in the reference's order
    ((2, 0.0, 0), tc.InvalidData, "Need at least 3 points for plane segmentation"),
    ((5, 0.0, 0), tc.InvalidData, "Threshold must be positive"),
    ((5, -0.1, 10), tc.InvalidData, "Threshold must be positive"),
    ((5, 0.1, 0), tc.InvalidData, "Max iterations must be positive"),
    ((5, 0.1, 2 ** 20 + 1), tc.Unsupported, "segment_plane: more than 2^20 iterations are not supported by the HIP backend"),
]


def test_errors_through_every_road(ctx):
    rng = np.random.default_rng(5)
    five = rng.random((5, 3), dtype=F)
    for (n, thr, iters), exc, msg in ERRORS:
        p = five[:n]
        for arr in (p, _dev(p)):
            _raises(lambda: ctx.segment_plane(arr, thr, iters), exc, msg)
        _raises(lambda: tc.segment_plane(p, thr, iters, ctx=ctx), exc, msg)
        _raises(lambda: tc.segment_plane_ransac(p, iters, thr, ctx=ctx), exc, msg)
        _raises(lambda: tc.plane_segmentation_ransac(p, iters, thr, ctx=ctx), exc, msg)
        _raises(lambda: tc.gpu_segment_plane_ransac(ctx, p, thr, iters), exc, msg)
        # an error of the inputs comes before the facade's min_inliers check; a limit of this backend after it
        _raises(lambda: tc.gpu_segment_plane(ctx, p, tc.GpuPlaneSegmentationConfig(iters, thr, 0 if exc is tc.InvalidData else 1)), exc, msg)
        _raises(lambda: threecrate.segment_plane(threecrate.PointCloud(p), thr, iters), RuntimeError, msg)
        if iters <= 10:         # the samples road has the same checks, n_samples in the place of max_iters
            smp = np.zeros((iters, 3), np.uint32)
            for arr, s in ((p, smp), (_dev(p), _dev(smp))):
                _raises(lambda: ctx.segment_plane_samples(arr, thr, s), exc, msg)
    # the raw entry points: status, message, *n_inliers zeroed, nothing else written
    L = ctx._L
    dp = _dev(five)
    import torch
    torch.cuda.synchronize()
    for fn, x in ((L.tc_segment_plane, five.ctypes.data), (L.tc_segment_plane_device, dp.data_ptr())):
        for (n, thr, iters), exc, msg in ERRORS:
            coeff, n_in, b = (C.c_float * 4)(7, 7, 7, 7), C.c_size_t(9), C.c_uint32(9)
            rc = fn(ctx._h, x, n, thr, iters, 0, coeff, None, C.byref(n_in), C.byref(b))
            assert rc == (_lib.TC_UNSUPPORTED if exc is tc.Unsupported else _lib.TC_INVALID_DATA)
            assert L.tc_last_error_message(ctx._h).decode() == msg and n_in.value == 0 and b.value == 9 and list(coeff) == [7.0] * 4
        coeff, n_in = (C.c_float * 4)(), C.c_size_t(9)
        assert fn(ctx._h, x, 2 ** 32 - 16, 0.1, 10, 0, coeff, None, C.byref(n_in), None) == _lib.TC_UNSUPPORTED
        assert L.tc_last_error_message(ctx._h) == b"more than 2^32 points"
        assert fn(ctx._h, x, 5, 0.1, 10, 0, None, None, C.byref(n_in), None) == _lib.TC_INVALID_DATA
        assert fn(ctx._h, x, 5, 0.1, 10, 0, coeff, None, None, None) == _lib.TC_INVALID_DATA
    for fn, x in ((L.tc_segment_plane_samples, five.ctypes.data), (L.tc_segment_plane_samples_device, dp.data_ptr())):
        coeff, n_in = (C.c_float * 4)(), C.c_size_t(9)
        assert fn(ctx._h, x, 5, 0.1, None, 4, coeff, None, C.byref(n_in), None) == _lib.TC_INVALID_DATA and n_in.value == 0
    # the facade's own checks (threecrate-gpu/src/segmentation.rs:304-324, :853-861)
    p = cloud("clutter", 1000)
    _raises(lambda: tc.gpu_segment_plane(ctx, p, tc.GpuPlaneSegmentationConfig(min_inliers=0)), tc.InvalidData, "min_inliers must be at least 1")
    r = tc.gpu_segment_plane(ctx, p)
    _raises(lambda: tc.gpu_segment_plane(ctx, p, tc.GpuPlaneSegmentationConfig(min_inliers=r.num_inliers + 1)), tc.AlgorithmError,
            f"Plane model has {r.num_inliers} inliers, below required minimum {r.num_inliers + 1}")
    assert tc.gpu_segment_plane(ctx, p, tc.GpuPlaneSegmentationConfig(min_inliers=r.num_inliers)).num_inliers == r.num_inliers
    _raises(lambda: ctx.segment_plane(p, 0.1, -1), tc.InvalidData, "max_iters must not be negative")


def test_python_roads_and_names_agree(ctx):
    """numpy road and torch road bit for bit; module functions, facades and the compat class return the same plane"""
    for n, iters in ((65, 65), (1025, 129), (20011, 1000)):
        p = cloud("two", n)
        a, b = ctx.segment_plane(p, THR, iters, seed=11), ctx.segment_plane(_dev(p), THR, iters, seed=11)
        assert hasattr(b.inlier_indices, "cpu") and not hasattr(a.inlier_indices, "cpu")
        assert np.array_equal(_bits(a.plane_coefficients), _bits(b.plane_coefficients))
        assert (a.best_iteration, a.num_inliers, a.iterations) == (b.best_iteration, b.num_inliers, b.iterations)
        assert np.array_equal(a.inlier_indices, _host(b.inlier_indices)) and a.inlier_indices.dtype == np.uint32
        t = triples(n, iters, 11)
        c, d = ctx.segment_plane_samples(p, THR, t), ctx.segment_plane_samples(_dev(p), THR, _dev(t))
        for r in (c, d):
            assert np.array_equal(_bits(r.plane_coefficients), _bits(a.plane_coefficients)) and r.best_iteration == a.best_iteration
            assert np.array_equal(_host(r.inlier_indices), a.inlier_indices)
    p = cloud("clutter", 1000)
    ref = reference("clutter", 1000, 1000, THR)
    assert_result(tc.segment_plane(p, THR, 1000, ctx=ctx), ref, 1000)
    assert_result(tc.gpu_segment_plane_ransac(ctx, p, THR, 1000), ref, 1000)
    assert_result(tc.gpu_segment_plane(ctx, p, tc.GpuPlaneSegmentationConfig(distance_threshold=THR)), ref, 1000)
    for fn in (tc.segment_plane_ransac, tc.plane_segmentation_ransac):
        coeff, inl = fn(p, 1000, THR, ctx=ctx)
        assert np.array_equal(_bits(coeff), ref[0].view(np.uint32)) and np.array_equal(inl, ref[1])
    cr = threecrate.segment_plane(threecrate.PointCloud(p), THR)
    assert np.array_equal(_bits(cr.plane_coefficients()), ref[0].view(np.uint32)) and cr.inlier_indices() == ref[1].tolist()
    assert cr.num_inliers == len(ref[1]) and np.array_equal(cr.inlier_cloud(threecrate.PointCloud(p)).to_numpy(), p[ref[1]])


def test_two_calls_are_bit_identical(ctx):
    p = cloud("two", 20011)
    for arr in (p, _dev(p)):
        a, b = (ctx.segment_plane(arr, THR, 1025, seed=3) for _ in range(2))
        assert np.array_equal(_bits(a.plane_coefficients), _bits(b.plane_coefficients))
        assert (a.best_iteration, a.num_inliers) == (b.best_iteration, b.num_inliers)
        assert np.array_equal(_host(a.inlier_indices), _host(b.inlier_indices))


def test_after_the_other_users_of_the_pinned_union(ctx):
    """plane_out shares its bytes with the filters' and the cluster extraction's read-back words: a call right after them on one
    context gives what a fresh context gives"""
    p = cloud("clutter", 4097)
    used = tc.GpuContext(0)
    try:
        used.radius_outlier_removal(p, 0.2, 3)
        used.extract_euclidean_clusters(p, 0.05, 5, 4097)
        a = used.segment_plane(p, THR, 129)
        used.statistical_outlier_removal(p, 8, 1.0)
        b = used.segment_plane(p, THR, 129)
    finally:
        used.close()
    fresh = tc.GpuContext(0)
    try:
        c = fresh.segment_plane(p, THR, 129)
    finally:
        fresh.close()
    ref = reference("clutter", 4097, 129, THR)
    for r in (a, b, c):
        assert_result(r, ref, 129)
