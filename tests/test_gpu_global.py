"""Descriptor matching and RANSAC over correspondences on the MI355X (csrc/global.hip, include/threecrate_hip_global.h, the companion
library) against tests/global_checker.py: matches and distances to the bit; every candidate's stored transform within the bound that
follows from an f64 solve; every candidate's count exactly, on the device's own transform bits; the winner's record in every field; the
seeded generator against the sequential recurrence; both roads.  What each input is there for is proven on the checker alone in
tests/test_global_cpu.py.  The whole pipeline: equal to its five public calls, and on the pose-recovery case the refined transform is the
planted one; the wheel-shaped functions of compat.py against GpuContext.global_registration; the header's order of checks."""
import ctypes as C
import functools

import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, synth
from tests import global_checker as G
from tests.test_gpu_parity import FROB_TOL

pytestmark = pytest.mark.gpu
F = np.float32


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
    return np.ascontiguousarray(_host(a)).view(np.uint32)


def _same_f32(got, want):
    """bit equality; two NaNs are equal whatever their sign and payload, which IEEE 754 leaves to the implementation"""
    g, w = np.ascontiguousarray(_host(got), F), np.ascontiguousarray(want, F)
    return g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


ROADS = ["numpy", "torch"]


def _to(road, *arrays):
    return [_dev(a) if road == "torch" else a for a in arrays]


# ---- matching ----
@functools.lru_cache(None)
def match_reference(kind, ns, nt):
    src, tgt = G.match_case(kind, ns, nt)
    return src, tgt, G.match(src, tgt)


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("kind", ["int", "float", "nan0", "nanmid", "equal"])
@pytest.mark.parametrize("ns,nt", G.MATCH_SIZES, ids=[f"{a}x{b}" for a, b in G.MATCH_SIZES])
def test_match_equals_the_checker_bit_for_bit(ctx, ns, nt, kind, road):
    src, tgt, (idx, dist) = match_reference(kind, ns, nt)
    s, t = _to(road, src, tgt)
    got_i, got_d = ctx.match_features(s, t, return_distance=True)
    assert np.array_equal(_bits(got_i), idx)
    assert _same_f32(got_d, dist)
    assert np.array_equal(_bits(ctx.match_features(s, t)), idx)                 # without the distances


@pytest.mark.parametrize("road", ROADS)
def test_match_refuses_another_dimension_and_an_empty_target(ctx, road):
    s, t = _to(road, np.zeros((4, 32), F), np.zeros((5, 32), F))
    with pytest.raises(tc.Unsupported):
        ctx.match_features(s, t)
    s, t = _to(road, np.zeros((4, 33), F), np.zeros((0, 33), F))
    with pytest.raises(tc.InvalidData):
        ctx.match_features(s, t)
    s, t = _to(road, np.zeros((0, 33), F), np.zeros((5, 33), F))
    assert len(ctx.match_features(s, t)) == 0


# ---- models ----
def _ulp(x):
    x = np.abs(np.asarray(x, F))
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)


@pytest.mark.parametrize("road", ROADS)
def test_models_are_the_f64_solve_rounded_once(ctx, road):
    """R within 2^-22 per entry, t within one f32 ulp of max(|t|, |c_t|, |c_s|): the device's f64 error at sigma_2 / sigma_1 >= 0.05 is
    many orders below half an f32 ulp, so the stored value is the correctly rounded one or its neighbour"""
    src, tgt, corr, smp, n_good = G.model_case()
    s, t, c, sm = _to(road, src, tgt, corr, smp)
    r = ctx.ransac_correspondences(s, t, c, c, 0.05, 2.0, samples=sm, candidates=True)
    T, cnt = _host(r.cand_transform), _bits(r.cand_count)
    worst_r = worst_t = 0.0
    for it in range(n_good):
        R, tt, cs, ct = G.model(src[smp[it].astype(np.int64)], tgt[smp[it].astype(np.int64)])
        dr = np.abs(T[it, :9].astype(np.float64) - R.reshape(9)).max()
        bound = _ulp(max(np.abs(tt).max(), np.abs(ct).max(), np.abs(cs).max()))
        dt = np.abs(T[it, 9:].astype(np.float64) - tt).max() / bound
        worst_r, worst_t = max(worst_r, dr), max(worst_t, dt)
    print(f"worst |dR| = {worst_r:.3e} (bound {2.0 ** -22:.3e}), worst |dt| = {worst_t:.3f} ulp of the bound's scale (bound 1)")
    assert worst_r <= 2.0 ** -22 and worst_t <= 1.0
    assert np.isfinite(T[:n_good]).all()
    # equal indices, an index >= m, three collinear points, a non-finite point: no model, count 0
    assert np.isnan(T[n_good:]).all() and (cnt[n_good:] == 0).all() and len(T) == n_good + 4


# ---- scores ----
@functools.lru_cache(None)
def score_inputs(m, n_cand):
    return G.score_case(m, n_cand)


def assert_scores(r, src, tgt, cs, ct, thr):
    """every count exact on the device's own stored transforms, and the record the literal loop's on those counts"""
    T = _host(r.cand_transform)
    ps, pt = G.gather(src, tgt, cs, ct)
    want = G.score(T, ps, pt, thr)
    assert np.array_equal(_bits(r.cand_count), want)
    return T, want


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("m,n_cand", G.SCORE_SIZES, ids=[f"{a}x{b}" for a, b in G.SCORE_SIZES])
def test_counts_are_exact_on_the_devices_own_transforms(ctx, m, n_cand, road):
    src, tgt, cs, ct, smp = score_inputs(m, n_cand)
    a = _to(road, src, tgt, cs, ct, smp)
    r = ctx.ransac_correspondences(*a[:4], G.SCORE_THRESHOLD, 2.0, samples=a[4], candidates=True)       # E = 2 m: no exit
    T, want = assert_scores(r, src, tgt, cs, ct, G.SCORE_THRESHOLD)
    ref = G.ransac(src, tgt, cs, ct, G.SCORE_THRESHOLD, 2.0, smp, transforms=T)
    assert (r.inlier_count, r.iterations_run, r.best_iteration, r.early_exit) == (ref["inlier_count"], n_cand, ref["best_iteration"], False)
    assert np.array_equal(_bits(r.transform), ref["transform"].view(np.uint32)) and F(r.inlier_ratio) == ref["inlier_ratio"]
    if m >= 8 and n_cand >= 8:
        assert np.isnan(T[2]).all() and np.isnan(T[5]).all()


@pytest.mark.parametrize("road", ROADS)
def test_threshold_ulp_by_ulp_across_a_pairs_distance(ctx, road):
    m, n_cand = 65, 129
    src, tgt, cs, ct, smp = score_inputs(m, n_cand)
    a = _to(road, src, tgt, cs, ct, smp)
    r = ctx.ransac_correspondences(*a[:4], G.SCORE_THRESHOLD, 2.0, samples=a[4], candidates=True)
    T = _host(r.cand_transform)
    ps, pt = G.gather(src, tgt, cs, ct)
    d2 = G.d2_all(T, ps, pt)
    c = int(np.nonzero(~np.isnan(T).any(1))[0][0])
    p = int(np.nanargmin(np.abs(d2[c] - F(0.09))))
    thr = F(np.sqrt(d2[c, p]))
    while thr * thr < d2[c, p]:
        thr = np.nextafter(thr, F(np.inf))
    while np.nextafter(thr, F(0)) * np.nextafter(thr, F(0)) >= d2[c, p]:
        thr = np.nextafter(thr, F(0))
    below = np.nextafter(thr, F(0))                 # thr: the smallest threshold whose f32 square reaches d2; below: the largest that does not
    assert below * below < d2[c, p] <= thr * thr
    counts = {}
    for name, v in (("below", below), ("at", thr), ("above", np.nextafter(thr, F(np.inf)))):
        rr = ctx.ransac_correspondences(*a[:4], float(v), 2.0, samples=a[4], candidates=True)
        assert np.array_equal(_bits(rr.cand_transform), T.view(np.uint32))
        counts[name] = assert_scores(rr, src, tgt, cs, ct, v)[1]
    assert counts["at"][c] == counts["below"][c] + 1 == counts["above"][c]


# ---- winner ----
@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("name", G.WINNER_CASES + ["tie_across_chunks"])
def test_winner_is_the_sequential_loops(ctx, name, road):
    src, tgt, corr = G.winner_pairs()
    smp = G.tie_case() if name == "tie_across_chunks" else G.winner_case(name)
    ratio = 0.9 if name in ("tie_across_chunks", "no_exit") else G.WINNER_RATIO
    s, t, c, sm = _to(road, src, tgt, corr, smp)
    r = ctx.ransac_correspondences(s, t, c, c, G.WINNER_THRESHOLD, ratio, samples=sm, candidates=True)
    T = _host(r.cand_transform)
    ref = G.ransac(src, tgt, corr, corr, G.WINNER_THRESHOLD, ratio, smp, transforms=T)
    run = ref["iterations_run"]
    # chunks behind the exit's are not scored (0); everything below iterations_run is
    done = min(len(smp), -(-run // G.CHUNK) * G.CHUNK)
    cnt = _bits(r.cand_count)
    assert np.array_equal(cnt[:done], ref["cand_count"][:done]) and (cnt[done:] == 0).all()
    assert (r.inlier_count, r.iterations_run, r.best_iteration, r.early_exit) == (ref["inlier_count"], run, ref["best_iteration"], ref["early_exit"])
    assert F(r.inlier_ratio) == ref["inlier_ratio"] and np.array_equal(_bits(r.transform), ref["transform"].view(np.uint32))
    expect = {"exit_first_chunk": (77, True, 78), "exit_chunk_last_row": (G.CHUNK - 1, True, G.CHUNK), "two_exits": (300, True, 301),
              "exit_second_chunk_first_row": (G.CHUNK, True, G.CHUNK + 1), "tie_across_chunks": (300, False, len(smp)),
              "nothing_wins": (0, False, len(smp)), "no_exit": (G.CHUNK + 904, False, len(smp))}.get(name)
    if expect:
        assert (r.best_iteration, r.early_exit, r.iterations_run) == expect
    if name == "nothing_wins":
        assert r.inlier_count == 0 and np.array_equal(r.transform, G.IDENTITY12)
    else:
        assert r.inlier_count == G.WINNER_INLIERS


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("m,iters,seed", [(3, 129, 0), (4, 129, 7), (5, 64, 1), (65, 2 * G.CHUNK + 1, 0), (1000, 4097, 2 ** 63 + 5)])
def test_seeded_twin_draws_the_recurrences_triples(ctx, m, iters, seed, road):
    src, tgt, cs, ct, _ = score_inputs(max(m, 8), 8)
    cs, ct = cs[:m].copy(), ct[:m].copy()
    smp = G.lcg_triples(m, iters, seed)
    a = _to(road, src, tgt, cs, ct, smp)
    seeded = ctx.ransac_correspondences(*a[:4], G.SCORE_THRESHOLD, 2.0, iters, seed, candidates=True)
    given = ctx.ransac_correspondences(*a[:4], G.SCORE_THRESHOLD, 2.0, samples=a[4], candidates=True)
    assert np.array_equal(_bits(seeded.cand_transform), _bits(given.cand_transform))
    assert np.array_equal(_bits(seeded.cand_count), _bits(given.cand_count))
    assert np.array_equal(_bits(seeded.transform), _bits(given.transform)) and seeded.best_iteration == given.best_iteration


@pytest.mark.parametrize("road", ROADS)
def test_errors_through_both_roads(ctx, road):
    src, tgt, cs, ct, smp = score_inputs(65, 8)
    a = _to(road, src, tgt, cs, ct, smp)
    with pytest.raises(tc.InvalidData, match="Too few feature correspondences"):
        ctx.ransac_correspondences(a[0], a[1], a[2][:2], a[3][:2], 0.1)
    with pytest.raises(tc.InvalidData, match="Threshold must be positive"):
        ctx.ransac_correspondences(*a[:4], 0.0)
    with pytest.raises(tc.InvalidData, match="Max iterations must be positive"):
        ctx.ransac_correspondences(*a[:4], 0.1, max_iterations=0)
    with pytest.raises(tc.Unsupported):
        ctx.ransac_correspondences(*a[:4], 0.1, max_iterations=G.MAX_ITERS + 1)
    r = ctx.ransac_correspondences(*a[:4], 0.1, max_iterations=64)              # the context is still usable
    assert r.iterations_run <= 64


# ---- the pipeline is its five public calls ----
@functools.lru_cache(None)
def pipeline_pair():
    """2 000 points of an asymmetric surface (a tilted paraboloid with a ridge) and the same surface moved"""
    u = synth.uniform_cloud(2000, 21)
    x, y = u[:, 0].astype(np.float64), u[:, 1].astype(np.float64)
    z = 0.4 * x * x + 0.15 * y + 0.25 * np.maximum(0.0, x - 0.6 * y) + 0.02 * u[:, 2]
    tgt = np.stack([x, y, z], 1).astype(F)
    src = synth.apply_isometry(synth.yaw_isometry((0.2, -0.1, 0.05), 0.3), tgt)
    return src, tgt


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("refine", [False, True])
@pytest.mark.parametrize("given_normals", [False, True])
def test_global_registration_is_its_five_public_calls(ctx, given_normals, refine, road):
    src, tgt = _to(road, *pipeline_pair())
    cfg = tc.GlobalRegistrationConfig(ransac_iterations=G.CHUNK + 1, distance_threshold=0.05, fpfh_radius=0.2, refine_with_icp=refine,
                                      icp_max_iterations=10, seed=3)
    sn, tn = ctx.estimate_normals(src, cfg.normal_k_neighbors), ctx.estimate_normals(tgt, cfg.normal_k_neighbors)
    got = ctx.global_registration(src, tgt, cfg, sn, tn) if given_normals else ctx.global_registration(src, tgt, cfg)
    sd = ctx.extract_fpfh_features_with_normals(sn, cfg.fpfh_radius, cfg.fpfh_k_neighbors)
    td = ctx.extract_fpfh_features_with_normals(tn, cfg.fpfh_radius, cfg.fpfh_k_neighbors)
    match = ctx.match_features(sd, td)
    n = len(pipeline_pair()[0])
    arange = _to(road, np.arange(n, dtype=np.uint32))[0]
    rr = ctx.ransac_correspondences(sn[:, 0:3], tn[:, 0:3], arange, match, cfg.distance_threshold, cfg.inlier_ratio, cfg.ransac_iterations, cfg.seed)
    assert np.array_equal(_bits(got.ransac.transform), _bits(rr.transform))
    assert (got.inlier_count, got.inlier_ratio, got.ransac.best_iteration) == (rr.inlier_count, rr.inlier_ratio, rr.best_iteration)
    init = tc.rotation_to_isometry(rr.transform)
    if refine:
        icp = ctx.icp_point_to_point(src, tgt, init, cfg.icp_max_iterations, 1e-6, None, correspondences=False)
        assert np.array_equal(_bits(got.transformation), _bits(icp.transformation)) and got.icp_result.iterations == icp.iterations
        assert F(got.icp_result.mse).view(np.uint32) == F(icp.mse).view(np.uint32)
    else:
        assert got.icp_result is None and np.array_equal(_bits(got.transformation), _bits(init))
        assert np.array_equal(got.matrix[:3, :3].reshape(9), rr.transform[:9])


# ---- the pipeline recovers a planted pose ----
@pytest.mark.parametrize("road", ROADS)
def test_global_registration_recovers_the_planted_pose(ctx, road):
    """global_checker.pose_case(): the CPU twin shows that the checker chain ends inside ICP's basin there (and that the identity does
    not).  The refined transform is the planted one within FROB_TOL, the bound tests/test_gpu_registration_variants.py holds
    point-to-point ICP to (scale 1: coordinates below 10)."""
    src, tgt, sn, tn, planted = G.pose_case()
    cfg = tc.GlobalRegistrationConfig(ransac_iterations=G.POSE_ITERS, distance_threshold=G.POSE_THRESHOLD, fpfh_radius=G.POSE_RADIUS,
                                      fpfh_k_neighbors=G.POSE_K, seed=G.POSE_SEED)
    a = _to(road, src, tgt, np.concatenate([src, sn], 1), np.concatenate([tgt, tn], 1))
    r = ctx.global_registration(a[0], a[1], cfg, a[2], a[3])
    coarse = np.linalg.norm(r.ransac.matrix.astype(np.float64) - planted)
    fine = np.linalg.norm(np.asarray(r.matrix, np.float64) - planted)
    print(f"inliers {r.inlier_count} of {len(src)}, winner {r.ransac.best_iteration}, Frobenius to the planted pose: RANSAC {coarse:.3e}, "
          f"refined {fine:.3e} (bound {FROB_TOL:.0e}); ICP iterations {r.icp_result.iterations}, mse {r.icp_result.mse:.3e}")
    assert r.inlier_count >= G.exit_count(0.25, len(src)) and G.partners_are_nearest(r.ransac.transform, src, tgt) == 1.0
    assert fine <= FROB_TOL
    # without the refinement the same call returns RANSAC's pose, and ICP from the identity does not find the planted one
    cfg.refine_with_icp = False
    r0 = ctx.global_registration(a[0], a[1], cfg, a[2], a[3])
    assert r0.icp_result is None and np.array_equal(_bits(r0.ransac.transform), _bits(r.ransac.transform))
    alone = ctx.icp_point_to_point(a[0], a[1], None, 50, 1e-6, None, correspondences=False)
    assert np.linalg.norm(np.asarray(alone.matrix, np.float64) - planted) > 1.0         # (2.73 on the oracle: the CPU twin)


def test_the_wheels_functions_are_the_contexts_pipeline():
    """compat.global_registration / global_registration_with_normals through PointCloud / NormalPointCloud against
    GpuContext.global_registration on the default context: the same matrix bits, statistics and refinement record"""
    src, tgt = pipeline_pair()
    kw = dict(ransac_iterations=G.CHUNK + 1, distance_threshold=0.04, inlier_ratio=0.3, fpfh_radius=0.2, fpfh_k_neighbors=11,
              normal_k_neighbors=12, refine_with_icp=True, icp_max_iterations=7)
    cfg = tc.GlobalRegistrationConfig(G.CHUNK + 1, 0.04, 0.3, 0.2, 11, 12, True, 7, None)
    dctx = tc.default_context()
    want = dctx.global_registration(src, tgt, cfg)
    got = threecrate.global_registration(threecrate.PointCloud(src), threecrate.PointCloud(tgt), **kw)
    sn, tn = dctx.estimate_normals(src, 12), dctx.estimate_normals(tgt, 12)
    got_n = threecrate.global_registration_with_normals(threecrate.NormalPointCloud(sn), threecrate.NormalPointCloud(tn),
                                                        threecrate.PointCloud(src), threecrate.PointCloud(tgt), **kw)
    for g in (got, got_n):
        assert np.array_equal(_bits(g.transformation()), _bits(want.matrix)) and g.transformation().shape == (4, 4)
        assert (g.inlier_count, g.inlier_ratio) == (want.inlier_count, want.inlier_ratio) and g.inlier_count > 0
        assert g.icp_converged == want.icp_result.converged and F(g.icp_mse).view(np.uint32) == F(want.icp_result.mse).view(np.uint32)
    kw["refine_with_icp"] = False
    g = threecrate.global_registration(threecrate.PointCloud(src), threecrate.PointCloud(tgt), **kw)
    assert g.icp_mse is None and g.icp_converged is None and np.array_equal(g.transformation()[:3, :3].reshape(9), want.ransac.transform[:9])
    with pytest.raises(RuntimeError, match="Source point cloud is empty"):
        threecrate.global_registration(threecrate.PointCloud(), threecrate.PointCloud(tgt))


# ---- the header's order of checks, at the raw entry points with a live context ----
def test_checks_come_in_the_headers_order(ctx):
    Lg, h = ctx._global(), ctx._h
    msg = lambda: ctx._L.tc_last_error_message(h).decode()
    buf = np.full(256, 7, np.uint32)
    p, big = buf.ctypes.data, (1 << 32) - 16
    T, r = (C.c_float * 12)(*([7.0] * 12)), _lib.RansacResultC(7, 7, 7, 7, 7.0)
    INV, UNS, OK = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED, _lib.TC_OK
    for fn in (Lg.tc_match_features, Lg.tc_match_features_device):
        assert fn(h, None, 0, None, 0, 32, None, None) == UNS                   # the dimension before ns == 0
        assert fn(h, None, 0, None, 0, 33, None, None) == OK                    # ns == 0 before the NULL arrays and nt == 0
        assert fn(h, None, 4, p, 0, 33, p, None) == INV and "NULL" in msg()     # a NULL array before nt == 0
        assert fn(h, p, 4, p, 0, 33, p, None) == INV and "no target" in msg()   # nt == 0 before the limit
        assert fn(h, p, big, p, 0, 33, p, None) == INV
        assert fn(h, p, big, p, 4, 33, p, None) == UNS and fn(h, p, 4, p, big, 33, p, None) == UNS
        assert fn(h, p, big - 1, p, 4, 32, p, None) == UNS
    seeded = [(Lg.tc_ransac_correspondences, False), (Lg.tc_ransac_correspondences_device, False),
              (Lg.tc_ransac_correspondences_samples, True), (Lg.tc_ransac_correspondences_samples_device, True)]
    for fn, smp in seeded:
        def call(m=4, thr=0.1, iters=10, src=p, samples=p, ns=4, nt=4, transform=T, result=C.byref(r)):
            mid = (samples, iters) if smp else (iters, 0)
            return fn(h, src, ns, p, nt, p, p, m, thr, 0.25, *mid, transform, result, None, None)
        assert call(transform=None, m=2) == INV and call(result=None, thr=0.0) == INV       # NULL outputs before everything
        assert call(m=2, thr=0.0) == INV and "Too few feature correspondences" in msg()
        assert call(thr=0.0, iters=0) == INV and "Threshold must be positive" in msg()
        assert call(thr=-1.0, src=None) == INV and "Threshold must be positive" in msg()
        assert call(iters=0, src=None) == INV and "Max iterations must be positive" in msg()
        assert call(src=None, ns=big) == INV and "NULL" in msg()
        if smp:
            assert call(samples=None, iters=(1 << 20) + 1) == INV and "samples is NULL" in msg()
        assert call(ns=big, iters=(1 << 20) + 1) == UNS and "2^32" in msg()
        assert call(nt=big) == UNS and call(m=big) == UNS
        assert call(iters=(1 << 20) + 1) == UNS and "2^20" in msg()
        assert call(iters=1 << 20, m=2) == INV
    assert (buf == 7).all() and list(T) == [7.0] * 12 and (r.inlier_count, r.iterations_run, r.best_iteration, r.early_exit) == (7, 7, 7, 7)


def test_index_arrays_of_the_other_kind_and_wider_integers(ctx):
    """host index arrays with device clouds are moved to the device; int64 indices keep their low 32 bits, 0xFFFFFFFF included"""
    import torch
    src, tgt, cs, ct, smp = score_inputs(65, 129)
    want = ctx.ransac_correspondences(src, tgt, cs, ct, G.SCORE_THRESHOLD, 2.0, samples=smp, candidates=True)
    assert (cs == G.NONE).any()
    d = _to("torch", src, tgt)
    wide = [torch.from_numpy(a.astype(np.int64)).cuda() for a in (cs, ct, smp)]
    for idx in ((cs, ct, smp), wide, (cs.astype(np.int64), ct.astype(np.int64), smp.astype(np.int64))):
        got = ctx.ransac_correspondences(d[0], d[1], idx[0], idx[1], G.SCORE_THRESHOLD, 2.0, samples=idx[2], candidates=True)
        assert np.array_equal(_bits(got.cand_count), _bits(want.cand_count)) and np.array_equal(_bits(got.cand_transform), _bits(want.cand_transform))
    got = ctx.ransac_correspondences(src, tgt, torch.from_numpy(cs.astype(np.int64)), ct.astype(np.int64), G.SCORE_THRESHOLD, 2.0, samples=smp,
                                     candidates=True)
    assert np.array_equal(_bits(got.cand_count), _bits(want.cand_count))
