"""GICP, KISS-ICP, multiscale ICP and the batch call against the oracle where their pair terms are visible.

The inputs come from tests/test_registration_inputs_cpu.py, which shows on the oracle alone that every case is usable (its f32
run and its exact_sums run agree to a third of the budget, the pair counts and error classes are the ones the case is built
for, exact ties are rarer than the share of differing pairs allowed here) and carries the mutation evidence: one Gauss-Newton
step from a non-trivial start on independent samplings of one surface moves by hundreds of budgets when a covariance, its
rotation or its order is wrong.

Transforms: h1.transform_budget at test_gpu_parity's FROB_TOL with scale = max(1, max |coordinate| / 10), the oracle as the
reference.  Pairs: equal to the oracle's; a differing pair must be an exact f32 tie under either side's transform, and at most
1e-3 of the pairs may differ (R.pairs_equal_or_tied).
"""
import numpy as np
import pytest
import torch

import threecrate_amd as tc

from oracle import oracle as O
from tests import h1
from tests import test_registration_inputs_cpu as R
from tests.test_gpu_parity import FROB_TOL

pytestmark = pytest.mark.gpu

assert FROB_TOL == R.FROB_TOL
ERROR_CLASS = {O.INVALID_DATA: tc.InvalidData, O.ALGORITHM: tc.AlgorithmError}


def _budget(g, run_ref, run_exact, *clouds):
    return h1.transform_budget(g.transformation, run_ref, run_exact, FROB_TOL, scale=R.scale_of(*clouds))


def _start(init):
    return O.IDENTITY if init is None else init


# ---- GICP -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(R.GICP_ONE_STEP))
def test_gicp_one_step_matches_oracle(ctx, case):
    """One Gauss-Newton step: curved sheet at k = 20 / 4 / 5 / 64, a volumetric pair, the out-of-box pair, the small and odd sizes
    and the 5 / 6 pair boundary.  The transform, mse and pairs are the oracle's, or the error class is."""
    s, t, init, (iters, md, thr, k) = R.GICP_ONE_STEP[case]
    cfg = tc.GicpConfig(iters, md, thr, k)
    want = R.GICP_EXPECTED_ERROR.get(case)
    if want is not None:
        with pytest.raises(ERROR_CLASS[want]):
            ctx.gicp(s, t, init, cfg)
        return
    g = ctx.gicp(s, t, init, cfg)
    r = R.run_gicp(case)
    report = _budget(g, lambda: r, lambda: R.run_gicp(case, exact_sums=True), s, t)
    print(case, report, "mse", g.mse, r.mse)
    assert g.iterations == 1 and not g.converged
    assert abs(g.mse - r.mse) <= 1e-5 * r.mse
    R.pairs_equal_or_tied(s, t, _start(init), _start(init), g.correspondences, r.correspondences)


@pytest.mark.parametrize("steps", [2, 3])
def test_gicp_unconverged_run_returns_its_last_step(ctx, steps):
    """threshold 0: exactly `steps` steps; the returned mse and pairs are the ones the last step measured before its update
    (gicp.rs:284-305).  The oracle's pairs and mse of the step before differ (shown in the inputs' module)."""
    s, t, init, (_, md, thr, k) = R.GICP_ONE_STEP["sheet_k20"]
    g = ctx.gicp(s, t, init, tc.GicpConfig(steps, md, thr, k))
    g_before = ctx.gicp(s, t, init, tc.GicpConfig(steps - 1, md, thr, k))
    r = R.run_gicp("sheet_k20", max_iterations=steps)
    r_before = R.run_gicp("sheet_k20", max_iterations=steps - 1)
    report = _budget(g, lambda: r, lambda: R.run_gicp("sheet_k20", exact_sums=True, max_iterations=steps), s, t)
    print(steps, report, "mse", g.mse, r.mse)
    assert g.iterations == steps and not g.converged
    assert abs(g.mse - r.mse) <= 1e-5 * r.mse
    R.pairs_equal_or_tied(s, t, g_before.transformation, r_before.transformation, g.correspondences, r.correspondences)


def test_gicp_out_of_box_queries_under_the_counting_instantiation(ctx):
    """The out-of-box pair again (its oracle comparison is the refine_k20 case above) in profile mode 3: GICP's main pass has a
    counting instantiation, and it must give the plain one's bits.  TC_COUNTER_ICP_* count the MAIN pass's searches; the length of
    the refine list is not among them, so that the pushed quarter of the source is served by the refine pass's copy of the
    accumulation rests on the construction (queries 0.2 ... 0.4 outside the target's box, paired under a distance of 1.0)."""
    s, t, init, (iters, md, thr, k) = R.GICP_ONE_STEP["refine_k20"]
    a = ctx.gicp(s, t, init, tc.GicpConfig(iters, md, thr, k))
    ctx.profile_enable(3)
    try:
        b = ctx.gicp(s, t, init, tc.GicpConfig(iters, md, thr, k))
        st = ctx.search_stats()
    finally:
        ctx.profile_enable(0)
    assert np.array_equal(a.transformation, b.transformation) and a.mse == b.mse and np.array_equal(a.correspondences, b.correspondences)
    assert st["iterations"] == 1 and st["searches"] == len(s)             # the cold first pass searches every point
    assert st["wave_trips"] * 64 >= len(s) and st["candidate_steps_needed"] >= st["searches"]
    _, _, pushed = R.gicp_refine_pair()
    assert np.isin(pushed, a.correspondences[:, 0]).all()


def test_gicp_device_inputs_equal_host_inputs(ctx):
    s, t, init, (iters, md, thr, k) = R.GICP_ONE_STEP["sheet_k20"]
    cfg = tc.GicpConfig(iters, md, thr, k)
    h = ctx.gicp(s, t, init, cfg)
    d = ctx.gicp(torch.from_numpy(s).cuda(), torch.from_numpy(t).cuda(), init, cfg)
    assert np.array_equal(d.transformation, h.transformation) and d.mse == h.mse and d.iterations == h.iterations
    assert d.converged == h.converged and np.array_equal(d.correspondences, h.correspondences)


# ---- KISS-ICP ------------------------------------------------------------------------------------------------------------------
def _kiss_compare(ctx, src, tgt, prior, min_range=0.0, max_range=100.0):
    """one iteration of kiss_icp against the oracle: n_source_down, the pairs over the down-sampled source, the transform (the
    budget, with the oracle's exact_sums run standing for the unspecified order of the reference's down-sampled source, as
    test_kiss_icp_matches_oracle does), iterations / converged, mse.  -> (gpu result, oracle result)"""
    cfg = tc.KissIcpConfig(R.KISS_VOXEL, max_range, min_range, 1)
    kw = dict(min_range=min_range, max_range=max_range)
    res, err = R.outcome(R.run_kiss, src, tgt, prior, **kw)
    if err is not None:
        with pytest.raises(ERROR_CLASS[err]):
            ctx.kiss_icp(src, tgt, prior, cfg)
        return None, None
    r, nd = res
    g = ctx.kiss_icp(src, tgt, prior, cfg)
    assert len(g.corr_target) == nd
    down, _ = R.kiss_down(src, R.KISS_VOXEL, min_range, max_range)
    R.pairs_equal_or_tied(down, tgt, _start(prior), _start(prior), g.correspondences, r.correspondences)
    report = _budget(g, lambda: r, lambda: R.run_kiss(src, tgt, prior, exact_sums=True, **kw)[0], src, tgt)
    print(report, "mse", g.mse, r.mse)
    assert (g.iterations, g.converged) == (r.iterations, r.converged) == (1, False)
    assert abs(g.mse - r.mse) <= 1e-3 * max(r.mse, 1e-6)                   # (test_kiss_icp_matches_oracle's bound)
    return g, r


def test_kiss_range_filter_keeps_both_ends(ctx):
    """min_range^2 <= |p|^2 <= max_range^2 in f32, both ends inclusive: points exactly on either end and one ulp inside are kept,
    one ulp outside are dropped; every such point has a voxel and a partner of its own, so n_source_down and the pairs tell."""
    src, tgt, specials, kept = R.kiss_range_case()
    g, r = _kiss_compare(ctx, src, tgt, None, R.KISS_MIN_RANGE, R.KISS_MAX_RANGE)
    dense = np.asarray(g.corr_target).astype(np.int64)
    down, _ = R.kiss_down(src, R.KISS_VOXEL, R.KISS_MIN_RANGE, R.KISS_MAX_RANGE)
    for p in np.nonzero(kept)[0]:
        hit = np.nonzero((down == specials[p]).all(1))[0]
        assert len(hit) == 1 and dense[hit[0]] == len(tgt) - 6 + p


@pytest.mark.parametrize("name", sorted(R.KISS_PRIORS))
def test_kiss_adaptive_threshold_clamps(ctx, name):
    """3 * motion clamped to [3, 10] voxels (kiss_icp.rs:82-95): the identity, a prior strictly between the clamps and a 5 m prior
    give three pair sets (three different counts in the oracle), each equal to the oracle's."""
    src, tgt, prior = R.kiss_prior_case(name)
    sigma = O.kiss_adaptive_threshold(prior, R.KISS_VOXEL)
    assert {"identity": sigma == pytest.approx(3 * R.KISS_VOXEL, rel=1e-6), "five_metres": sigma == pytest.approx(10 * R.KISS_VOXEL, rel=1e-6),
            "between": 3 * R.KISS_VOXEL < sigma < 10 * R.KISS_VOXEL}[name]
    g, r = _kiss_compare(ctx, src, tgt, prior)
    # the pairs are the ones within that threshold: every paired source within sigma, every unpaired one beyond it
    down, _ = R.kiss_down(src, R.KISS_VOXEL, 0.0, 100.0)
    ts = O.isometry_apply(prior, down)
    nn = np.sqrt(np.array([h1.d2_f32(tgt, q).min() for q in ts], np.float32))
    paired = np.zeros(len(down), bool)
    paired[g.correspondences[:, 0]] = True
    assert (nn[paired] <= np.float32(sigma)).all() and (nn[~paired] > np.float32(sigma)).all()


@pytest.mark.parametrize("n_down", R.KISS_SIZES)
def test_kiss_small_down_sampled_sources(ctx, n_down):
    """the voxel filter leaves 1, 2 (fewer than three pairs: the oracle's error class), 5, 64 and 257 points; "row5": five nearly
    collinear points far from the target's box centre, where sums of uncentred f32 products ended 3.0e-5 from the oracle"""
    src, tgt = R.kiss_size_case(n_down)
    want = 5 if n_down == "row5" else n_down
    g, r = _kiss_compare(ctx, src, tgt, None)
    assert (g is None) == (want < 3)
    if g is not None:
        assert len(g.correspondences) == want


# ---- multiscale ICP -----------------------------------------------------------------------------------------------------------
def _multiscale_config(levels):
    fin_it, fin_md, thr = R.MULTISCALE_TAIL
    return tc.MultiScaleIcpConfig([tc.IcpScaleLevel(v, it, md) for v, it, md in levels], fin_it, fin_md, thr)


@pytest.mark.parametrize("name", ["skipped_level", "init", "biting"])
def test_multiscale_matches_oracle(ctx, name):
    """a first level that leaves fewer than three voxels and is skipped; a non-identity init; level distances that drop 40 % of
    the pairs: iterations, converged and the transform are the oracle's"""
    src, tgt, init, levels = R.multiscale_cases()[name]
    g = ctx.multiscale_icp_point_to_point(src, tgt, init, _multiscale_config(levels))
    r = R.run_multiscale(src, tgt, init, levels)
    report = _budget(g, lambda: r, lambda: R.run_multiscale(src, tgt, init, levels, exact_sums=True), src, tgt)
    print(name, report, g.iterations, r.iterations)
    assert (g.iterations, g.converged) == (r.iterations, r.converged)
    assert len(g.correspondences) == len(r.correspondences)


def test_multiscale_every_level_skipped(ctx):
    """no level has three voxels on both sides: an algorithm error (registration.rs:767-771), not a refinement from the init"""
    src, tgt = R.multiscale_pair()
    with pytest.raises(tc.AlgorithmError):
        ctx.multiscale_icp_point_to_point(src, tgt, None, _multiscale_config(R.MULTISCALE_ALL_COARSE))


# ---- batch ---------------------------------------------------------------------------------------------------------------------
def _jobs():
    return [tc.BatchICPJob(*j) for j in R.batch_jobs()]


def _identity(res):
    return np.array_equal(res.transformation, np.array([0, 0, 0, 1, 0, 0, 0], np.float32))


@pytest.fixture(scope="module")
def two_contexts():
    ctxs = [tc.GpuContext(0), tc.GpuContext(0)]
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.fixture(scope="module")
def single_calls():
    """every job of R.batch_jobs() through icp_point_to_point on a fresh context"""
    out = []
    for src, tgt, iters, thr, md in R.batch_jobs():
        c = tc.GpuContext(0)
        try:
            out.append(c.icp_point_to_point(src, tgt, None, iters, thr, md))
        finally:
            c.close()
    return out


def _same_as_single(b, single):
    return (b.status == 0 and np.array_equal(b.transformation, single.transformation) and b.final_error == single.mse
            and b.iterations == single.iterations)


def test_batch_mixed_jobs_over_two_contexts(two_contexts, single_calls):
    """five jobs, two contexts on one device: each result is the single call's bit for bit and within the budget of the oracle"""
    got = tc.gpu_batch_icp(two_contexts, _jobs())
    assert len(got) == 5
    for b, single, (src, tgt, iters, thr, md) in zip(got, single_calls, R.batch_jobs()):
        assert _same_as_single(b, single), (b, single)
        r = O.icp_point_to_point(src, tgt, None, iters, thr, md)
        report = _budget(b, lambda: r, lambda: O.icp_detailed(src, tgt, None, iters, md, thr, exact_sums=True), src, tgt)
        print(report, b.final_error, r.mse)
        assert b.iterations == r.iterations and single.converged == r.converged
        assert abs(b.final_error - r.mse) <= 1e-3 * max(r.mse, 1e-6)       # (the registration tests' bound on mse)


def test_batch_failing_job_between_good_ones(two_contexts, single_calls):
    """an empty source: its own non-zero status, the identity, zero iterations; the neighbours are what they are without it"""
    jobs = _jobs()
    bad = tc.BatchICPJob(np.zeros((0, 3), np.float32), jobs[0].target, 5, 1e-6, 0.5)
    got = tc.gpu_batch_icp(two_contexts, [jobs[0], jobs[1], bad, jobs[2], jobs[3]])
    assert got[2].status == tc._lib.TC_INVALID_DATA and _identity(got[2]) and got[2].iterations == 0
    for b, i in ((got[0], 0), (got[1], 1), (got[3], 2), (got[4], 3)):
        assert _same_as_single(b, single_calls[i]), (i, b)


def test_batch_degenerate_counts(two_contexts, single_calls):
    jobs = _jobs()
    one = tc.gpu_batch_icp(two_contexts, jobs[3:4])                         # fewer jobs than contexts
    assert len(one) == 1 and _same_as_single(one[0], single_calls[3])
    assert tc.gpu_batch_icp(two_contexts, []) == []                         # no job: TC_OK, nothing to return
    with pytest.raises(tc.InvalidData):
        tc.gpu_batch_icp([], jobs[:1])                                      # no context
