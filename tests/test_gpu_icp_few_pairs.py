"""Registration steps in which max_correspondence_distance keeps a handful of pairs out of a LARGE source.

The inputs come from tests/test_registration_inputs_cpu.py, which shows on the oracle alone that every case is usable (the f32
run, the exact_sums run and the same step in f64 agree to a third of the budget, one-ulp moves of the input move the step by
less than that, exact ties are rarer than the share of differing pairs allowed here) and carries the mutation evidence: sums of
f32 products of coordinates taken from the target's box centre end more than three budgets from the oracle on the "row5" and 3
cases.  The size of the source decides which kernels form the sums; the pairs, and so the expected step, do not depend on it.

The checks are those of tests/test_gpu_registration_variants.py: h1.transform_budget at test_gpu_parity's FROB_TOL with
scale = R.scale_of (1.0 for every case here), R.pairs_equal_or_tied, iterations == 1 and not converged, mse within
1e-3 max(mse, 1e-6) of the oracle's.
"""
import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import distributed as D

from oracle import oracle as O
from tests import h1
from tests import test_registration_inputs_cpu as R
from tests.test_gpu_parity import FROB_TOL
from tests.test_gpu_registration_variants import _kiss_compare, _multiscale_config

pytestmark = pytest.mark.gpu

assert FROB_TOL == R.FROB_TOL

_ORACLE = {}


def _oracle(case, max_iters=1):
    """the case and the oracle's run of it, computed once and shared (nothing below writes to either)"""
    key = (case, max_iters)
    if key not in _ORACLE:
        src, tgt, md = R.few_pairs_case(*case)
        _ORACLE[key] = (src, tgt, md, R.run_few(src, tgt, md, max_iters=max_iters))
    return _ORACLE[key]


def _check(g, case, label, max_iters=1, mse=None):
    """one result against the oracle's run of the case"""
    src, tgt, md, r = _oracle(case, max_iters)
    report = h1.transform_budget(g.transformation, lambda: r, lambda: R.run_few(src, tgt, md, True, max_iters=max_iters), FROB_TOL,
                                 scale=R.scale_of(src, tgt))
    g_mse = g.mse if mse is None else mse
    print(label, R.few_id(case), report, "mse", g_mse, r.mse)
    assert g.iterations == max_iters
    assert abs(g_mse - r.mse) <= 1e-3 * max(r.mse, 1e-6)
    return r


def _same_bits(a, b):
    return (np.array_equal(a.transformation, b.transformation) and a.mse == b.mse and a.iterations == b.iterations
            and a.converged == b.converged and np.array_equal(a.correspondences, b.correspondences))


# ---- plain point-to-point ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FEW_CASES, ids=R.few_id)
def test_one_step_matches_oracle(ctx, case):
    """kind x source size x placement through ctx.icp_detailed; a second run of the same call gives the same bits (the sums are
    folded in a fixed order)"""
    src, tgt, md, _ = _oracle(case)
    g = ctx.icp_detailed(src, tgt, None, 1, md, 0.0)
    r = _check(g, case, "host")
    assert not g.converged and len(g.correspondences) == R.few_pairs_count(case[0])
    R.pairs_equal_or_tied(src, tgt, O.IDENTITY, O.IDENTITY, g.correspondences, r.correspondences)
    assert _same_bits(ctx.icp_detailed(src, tgt, None, 1, md, 0.0), g)


@pytest.mark.parametrize("case", R.FEW_CASES, ids=R.few_id)
def test_one_step_device_inputs_equal_host_inputs(ctx, case):
    src, tgt, md, _ = _oracle(case)
    h = ctx.icp_detailed(src, tgt, None, 1, md, 0.0)
    d = ctx.icp_detailed(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), None, 1, md, 0.0)
    _check(d, case, "torch")
    assert _same_bits(d, h)


@pytest.mark.parametrize("case", R.FEW_CASES, ids=R.few_id)
def test_one_step_between_cloud_handles(ctx, case):
    src, tgt, md, _ = _oracle(case)
    s, t = tc.Cloud(ctx, src), tc.Cloud(ctx, tgt)
    try:
        g = s.icp_detailed(t, None, 1, md, 0.0, correspondences=True)
    finally:
        s.close()
        t.close()
    r = _check(g, case, "handle")
    assert not g.converged
    R.pairs_equal_or_tied(src, tgt, O.IDENTITY, O.IDENTITY, g.correspondences, r.correspondences)


@pytest.mark.parametrize("case", R.FEW_CASES, ids=R.few_id)
def test_one_step_sharded_on_one_rank(ctx, case):
    src, tgt, md, _ = _oracle(case)
    comm = D.Comm.local(ctx)
    try:
        g = D.sharded_icp_detailed(ctx, torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), None, 1, md, 0.0, comm=comm,
                                   correspondences=True)
    finally:
        comm.close()
    r = _check(g, case, "sharded")
    assert not g.converged
    R.pairs_equal_or_tied(src, tgt, O.IDENTITY, O.IDENTITY, g.correspondences, r.correspondences)


@pytest.fixture(scope="module")
def two_contexts():
    ctxs = [tc.GpuContext(0), tc.GpuContext(0)]
    yield ctxs
    for c in ctxs:
        c.close()


@pytest.mark.parametrize("case", [("row5", 4097, "spread"), (3, 20000, "block"), (64, 4097, "block")], ids=R.few_id)
def test_batch_job_between_two_ordinary_ones(two_contexts, case):
    """tc_batch_icp: a few-pairs job between two ordinary ones, one step each (the checked entry point wants a positive threshold;
    1e-30 stops no run after its first step: the first step's change is measured against an infinite previous mse).  A
    BatchICPResult carries the transform, the error, the iteration count and a status -- no pairs and no `converged` -- so those two
    checks of the other roads have nothing to look at here."""
    src, tgt, md, _ = _oracle(case)
    jobs = R.batch_jobs()
    mk = lambda j: tc.BatchICPJob(j[0], j[1], 1, 1e-30, j[4])
    got = tc.gpu_batch_icp(two_contexts, [mk(jobs[0]), tc.BatchICPJob(src, tgt, 1, 1e-30, md), mk(jobs[2])])
    assert [b.status for b in got] == [0, 0, 0]
    _check(got[1], case, "batch", mse=got[1].final_error)
    for b, j in ((got[0], jobs[0]), (got[2], jobs[2])):
        r = O.icp_point_to_point(j[0], j[1], None, 1, 1e-30, j[4])
        report = h1.transform_budget(b.transformation, lambda: r, lambda: O.icp_detailed(j[0], j[1], None, 1, j[4], 1e-30, exact_sums=True),
                                     FROB_TOL, scale=R.scale_of(j[0], j[1]))
        print("batch neighbour", report)
        assert b.iterations == r.iterations == 1 and abs(b.final_error - r.mse) <= 1e-3 * max(r.mse, 1e-6)


def test_three_steps_keep_the_five_pairs(ctx):
    """threshold 0, max_iters = 3 on the row5 case in a source of 4 097: the error of step 1 is not hidden by the later steps (the
    oracle's three steps pair the same five rows each time: shown in the inputs' module)"""
    case = ("row5", 4097, "spread")
    src, tgt, md, _ = _oracle(case, 3)
    g = ctx.icp_detailed(src, tgt, None, 3, md, 0.0)
    r = _check(g, case, "three steps", max_iters=3)
    assert not g.converged and len(g.correspondences) == 5
    g2 = ctx.icp_detailed(src, tgt, None, 2, md, 0.0)
    r2 = R.run_few(src, tgt, md, max_iters=2)
    R.pairs_equal_or_tied(src, tgt, g2.transformation, r2.transformation, g.correspondences, r.correspondences)


# ---- KISS-ICP and multiscale ICP -----------------------------------------------------------------------------------------------------
def test_kiss_large_down_sampled_source_five_pairs(ctx):
    """the voxel filter leaves 4 205 points, sigma pairs the five "row5" rows"""
    src, tgt = R.kiss_few_pairs_case()
    g, r = _kiss_compare(ctx, src, tgt, None)
    assert len(g.corr_target) == 4205 and len(g.correspondences) == 5


def _multiscale_few_pairs(ctx, kind):
    """the finest level and the final refinement see more than 4 096 source points and pair twenty well spread rows of them, or
    ("row5", both levels) only the five nearly collinear ones, where sums of uncentred f32 products show"""
    src, tgt, init, levels = R.multiscale_few_pairs_case(kind)
    g = ctx.multiscale_icp_point_to_point(src, tgt, init, _multiscale_config(levels))
    r = R.run_multiscale(src, tgt, init, levels)
    report = h1.transform_budget(g.transformation, lambda: r, lambda: R.run_multiscale(src, tgt, init, levels, exact_sums=True), FROB_TOL,
                                 scale=R.scale_of(src, tgt))
    print("multiscale", kind, report, g.iterations, r.iterations)
    assert (g.iterations, g.converged) == (r.iterations, r.converged)
    assert len(g.correspondences) == len(r.correspondences) == R.MULTISCALE_FEW_KINDS[kind][1]


def test_multiscale_large_finest_level_twenty_pairs(ctx):
    _multiscale_few_pairs(ctx, "twenty")


def test_multiscale_large_levels_row5_pairs(ctx):
    _multiscale_few_pairs(ctx, "row5")


# ---- point-to-plane --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.P2PLANE_FEW_PAIRS)
def test_point_to_plane_one_step_matches_oracle(ctx, m):
    """7, 12 and 64 pairs out of 4 097 source points, host and torch roads"""
    src, tgt, nrm, md = R.p2plane_few_case(m)
    r = R.run_p2plane_few(src, tgt, nrm, md)
    g = ctx.icp_point_to_plane_detailed(src, tgt, nrm, None, 1, md, 0.0)
    report = h1.transform_budget(g.transformation, lambda: r, lambda: R.run_p2plane_few(src, tgt, nrm, md, True), FROB_TOL, scale=R.scale_of(src, tgt))
    print("p2plane", m, report, "mse", g.mse, r.mse)
    assert g.iterations == 1 and not g.converged and len(g.correspondences) == m
    assert abs(g.mse - r.mse) <= 1e-3 * max(r.mse, 1e-6)
    R.pairs_equal_or_tied(src, tgt, O.IDENTITY, O.IDENTITY, g.correspondences, r.correspondences)
    d = ctx.icp_point_to_plane_detailed(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(nrm).cuda(), None, 1, md, 0.0)
    assert _same_bits(d, g)
