"""FPFH where fpfh_device() branches (tests/fpfh_cases.py; what every case is there for is proved on the checker alone in
tests/test_fpfh_edges_cpu.py): radii on and next to a lattice shell with k below, at and above the count; far outliers that clamp
the grid, with pairs and a triple among them; balls that hold the whole cloud (r^2 finite, above 3.0e38, infinite); more than k
duplicates of a point; k + 1 either side of every list size of the fallback search and k >= n; n at the block ends of the SPFH
(256 lanes) and sum (128 lanes) kernels with radius, fallback and inert points mixed; clouds 2^10 and 2^13 from the origin; and
more fallback points than one chunk of k-NN lists holds (2^25 entries), where the lists are searched a second time for the sums.

Every case runs through the host road (numpy in) and the device road (a torch device tensor in); the two are bit-equal, and the
compared rows go through F.compare with its 1e-5."""
import os
import re

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from tests import fpfh_cases as C
from tests import fpfh_checker as F

pytestmark = pytest.mark.gpu

CASES, CHUNKED, ALL_ZERO = C.cases(), C.chunked_cases(), C.all_zero_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the profile rows of fpfh_device() and of the k-NN launcher behind its fallback, as the library names them
SCOPES = set(re.findall(r'ProfScope ps\(ctx, "(\w+)"', open(os.path.join(ROOT, "threecrate_amd", "csrc", "fpfh.hip")).read()))
FALLBACK_ROWS = ("fpfh_knn_fallback", "knn_batch")


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _np6(pos, nrm):
    return np.ascontiguousarray(np.concatenate([pos, nrm], 1), np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def both_roads(ctx, c):
    """the descriptors of a case from the host road, after asserting that the device road gives the same bits"""
    pos, nrm, rows = C.case_input(c)
    c6 = _np6(pos, nrm)
    host = ctx.extract_fpfh_features_with_normals(c6, c.radius, c.k)
    dev = ctx.extract_fpfh_features_with_normals(torch.from_numpy(c6).to("cuda:0"), c.radius, c.k)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and host.shape == (len(pos), 33)
    assert np.array_equal(_bits(host), _bits(dev.cpu().numpy())), C.case_id(c)
    return host, pos, rows


@pytest.mark.parametrize("c", CASES, ids=C.case_id)
def test_case_matches_the_checker_on_both_roads(ctx, c):
    got, pos, rows = both_roads(ctx, c)
    ref = C.reference(c)
    F.compare(got if rows is None else got[rows], ref)
    inert = ~np.isfinite(pos).all(axis=1)
    assert (got[inert] == 0).all()
    if c.name == "identical":
        assert (got == 0).all()                                   # every pair is a skipped one
    if c.name == "two_sites":
        # the rows of one site are the same bits wherever the checker's are (the copies share position and normal; a copy's own list
        # leaves out another entry of the same plateau, and the walk meets the others in the same order)
        for site in (0, 1):
            mine = np.arange(site, 600, 2)
            want = _bits(ref["desc"][mine])
            assert (want == want[0]).all()
            assert (_bits(got[mine]) == _bits(got[mine[0]])).all(), site


@pytest.mark.parametrize("c", ALL_ZERO, ids=C.case_id)
def test_more_than_k_duplicates_everywhere_gives_zero_rows(ctx, c):
    """every point falls back and its k + 1 nearest are copies of itself, itself among them or not (the first-k branch of the
    fallback list): no valid pair, no weight, all-zero rows whichever copies the search names"""
    got, pos, _ = both_roads(ctx, c)
    assert (got == 0).all() and not np.signbit(got).any()


def test_translation(ctx):
    """parity at 2^10 and 2^13 from the origin is test_case_matches_the_checker_on_both_roads[shifted-*]; whether the bits equal the
    unmoved run's is printed, not asserted (the differences are exact, the walk's order may differ)"""
    runs = {c.name: both_roads(ctx, c)[0] for c in CASES if c.family == "shifted"}
    for name, got in runs.items():
        same = _bits(got) == _bits(runs["by0"])
        print(f"shifted {name}: {int(same.all(axis=1).sum())} of {len(got)} rows bit-equal to the unmoved run, "
              f"largest difference {float(np.abs(got - runs['by0']).max()):.3g}")


def _launches(ctx, call):
    ctx.profile_reset()
    call()
    rows = ctx.profile_read()
    return {name: rows.get(name, (0,))[0] for name in ("fpfh_spfh", "fpfh_sum") + FALLBACK_ROWS}


def test_the_intended_code_ran(ctx):
    """tc_profile_read rows (name, launches) of one call: the SPFH pass once, the fallback search once where some point falls back and
    not at all where the checker says none does.  Nothing visible tells fpfh_spfh_kernel<true> from <false>: that the clamped
    instantiation runs in far_pairs-clamped rests on search_checker.grid_box(), as in the search tests."""
    assert {"fpfh_spfh", "fpfh_sum", "fpfh_knn_fallback"} <= SCOPES
    picked = {}
    for c in CASES:
        if c.rows is None and c.family != "blocks":
            nl = C.reference(c)["nlist"]
            some, none = bool((nl < c.k).any() or np.isnan(c.radius)), bool((nl > c.k).all() or c.k == 0)
            if some or none:
                picked.setdefault((c.family, some), (c, some))
    # every point of x12 has its 11 copies in the ball: cnt >= k = 11 everywhere, cnt == k on the isolated sites -- `cnt < k` is false there
    at_k = [c for c in CASES if (c.family, c.name, c.k) == ("duplicates", "x12", 11)][0]
    assert (C.reference(at_k)["nlist"] == 11).any()
    picked[("cnt == k", False)] = (at_k, False)
    assert len({f for f, _ in picked}) >= 4 and {s for _, s in picked} == {True, False}
    ctx.profile_enable(True)
    try:
        for c, some in picked.values():
            pos, nrm, _ = C.case_input(c)
            c6 = _np6(pos, nrm)
            for arg in (c6, torch.from_numpy(c6).to("cuda:0")):
                got = _launches(ctx, lambda: ctx.extract_fpfh_features_with_normals(arg, c.radius, c.k))
                want = {"fpfh_spfh": 1, "fpfh_sum": 2 if some else 1, "fpfh_knn_fallback": int(some), "knn_batch": int(some)}
                assert got == want, (C.case_id(c), got, want)
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


@pytest.mark.parametrize("c", CHUNKED, ids=C.case_id)
def test_more_fallback_points_than_one_chunk_of_lists(ctx, c):
    """k = 31: a chunk is 2^20 lists.  mixed: 1 506 860 fallback points (test_fpfh_edges_cpu.py proves the count), two chunks, and the
    sums of the radius rows at the dense cube's top face read SPFH rows that the second chunk wrote; all_fallback: 2^20 + 1 points,
    the second chunk holds one query.  The fallback search runs once per chunk in each of the two passes."""
    pos, nrm, rows = C.case_input(c)
    c6 = _np6(pos, nrm)
    d6 = torch.from_numpy(c6).to("cuda:0")
    ctx.profile_enable(True)
    try:
        got = _launches(ctx, lambda: ctx.extract_fpfh_features_with_normals(d6, c.radius, c.k))
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    assert got == {"fpfh_spfh": 1, "fpfh_sum": 3, "fpfh_knn_fallback": 4, "knn_batch": 4}, got
    a = ctx.extract_fpfh_features_with_normals(d6, c.radius, c.k)
    b = ctx.extract_fpfh_features_with_normals(d6, c.radius, c.k)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))                    # two calls, the same bits
    assert bool(torch.isfinite(a).all()) and bool((a >= 0).all())
    sums = a.view(len(pos), 3, 11).sum(dim=2)
    assert bool(((sums == 0) | ((sums - 1.0).abs() <= 1e-4)).all())
    assert bool((a != 0).any(dim=1).all())                                           # every point is finite: no all-zero row
    host = ctx.extract_fpfh_features_with_normals(c6, c.radius, c.k)
    sample = a[torch.from_numpy(rows).to("cuda:0")].cpu().numpy()
    assert np.array_equal(_bits(host[rows]), _bits(sample))
    del a, b, host
    F.compare(sample, C.reference(c), min_strict=0.98)
