"""The statistical filter, the radius filter and cluster extraction on the MI355X at the cases of tests/filter_cases.py (what each
is there for is proved on the checkers alone in tests/test_filter_edges_cpu.py): a grid whose box the builder clamps, with pairs
and triples up to 10^6 box diagonals outside it, at every list size of sor_mean_kernel and both buffers of sor_mean_coop_kernel;
point counts either side of the blocks of every kernel, with inert rows; the statistics' partial sums at 255 / 256 / 257 blocks and
past 1 024; clouds 2^10 ... 2^16 from the origin; size windows that touch the component sizes; radii on and next to lattice shells.

Every case runs through the host road (numpy in) and the device road (a torch device tensor in).  mean_distance is compared bit
for bit (NaN as NaN), kept sets, n_out, labels, members and offsets exactly; the threshold by the rule of
test_gpu_outliers.py (one ulp from the exactly summed one, and the kept set = `mean <= threshold_used`).  No tolerance, no row left
out.  The profile rows of every call say that the intended passes ran, once."""
import ctypes as C_

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import _lib
from tests import cluster_checker as K
from tests import filter_cases as C
from tests import outlier_checker as OC

pytestmark = pytest.mark.gpu

CASES = C.cases()


def _of(op, family=None):
    return [c for c in CASES if c.op == op and (family is None or c.family == family)]


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()          # (the case inputs are read-only)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_host(a), np.float32).view(np.uint32)


def assert_same_floats(got, ref, what):
    got, ref = np.asarray(_host(got), np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, what
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows", np.nonzero(np.isnan(got) != nan)[0][:5])
    bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)) & ~nan)[0]
    assert len(bad) == 0, f"{what}: {len(bad)} means differ, first rows {bad[:5].tolist()}: got {got[bad[:5]]!r}, expected {ref[bad[:5]]!r}"


def _profiled(ctx, call):
    """the call's result and its tc_profile_read rows as {name: launches}"""
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        got = call()
        rows = {name: v[0] for name, v in ctx.profile_read().items()}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    return got, rows


def _check_kept(p, r, keep, what):
    idx = _host(r.index).astype(np.int64) & 0xFFFFFFFF
    assert len(idx) == len(keep), (what, "n_out", len(idx), len(keep))
    assert np.array_equal(idx, keep), (what, np.setxor1d(idx, keep)[:8])
    assert np.array_equal(_bits(r.points), p[idx].view(np.uint32)), what


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


# ---- the statistical filter ---------------------------------------------------------------------------------------------------------
def _sor_both_roads(ctx, c, mult):
    p, k = C.case_input(c), c.params[0]
    ref = C.ref_mean(c.cloud, k)
    t_f64 = OC.thresholds(ref, mult)[1]
    runs = []
    for road, arr in (("numpy", p), ("torch", _dev(p))):
        what = f"{C.case_id(c)} road {road} mult {mult}"
        r, rows = _profiled(ctx, lambda: ctx.statistical_outlier_removal_detailed(arr, k, mult))
        assert rows.get("sor_mean") == 1 and rows.get("sor_stats") == 1 and rows.get("sor_flag") == 1, (what, rows)
        assert_same_floats(r.mean_distance, ref, what)
        thr = np.float32(r.threshold)
        if np.isnan(t_f64):
            assert np.isnan(thr), what                                  # no finite point: nothing to average
        else:
            assert _ulps(thr, t_f64) <= 1, (what, thr, t_f64)
        _check_kept(p, r, OC.sor_keep(ref, thr), what)
        _check_kept(p, r, OC.sor_keep(_host(r.mean_distance), thr), what)       # ... and on the device's own returned bits
        runs.append(r)
    a, b = runs
    assert _ulps(a.threshold, b.threshold) == 0 or (np.isnan(a.threshold) and np.isnan(b.threshold))
    return a


@pytest.mark.parametrize("c", [c for c in _of("sor") if c.family != "shifted"], ids=C.case_id)
def test_mean_distance_to_the_bit(ctx, c):
    r = _sor_both_roads(ctx, c, 1.0)
    if c.cloud == ("clamped_far", True) and c.params[0] == 1:
        out = np.concatenate(C.clamped_far(True)[1])
        assert (_bits(r.mean_distance)[out] == _bits(np.sqrt(C.FAR_PAIR_D2))).all()     # an outlier's mean is its partner's distance


@pytest.mark.parametrize("c", _of("stats"), ids=C.case_id)
def test_threshold_at_the_block_counts_of_the_statistics(ctx, c):
    p, k = C.case_input(c), c.params[0]
    for mult in OC.SOR_MULTIPLIERS:
        a = _sor_both_roads(ctx, c, mult)
        b = ctx.statistical_outlier_removal_detailed(p, k, mult)             # two calls: the same bits
        assert np.array_equal(_bits(a.mean_distance), _bits(b.mean_distance)) and _ulps(a.threshold, b.threshold) == 0
        assert np.array_equal(_host(a.index), _host(b.index)) and np.array_equal(_bits(a.points), _bits(b.points))
        print(f"{C.case_id(c)} mult {mult}: blocks {C.stat_blocks(len(p))}, threshold_used {np.float32(a.threshold)!r}, kept {len(a.index)}")


# ---- the radius filter --------------------------------------------------------------------------------------------------------------
def _radius_both_roads(ctx, c):
    p, radius = C.case_input(c), c.params[0]
    counts = C.ref_counts(c.cloud, radius)
    kept = {}
    for m in C.radius_mins(c):
        keep = OC.keep_of_counts(counts, m)
        for road, arr in (("numpy", p), ("torch", _dev(p))):
            what = f"{C.case_id(c)} road {road} min_neighbors {m}"
            (out, idx), rows = _profiled(ctx, lambda: ctx.radius_outlier_removal(arr, radius, m, return_index=True))
            assert rows.get("radius_keep") == 1, (what, rows)
            _check_kept(p, tc.OutlierResult(out, idx), keep, what)
        kept[m] = keep
    return kept


@pytest.mark.parametrize("c", [c for c in _of("radius") if c.family != "shifted"], ids=C.case_id)
def test_radius_kept_sets(ctx, c):
    kept = _radius_both_roads(ctx, c)
    if c.cloud == ("clamped_far", True) and c.params[1] == (1, 2, 3):
        rows = C.clamped_far(True)[1]
        pairs, triples = (set(np.concatenate([r for r in rows if len(r) == s]).tolist()) for s in (2, 3))
        assert pairs <= set(kept[1].tolist()) and not pairs & set(kept[2].tolist())
        assert triples <= set(kept[2].tolist()) and not triples & set(kept[3].tolist())


# ---- cluster extraction -------------------------------------------------------------------------------------------------------------
def _cluster_both_roads(ctx, c):
    p, tol = C.case_input(c), c.params[0]
    got = {}
    for mn, mx in c.params[1]:
        el, em, eo = C.ref_clusters(c.cloud, tol, mn, mx)
        for road, arr in (("numpy", p), ("torch", _dev(p))):
            what = f"{C.case_id(c)} road {road} window ({mn}, {mx})"
            (labels, members, offsets), rows = _profiled(ctx, lambda: ctx.extract_euclidean_clusters_labels(arr, tol, mn, mx))
            labels, members, offsets = _host(labels).view(np.uint32), _host(members).view(np.uint32), _host(offsets).astype(np.uint64)
            nc = len(eo) - 1
            want = {"cluster_hook": 1, "cluster_compress": 1, "cluster_select": 1, "cluster_rank": int(nc > 0), "cluster_members": int(nc > 0)}
            assert {name: rows.get(name, 0) for name in want} == want, (what, rows)
            assert len(offsets) == len(eo), (what, "n_clusters", len(offsets) - 1, nc)
            assert np.array_equal(offsets, eo), what
            assert np.array_equal(labels, el), (what, int(np.count_nonzero(labels != el)), np.nonzero(labels != el)[0][:8])
            assert np.array_equal(members, em), what
        got[(mn, mx)] = el
    return got


@pytest.mark.parametrize("c", [c for c in _of("cluster") if c.family != "shifted"], ids=C.case_id)
def test_cluster_labels_members_offsets(ctx, c):
    _cluster_both_roads(ctx, c)


# ---- shifted: the checker at every shift, and the unmoved run's bits ---------------------------------------------------------------
def test_shifted_runs_equal_the_checker_and_the_unmoved_run(ctx):
    base = {}
    for c in _of("sor", "shifted") + _of("radius", "shifted") + _of("cluster", "shifted"):
        key = (c.op, c.params[0])
        if c.op == "sor":
            got = _bits(_sor_both_roads(ctx, c, 1.0).mean_distance)
        elif c.op == "radius":
            got = _radius_both_roads(ctx, c)
            got = np.concatenate([got[m] for m in sorted(got)])
        else:
            got = _cluster_both_roads(ctx, c)
            got = np.concatenate([got[w] for w in sorted(got)])
        if c.cloud[1] == 0.0:
            base[key] = got
        else:
            assert np.array_equal(got, base[key]), C.case_id(c)


# ---- the raw entry points: every subset of the outputs NULL ------------------------------------------------------------------------
def test_cluster_entry_points_with_null_outputs(ctx):
    """labels / members / offsets each wanted or NULL (members without offsets is refused: test_c_abi_status_and_message), at a window
    that keeps ten clusters and at (7, 7), which keeps none"""
    L = ctx._L
    p, _ = C.sized_components()
    n = len(p)
    x = _dev(p)
    for mn, mx in ((5, 6), (7, 7)):
        el, em, eo = C.ref_clusters(("sized",), C.SIZE_TOL, mn, mx)
        for road in ("host", "device"):
            fn = L.tc_extract_euclidean_clusters_device if road == "device" else L.tc_extract_euclidean_clusters
            for want_l, want_m, want_o in [(1, 1, 1), (1, 0, 1), (1, 0, 0), (0, 1, 1), (0, 0, 1), (0, 0, 0)]:
                def buf(count, dtype):
                    a = np.full(count, 0x55, dtype)
                    return _dev(a.view(np.int32 if dtype == np.uint32 else np.int64)) if road == "device" else a
                lab = buf(n, np.uint32) if want_l else None
                mem = buf(n, np.uint32) if want_m else None
                off = buf(n // mn + 1, np.uint64) if want_o else None
                ptr = lambda a: None if a is None else (a.data_ptr() if road == "device" else a.ctypes.data)
                n_cl = C_.c_size_t(99)
                torch.cuda.synchronize()
                rc = fn(ctx._h, x.data_ptr() if road == "device" else p.ctypes.data, n, C.SIZE_TOL, mn, mx, ptr(lab), ptr(mem), ptr(off), C_.byref(n_cl))
                what = (road, mn, mx, want_l, want_m, want_o)
                assert rc == _lib.TC_OK and n_cl.value == len(eo) - 1, what
                if want_l:
                    assert np.array_equal(_host(lab).view(np.uint32), el), what
                if want_o:
                    assert np.array_equal(_host(off).view(np.uint64)[:len(eo)], eo), what
                if want_m:
                    got = _host(mem).view(np.uint32)
                    assert np.array_equal(got[:len(em)], em), what
                    assert road == "device" or (got[len(em):] == 0x55).all(), what       # (the device road sorts all n indices into it)
