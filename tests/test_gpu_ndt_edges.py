"""NDT on the MI355X at the cases of tests/ndt_cases.py (what each is there for is proved on the checker alone in
tests/test_ndt_edges_cpu.py): points on and one float either side of voxel faces, as target and as source; keys saturated at
INT32_MAX / INT32_MIN, the 64-bit key box and the refused 65-bit one; sources either side of 262 144 points and past twice that; more
listed long runs than their launch has blocks; voxels of identical, collinear and coplanar points, min_points 0 and 1; the target's
own points as source through the dense and the hash table; non-finite source rows; the pair 2^10 and 2^13 from the origin, one step and loops of 3 to 35 iterations.

The yardstick is tests/ndt_checker.py with the header's keys (f32, true division, saturating) and f64 sums.  Keys, counts, n_voxels,
n_hits, iterations, converged and errors are exact.  The voxel map is held to the tight bound of ndt_cases.voxel_excess (one f32 ulp;
2^-40 of the largest element on top for inv_cov).  Pose and score are held to the project's rule, 4 x the reference's own f32-to-f64
distance on that input.  Every case runs through the host road (numpy in) and the device road (a torch device tensor in)."""
import ctypes as C_

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import _lib
from tests import ndt_cases as C
from tests import ndt_checker as NC

pytestmark = pytest.mark.gpu
F = np.float32


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()          # (the case inputs are read-only)


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_host(a), F).view(np.uint32)


ROADS = (("numpy", lambda a: np.array(a, copy=True)), ("torch", _dev))


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


# ---- the voxel map ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.of("voxels"), ids=C.case_id)
def test_voxel_map(ctx, c):
    cloud = C.case_input(c)[0]
    res, min_points, tight = c.params
    g = C.ref_voxels(c)
    outs = []
    for road, put in ROADS:
        keys, counts, mean, inv = [_host(x) for x in ctx.ndt_voxels(put(cloud), res, min_points)]
        what = f"{C.case_id(c)} ({road})"
        assert len(keys) == len(g[0]), (what, "n_voxels", len(keys), len(g[0]))
        assert np.array_equal(keys.astype(np.int64), g[0]), (what, "keys", np.nonzero((keys != g[0]).any(axis=1))[0][:5])
        assert np.array_equal(counts.astype(np.int64), g[1]), (what, "counts", np.nonzero(counts != g[1])[0][:5])
        assert np.isfinite(mean).all() and np.isfinite(inv).all(), what
        mask = None if tight else C.voxel_conds(g) <= C.COND_MAX
        em, ei = C.voxel_excess(mean, inv, g, mask)
        print(f"voxels {what}: V = {len(keys)}, mean {em:.2f} ulp, inv_cov {ei:.2f} x (one ulp + 2^-40 of the largest element)")
        assert em <= 1.0 and ei <= 1.0, (what, em, ei)
        if not tight:                                           # the far voxel's mean is still one ulp (256 there) from the yardstick's
            assert C.voxel_excess(mean, inv, g)[0] <= 1.0, what
        outs.append((keys, counts, mean, inv))
    for x, y in zip(*outs):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)), C.case_id(c)


def test_degenerate_voxels_have_the_closed_form(ctx):
    cloud, pts = C.degenerate(), C.scattered()
    order = np.lexsort(NC.keys_of(pts, 1.0, F).T[::-1])
    for road, put in ROADS:
        keys, counts, mean, inv = [_host(x) for x in ctx.ndt_voxels(put(cloud), 1.0, 5)]
        assert keys.tolist() == [[-3, 1, -2], [0, 0, 0], [2, 0, 0], [4, 0, 0]] and counts.tolist() == [5, 5, 5, 6], road
        for v in (0, 1):                                        # five identical points: cov = 0, inv_cov = 1e4 I
            assert (inv[v][[1, 2, 4]] == 0).all() and (np.abs(inv[v][[0, 3, 5]].astype(np.float64) - 1e4) <= C.ulp32(1e4)).all(), road
            same = cloud[(NC.keys_of(cloud, 1.0, F) == keys[v]).all(axis=1)]
            assert np.array_equal(_bits(mean[v]), _bits(same[0])), road
        for m in (0, 1):                                        # one point per voxel: the mean is the point
            keys, counts, mean, inv = [_host(x) for x in ctx.ndt_voxels(put(pts), 1.0, m)]
            assert len(keys) == len(pts) and (counts == 1).all() and np.array_equal(_bits(mean), _bits(pts[order])), (road, m)
            assert (inv[:, [1, 2, 4]] == 0).all() and (np.abs(inv[:, [0, 3, 5]].astype(np.float64) - 1e4) <= C.ulp32(1e4)).all(), (road, m)
        with pytest.raises(tc.AlgorithmError, match="Target point cloud has too few points for NDT voxel grid"):
            ctx.ndt_registration(put(pts), put(pts), None, min_points_per_voxel=len(pts) + 1)


# ---- registration -------------------------------------------------------------------------------------------------------------------------
def _register_both_roads(ctx, c):
    src, tgt, init = C.case_input(c)
    kw = C.loop_of(c)
    runs = []
    for road, put in ROADS:
        r, rows = _profiled(ctx, lambda: ctx.ndt_registration(put(src), put(tgt), init, **kw))
        assert rows.get("ndt_evaluate") == rows.get("ndt_finalize") and rows["ndt_evaluate"] >= r.iterations, (C.case_id(c), road, rows)
        runs.append((road, r, rows))
    (_, x, _), (_, y, _) = runs
    assert np.array_equal(_bits(x.transformation), _bits(y.transformation)) and _bits(x.score) == _bits(y.score), C.case_id(c)
    assert (x.iterations, x.converged, x.n_voxels, x.n_hits) == (y.iterations, y.converged, y.n_voxels, y.n_hits), C.case_id(c)
    return runs


@pytest.mark.parametrize("c", [c for c in C.of("register") if c.params["expect"] == "budget"], ids=C.case_id)
def test_registration_against_the_yardstick(ctx, c):
    a, b = C.ref_runs(c)
    bp, bs = C.budget(c)
    for road, r, rows in _register_both_roads(ctx, c):
        what = f"{C.case_id(c)} ({road})"
        fro, rel = NC.distances((r.transformation, r.score), b)
        print(f"{what}: pose {fro:.2e} (budget {bp:.2e}), score {rel:.2e} (budget {bs:.2e}), hits {r.n_hits} of {len(C.case_input(c)[0])}")
        assert (r.iterations, r.converged, r.n_voxels, r.n_hits) == (b["iterations"], b["converged"], b["n_voxels"], b["n_hits"]), what
        assert fro <= bp and rel <= bs, what
        assert rows["ndt_evaluate"] == b["iterations"], (what, rows)       # one launch per iteration: the grid-stride loop serves a long source


@pytest.mark.parametrize("c", [c for c in C.of("register") if c.params["expect"] == "own"], ids=C.case_id)
def test_own_points_score_one_each_through_both_tables(ctx, c):
    """d = 0 for the target's own points: e = 1, g = 0, the step is 0 < epsilon: converged at once with init's bits.  Nothing visible from
    Python names the table: the key box's cells choose it (tests/test_ndt_edges_cpu.py), and the two boxes are on either side"""
    src, tgt, init = C.case_input(c)
    k = NC.keys_of(tgt, C.OWN_RES, F)
    assert (np.prod((k.max(axis=0) - k.min(axis=0) + 1).astype(np.float64)) > C.DENSE_CELLS) == (c.name == "hash")
    for road, r, rows in _register_both_roads(ctx, c):
        what = f"{C.case_id(c)} ({road})"
        assert (r.n_hits, r.score, r.n_voxels) == (C.OWN_N, float(C.OWN_N), C.OWN_N), (what, r.n_hits, r.score)
        assert (r.iterations, r.converged) == (1, True) and np.array_equal(_bits(r.transformation), _bits(init)), what
        assert rows.get("ndt_table", 0) >= 1 and rows["ndt_evaluate"] == 5, (what, rows)       # the chunk of five was enqueued, one was used


def test_non_finite_source_rows_score_nothing(ctx):
    c = C.by_id("nonfinite_source-rows")
    src, tgt, init = C.case_input(c)
    twin = C.nonfinite_source(True)[0]
    b = C.ref_runs(c)[1]
    kw = C.loop_of(c)
    for road, r, _ in _register_both_roads(ctx, c):
        t = ctx.ndt_registration(dict(ROADS)[road](twin), dict(ROADS)[road](tgt), init, **kw)
        assert (r.iterations, r.converged, r.n_voxels) == (C.NONFINITE_ITERS, False, b["n_voxels"]) and r.n_hits == t.n_hits == b["n_hits"], (road, r.n_hits, t.n_hits)
        assert np.isfinite(r.transformation).all() and np.array_equal(_bits(r.transformation), _bits(t.transformation)) and _bits(r.score) == _bits(t.score), road


# ---- the refused key boxes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.of("unsupported"), ids=C.case_id)
def test_a_key_box_of_more_than_64_bits_is_unsupported_through_every_road(ctx, c):
    import threecrate_amd.compat as threecrate
    src, tgt, init = C.case_input(c)
    src, tgt = np.array(src), np.array(tgt)
    for road, put in ROADS:
        with pytest.raises(tc.Unsupported, match="more than 64 bits"):
            ctx.ndt_registration(put(src), put(tgt), init)
        with pytest.raises(tc.Unsupported, match="more than 64 bits"):
            ctx.ndt_voxels(put(tgt), 1.0)
    with pytest.raises(tc.Unsupported):
        tc.ndt_registration(src, tgt, init, tc.NdtConfig(), ctx=ctx)
    with pytest.raises(RuntimeError):
        threecrate.ndt_registration(threecrate.PointCloud(src), threecrate.PointCloud(tgt))
    L = ctx._L
    cfg = _lib.NdtConfigC(1.0, 0.1, 35, 1e-4, 5)
    ds, dt = _dev(src), _dev(tgt)
    torch.cuda.synchronize()
    for fn, s, t in ((L.tc_ndt_registration, src.ctypes.data, tgt.ctypes.data), (L.tc_ndt_registration_device, ds.data_ptr(), dt.data_ptr())):
        res = _lib.NdtResultC()
        res.score, res.iterations, res.n_hits = 7.0, 7, 7
        assert fn(ctx._h, s, len(src), t, len(tgt), init.ctypes.data, C_.byref(cfg), C_.byref(res)) == _lib.TC_UNSUPPORTED
        assert (res.iterations, res.score, res.n_hits) == (0, 7.0, 7)
    nv = C_.c_size_t(7)
    assert L.tc_ndt_voxels(ctx._h, tgt.ctypes.data, len(tgt), 1.0, 5, None, None, None, None, 0, C_.byref(nv)) == _lib.TC_UNSUPPORTED and nv.value == 0
    # and the context serves the next call
    ok = C.by_id("saturated-bits64")
    assert ctx.ndt_registration(*[np.array(x) for x in C.case_input(ok)], max_iterations=1).n_hits == C.ref_runs(ok)[1]["n_hits"]
