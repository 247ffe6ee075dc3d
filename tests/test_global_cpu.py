"""Descriptor matching and RANSAC over correspondences without a GPU: the numpy checker (tests/global_checker.py) against the
reference's own unit tests where they concern these two steps, the closed form of the winner rule against the literal loop, the draw
mapping and the LCG jump-ahead, the companion library's validation (which comes before any device work), the facades' surface -- and,
for every input of tests/test_gpu_global.py, the proof that it contains what it is there for and which checker mutant it tells apart."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import global_checker as G

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "threecrate_hip_global.h"


# ---- the reference's unit tests (global_registration.rs:339 onward) where they concern these two steps ----
def test_estimate_transform_svd_three_points():
    """:434-450: a pure shift of three points comes back as that shift"""
    src = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F)
    r, t, _, _ = G.model(src, src + F((1, 2, 3)))
    assert np.abs(t - (1, 2, 3)).max() < 1e-4 and np.abs(r - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(r) - 1) < 1e-12


def test_config_defaults_are_the_references():
    """:453-459 and :48-62"""
    import threecrate_amd as tc
    c = tc.GlobalRegistrationConfig()
    assert (c.ransac_iterations, c.distance_threshold, c.inlier_ratio, c.fpfh_radius, c.fpfh_k_neighbors, c.normal_k_neighbors, c.refine_with_icp,
            c.icp_max_iterations, c.icp_distance_threshold, c.seed) == (50_000, 0.05, 0.25, 0.25, 10, 10, True, 50, None, 0)


def test_identical_descriptor_sets_match_themselves_and_every_pair_is_an_inlier():
    """:384-397 on the two steps: the same cloud twice gives the identity correspondences, and any model from them counts every pair"""
    rng = np.random.default_rng(0)
    d, pts = rng.random((40, G.DIM), F), rng.random((40, 3), F)
    idx, dist = G.match(d, d)
    assert np.array_equal(idx, np.arange(40)) and (dist == 0).all()
    r = G.ransac(pts, pts, np.arange(40), idx, 0.5, 0.25, G.lcg_triples(40, 20))
    assert r["inlier_count"] == 40 and r["early_exit"] and r["iterations_run"] == 1 and r["inlier_ratio"] == 1


def test_a_reflection_is_fixed_and_a_model_is_a_rotation():
    rng = np.random.default_rng(1)
    for _ in range(50):
        s, t = rng.random((3, 3), F), rng.random((3, 3), F)
        r = G.model(s, t)[0]
        assert abs(np.linalg.det(r) - 1) < 1e-9 and np.abs(r @ r.T - np.eye(3)).max() < 1e-9


# ---- winner: the closed form is the loop ----
def test_closed_form_of_the_winner_rule_equals_the_literal_loop():
    rng = np.random.default_rng(2)
    seen = set()
    for trial in range(3000):
        n = int(rng.integers(1, 40))
        counts = rng.integers(0, int(rng.integers(1, 12)), n)               # small ranges: plateaus
        valid = rng.random(n) < 0.8
        E = int(rng.integers(3, 14))
        a, b = G.winner(counts, valid, E), G.winner_closed(counts, valid, E)
        assert a == b, (counts, valid, E)
        seen.add((a[0], a[3]))
    assert seen == {(False, False), (True, False), (True, True)}            # nothing wins, E not reached, E reached


def test_exit_count_is_the_f32_ceiling_saturated():
    assert G.exit_count(0.25, 200) == 50 and G.exit_count(0.25, 201) == 51 and G.exit_count(0.0, 10) == 3 and G.exit_count(-1.0, 10) == 3
    assert G.exit_count(float("nan"), 10) == 3 and G.exit_count(float("inf"), 10) == (1 << 64) - 1 and G.exit_count(2.0, 65) == 130
    assert G.exit_count(0.1, 16777217) == int(np.ceil(F(0.1) * F(16777217)))       # m as f32 first


# ---- samples ----
@pytest.mark.parametrize("m", [3, 4, 5, 1000])
def test_draw_mapping_never_repeats_an_index(m):
    t = G.lcg_triples(m, 3000, seed=m)
    assert t.max() < m and (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    if m <= 5:                                                              # and every ordered triple of distinct indices can come up
        assert len({tuple(r) for r in t.tolist()}) == m * (m - 1) * (m - 2)
    rng = np.random.default_rng(m)
    for r in rng.integers(0, 1 << 32, (2000, 3)).tolist():
        assert len(set(G.map_draws(*r, m))) == 3


def test_lcg_jump_ahead_equals_the_recurrence():
    s0 = G.state0(1000, 50_000, 12345)
    assert s0 == ((1000 << 32) ^ 50_000 ^ G.GOLDEN) ^ 12345
    s, states = s0, [s0]
    for _ in range(400):
        s = (s * G.LCG_MULT + G.LCG_INC) & G.MASK
        states.append(s)
    for steps in (0, 1, 2, 3, 6, 7, 64, 399, 400):
        mult, inc = G.lcg_jump(steps)
        assert (s0 * mult + inc) & G.MASK == states[steps]
    t, s0 = G.lcg_triples(1000, 100, 12345), G.state0(1000, 100, 12345)       # (max_iters is part of the initial state)
    for it in (0, 1, 50, 99):                                               # an iteration from its own jump, as the device does it
        mult, inc = G.lcg_jump(3 * it)
        s, r = (s0 * mult + inc) & G.MASK, []
        for _ in range(3):
            s = (s * G.LCG_MULT + G.LCG_INC) & G.MASK
            r.append(s >> 32)
        assert tuple(t[it]) == G.map_draws(*r, 1000)


# ---- the companion library: validation before any device work ----
def _lib_global():
    return _lib.load_companion(HEADER)


def test_null_context_calls_are_invalid_data_and_write_nothing():
    L = _lib_global()
    buf = np.full(64, 7, np.uint32)
    T, r = (C.c_float * 12)(*([7.0] * 12)), _lib.RansacResultC(7, 7, 7, 7, 7.0)
    p = buf.ctypes.data
    for fn in (L.tc_match_features, L.tc_match_features_device):
        assert fn(None, p, 4, p, 4, 33, p, p) == _lib.TC_INVALID_DATA
        assert fn(None, p, 0, p, 4, 33, p, p) == _lib.TC_INVALID_DATA
    for fn in (L.tc_ransac_correspondences, L.tc_ransac_correspondences_device):
        assert fn(None, p, 4, p, 4, p, p, 4, 0.1, 0.25, 10, 0, T, C.byref(r), None, None) == _lib.TC_INVALID_DATA
    for fn in (L.tc_ransac_correspondences_samples, L.tc_ransac_correspondences_samples_device):
        assert fn(None, p, 4, p, 4, p, p, 4, 0.1, 0.25, p, 10, T, C.byref(r), None, None) == _lib.TC_INVALID_DATA
    assert (buf == 7).all() and list(T) == [7.0] * 12 and (r.inlier_count, r.iterations_run, r.best_iteration, r.early_exit) == (7, 7, 7, 7)


def test_companion_refuses_another_build_of_the_product_library(monkeypatch):
    monkeypatch.setattr(_lib, "LIB_PATH", os.path.join(ROOT, "threecrate_amd", "variants", "libthreecrate_hip_dev.so"))
    monkeypatch.setattr(_lib, "_companion_libs", {})
    with pytest.raises(ImportError, match="TC_HIP_LIB"):
        _lib.load_companion(HEADER)


def test_the_companion_finds_the_product_library_beside_itself():
    out = os.popen(f"readelf -d {os.path.join(ROOT, 'threecrate_amd', 'libthreecrate_hip_global.so')}").read()
    assert re.search(r"NEEDED.*\[libthreecrate_hip\.so\]", out) and re.search(r"(RUNPATH|RPATH).*\$ORIGIN", out)
    mk = open(os.path.join(ROOT, "threecrate_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all: .*\$\(GLOBAL_OUT\)", mk, re.M) and "global.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


# ---- the facades ----
def test_python_surface():
    import threecrate_amd as tc
    import threecrate_amd.compat as threecrate
    sig = inspect.signature(tc.GpuContext.match_features).parameters
    assert list(sig)[1:] == ["src_desc", "tgt_desc", "return_distance"] and sig["return_distance"].default is False
    sig = inspect.signature(tc.GpuContext.ransac_correspondences).parameters
    assert list(sig)[1:] == ["source", "target", "corr_src", "corr_tgt", "threshold", "inlier_ratio", "max_iterations", "seed", "samples", "candidates"]
    assert [sig[k].default for k in list(sig)[6:]] == [0.25, 50_000, 0, None, False]
    sig = inspect.signature(tc.GpuContext.global_registration).parameters
    assert list(sig)[1:] == ["source", "target", "config", "source_normals", "target_normals"]
    for name in ("GlobalRegistrationConfig", "GlobalRegistrationResult", "RansacResult", "global_registration", "global_registration_with_normals"):
        assert hasattr(tc, name) and name in tc.__all__, name
    assert [f for f in tc.GlobalRegistrationResult.__dataclass_fields__][:4] == ["transformation", "inlier_count", "inlier_ratio", "icp_result"]
    # the wheel's parameters and defaults (threecrate-python/src/lib.rs:1026-1049, :1090-1114)
    names = ["ransac_iterations", "distance_threshold", "inlier_ratio", "fpfh_radius", "fpfh_k_neighbors", "normal_k_neighbors", "refine_with_icp",
             "icp_max_iterations"]
    defaults = [50_000, 0.05, 0.25, 0.25, 10, 10, True, 50]
    sig = inspect.signature(threecrate.global_registration).parameters
    assert list(sig) == ["source", "target"] + names and [sig[k].default for k in names] == defaults
    sig = inspect.signature(threecrate.global_registration_with_normals).parameters
    assert list(sig) == ["source_normals", "target_normals", "source", "target"] + names and [sig[k].default for k in names] == defaults
    for name in ("global_registration", "global_registration_with_normals", "GlobalRegistrationResult"):
        assert name in threecrate.__all__
    rr = tc.RansacResult(G.IDENTITY12.copy(), 5, 0.5, 10, 3, False)
    res = threecrate.GlobalRegistrationResult(tc.GlobalRegistrationResult(tc.rotation_to_isometry(rr.transform), 5, 0.5, None, rr))
    assert repr(res) == "GlobalRegistrationResult(inliers=5, ratio=0.500)" and res.icp_mse is None and res.icp_converged is None
    assert np.array_equal(res.transformation(), np.eye(4, dtype=F)) and res.transformation().dtype == F


def test_rotation_to_isometry_round_trips_through_every_branch():
    import threecrate_amd as tc
    rng = np.random.default_rng(4)
    axes = [rng.normal(size=3) for _ in range(40)] + [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    for axis in axes:
        for angle in (0.0, 0.3, 2.0, np.pi - 1e-3, np.pi):
            r = G.rot(axis, angle)
            T = tc.rotation_to_isometry(np.concatenate([r.reshape(9), (1, 2, 3)]))
            assert np.abs(tc.isometry_to_matrix(T)[:3, :3] - r).max() < 1e-6 and list(T[4:]) == [1, 2, 3]


def test_rust_facade_has_the_reference_names():
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ("global_registration", "global_registration_with_normals", "match_features", "ransac_correspondences"):
        assert re.search(r"^pub fn " + fn + r"\(", lib_rs, re.M), fn
    for st in ("GlobalRegistrationConfig", "GlobalRegistrationResult"):
        assert re.search(r"^pub struct " + st + r"\b", lib_rs, re.M), st
    build = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "build.rs")).read()
    assert "threecrate_hip_global" in build


def test_constants_are_the_ones_the_tests_name():
    src = open(os.path.join(ROOT, "threecrate_amd", "csrc", "global.hip")).read()
    val = lambda name: int(re.search(r"constexpr int " + name + r" = (\d+);", src).group(1))
    assert (val("kMatchSrcPerBlock"), val("kMatchTgtTile"), val("kRansacCandTile"), val("kRansacChunk")) == (
        G.MATCH_SRC_PER_BLOCK, G.MATCH_TGT_TILE, G.CAND_TILE, G.CHUNK)
    assert val("kRansacBlock") * val("kRansacPerLane") == G.PAIRS_PER_BLOCK
    hdr = open(os.path.join(ROOT, "include", HEADER)).read()
    assert "#define TC_RANSAC_MAX_ITERS ((size_t)1 << 20)" in hdr and _lib.TC_RANSAC_MAX_ITERS == G.MAX_ITERS and "chunks of 4096" in hdr


# ---- what every GPU input is there for, by the checker alone ----
def test_match_inputs_contain_what_they_are_there_for():
    T = G.MATCH_TGT_TILE
    src, tgt = G.match_case("int", 65, 2 * T + 1)
    d = G.distances(src, tgt)
    idx, dist = G.match(src, tgt)
    ties = (d == dist[:, None]).sum(1)
    assert (ties > 1).sum() >= 10                                           # genuine ties, in many rows
    assert idx[0] == T - 1 and dist[0] == 1 and d[0, T] == 1 and d[0, T + 5] == 1            # the planted tie spans the tile boundary
    src, tgt = G.match_case("nan0", 65, 2 * T + 1)
    idx, dist = G.match(src, tgt)
    assert (idx == 0).all() and np.isnan(dist).all()                        # the NaN incumbent is never replaced
    src, tgt = G.match_case("nanmid", 65, 2 * T + 1)
    idx, dist = G.match(src, tgt)
    assert np.isnan(tgt[T + T // 2]).any() and (idx != T + T // 2).all() and np.isfinite(dist).all()
    src, tgt = G.match_case("equal", 65, 2 * T + 1)
    assert (G.match(src, tgt)[0] == 0).all()
    assert {ns for ns, _ in G.MATCH_SIZES} == set(G.MATCH_NS) and {nt for _, nt in G.MATCH_SIZES} == set(G.MATCH_NT)


def test_model_inputs_are_well_conditioned_and_the_degenerate_rows_have_no_model():
    src, tgt, corr, smp, n_good = G.model_case()
    for row in smp[:n_good].astype(np.int64):
        assert G.singular_ratio(src[row], tgt[row]) >= 0.05 and src[row].min() >= 0 and src[row].max() <= 1
    T, valid = G.models(src, tgt, smp)
    assert valid[:n_good].all() and not valid[n_good:].any() and len(smp) == n_good + 4
    base = int(smp[n_good + 2, 0])
    assert G.singular_ratio(src[base:base + 3], tgt[base:base + 3]) < 1e-12 # exactly collinear: rounding noise, seven orders below the 1e-9 of the contract
    # the fits are least-squares fits, not exact ones: the residual is the noise's
    r, t, _, _ = G.model(src[:3], tgt[:3])
    assert 1e-4 < np.abs(src[:3].astype(np.float64) @ r.T + t - tgt[:3]).max() < 0.1


def _ulps_from_threshold(d2, thr):
    thr2 = F(thr) * F(thr)
    with np.errstate(invalid="ignore"):
        return np.nanmin(np.abs(d2.astype(np.float64) - np.float64(thr2))) / np.float64(np.spacing(thr2))


@pytest.fixture(scope="module")
def winner_runs():
    src, tgt, corr = G.winner_pairs()
    runs = {}
    for name in G.WINNER_CASES + ["tie_across_chunks"]:
        smp = G.tie_case() if name == "tie_across_chunks" else G.winner_case(name)
        ratio = 0.9 if name in ("tie_across_chunks", "no_exit") else G.WINNER_RATIO
        runs[name] = (smp, ratio, G.ransac(src, tgt, corr, corr, G.WINNER_THRESHOLD, ratio, smp))
    return runs


def test_winner_inputs_contain_what_they_are_there_for(winner_runs):
    src, tgt, corr = G.winner_pairs()
    ps, pt = G.gather(src, tgt, corr, corr)
    assert G.exit_count(G.WINNER_RATIO, G.WINNER_M) == 50 and G.exit_count(0.9, G.WINNER_M) == 180
    expect = {"exit_first_chunk": (77, True, 78), "exit_chunk_last_row": (G.CHUNK - 1, True, G.CHUNK), "two_exits": (300, True, 301),
              "exit_second_chunk_first_row": (G.CHUNK, True, G.CHUNK + 1), "tie_across_chunks": (300, False, 2 * G.CHUNK + 1),
              "nothing_wins": (0, False, 2 * G.CHUNK + 1)}
    for name, (smp, ratio, r) in winner_runs.items():
        assert len(smp) == 2 * G.CHUNK + 1
        if name in expect:
            assert (r["best_iteration"], r["early_exit"], r["iterations_run"]) == expect[name], name
        # no pair within 4 f32 ulps of the threshold under the checker's own models
        assert _ulps_from_threshold(G.d2_all(r["cand_transform"][r["valid"]], ps, pt), G.WINNER_THRESHOLD) > 4 if r["valid"].any() else True
    r = winner_runs["tie_across_chunks"][2]
    c = r["cand_count"]
    assert c[300] == c[G.CHUNK + 9] == c.max() == G.WINNER_INLIERS and (c == c.max()).sum() == 2           # equal bests in two chunks
    r = winner_runs["no_exit"][2]
    assert r["inlier_count"] == G.WINNER_INLIERS < 180 and not r["early_exit"] and r["best_iteration"] == G.CHUNK + 904      # E is not reached
    r = winner_runs["nothing_wins"][2]
    assert not r["valid"].any() and r["inlier_count"] == 0 and np.array_equal(r["transform"], G.IDENTITY12)
    for name in ("exit_first_chunk", "exit_chunk_last_row", "exit_second_chunk_first_row", "two_exits"):
        assert winner_runs[name][2]["inlier_count"] == G.WINNER_INLIERS


def test_score_inputs_contain_what_they_are_there_for():
    assert {m for m, _ in G.SCORE_SIZES} == set(G.SCORE_M) and {n for _, n in G.SCORE_SIZES} == set(G.SCORE_CAND)
    src, tgt, cs, ct, smp = G.score_case(65, 129)
    ps, pt = G.gather(src, tgt, cs, ct)
    assert np.isnan(ps).any(1).sum() == 3 and (cs == G.NONE).sum() == 1 and (ct == len(tgt)).sum() == 1     # pairs that are never counted
    r = G.ransac(src, tgt, cs, ct, G.SCORE_THRESHOLD, 2.0, smp)
    assert not r["valid"][2] and not r["valid"][5] and r["valid"].sum() > 100 and not r["early_exit"]
    assert len(np.unique(r["cand_count"])) > 10 and r["cand_count"].max() < 65                              # counts that vary
    assert _ulps_from_threshold(G.d2_all(r["cand_transform"][r["valid"]], ps, pt), G.SCORE_THRESHOLD) > 4


def test_every_mutant_is_told_apart_by_some_gpu_input_or_shown_equivalent(winner_runs):
    table = {}
    T = G.MATCH_TGT_TILE
    for mutant in G.MATCH_MUTANTS:
        hits = []
        for kind in ("int", "nan0", "equal"):
            src, tgt = G.match_case(kind, 65, 2 * T + 1)
            if not np.array_equal(G.match(src, tgt)[0], G.match(src, tgt, mutant)[0]):
                hits.append(kind)
        table[mutant] = hits
    src, tgt, corr = G.winner_pairs()
    ps, pt = G.gather(src, tgt, corr, corr)
    # d2 <= thr^2: the ulp-by-ulp test puts the threshold's square ON a pair's d2, where < and <= differ by that pair
    s2, t2, cs, ct, smp = G.score_case(65, 129)
    r = G.ransac(s2, t2, cs, ct, G.SCORE_THRESHOLD, 2.0, smp)
    p2s, p2t = G.gather(s2, t2, cs, ct)
    c = int(np.nonzero(r["valid"])[0][0])
    d2 = G.d2_all(r["cand_transform"][c], p2s, p2t)[0]
    p = int(np.nanargmin(np.abs(d2 - F(0.09))))
    thr = F(np.sqrt(d2[p]))
    while thr * thr < d2[p]:
        thr = np.nextafter(thr, F(np.inf))
    while np.nextafter(thr, F(0)) * np.nextafter(thr, F(0)) >= d2[p]:
        thr = np.nextafter(thr, F(0))
    good, bad = G.score(r["cand_transform"][c], p2s, p2t, thr)[0], G.score(r["cand_transform"][c], p2s, p2t, thr, "lt_for_le")[0]
    table["lt_for_le"] = ["threshold ulp by ulp"] if (thr * thr == d2[p] and good == bad + 1) else []
    for mutant in G.WINNER_MUTANTS:
        hits = []
        for name, (smp, ratio, r) in winner_runs.items():
            m = G.winner(r["cand_count"], r["valid"], G.exit_count(ratio, G.WINNER_M), mutant)
            if m != G.winner(r["cand_count"], r["valid"], G.exit_count(ratio, G.WINNER_M)):
                hits.append(name)
        table[mutant] = hits
    for mutant, hits in table.items():
        print(f"{mutant:28s} differs on {hits}")
    # the exit at the first count >= E without the strict-best test is the same rule: the best is below E until the loop stops, so the
    # first count that reaches E is a new best.  No input can tell it apart, here or anywhere
    assert table.pop("exit_without_strict_best") == []
    rng = np.random.default_rng(9)
    for _ in range(2000):
        n = int(rng.integers(1, 30))
        counts, valid, E = rng.integers(0, 9, n), rng.random(n) < 0.8, int(rng.integers(3, 10))
        assert G.winner(counts, valid, E, "exit_without_strict_best") == G.winner(counts, valid, E)
    assert all(table.values()), [m for m, h in table.items() if not h]
    assert "tie_across_chunks" in table["last_of_equal"] and "two_exits" in table["exit_ignored"]


# ---- the pose-recovery case: the checker chain ends inside ICP's basin ----
def test_the_checker_chain_ends_inside_the_basin_of_icp_on_the_pose_case():
    """fpfh_checker -> match -> winner on global_checker.pose_case() with POSE_SEED: under the chain's transform every source point's nearest
    target point is its own image, so the first point-to-point ICP step is the Kabsch fit over the true pairs; under the identity none is,
    and the oracle's point-to-point ICP from the identity converges to another pose, while from the chain's pose it ends on the planted one
    within the bound the GPU test uses.  The planted motion is a rigid one and the clouds are each other's images to f32 rounding."""
    src, tgt, sn, tn, planted = G.pose_case()
    assert len(src) == G.POSE_N == 2000 and abs(np.linalg.det(planted[:3, :3]) - 1) < 1e-12
    back = src.astype(np.float64) @ planted[:3, :3].T + planted[:3, 3]
    assert np.abs(back - tgt).max() < 4e-7                                              # f32 rounding of coordinates below 2
    assert np.abs(sn.astype(np.float64) @ planted[:3, :3].T - tn).max() < 4e-7 and np.abs(np.linalg.norm(tn, axis=1) - 1).max() < 1e-6
    r, share = G.pose_chain()
    print(f"correct matches {share:.4f}, inliers {r['inlier_count']}, winner {r['best_iteration']}, exit {r['early_exit']}")
    assert share > 0.9 and r["early_exit"] and r["inlier_count"] >= G.exit_count(0.25, G.POSE_N)
    assert G.partners_are_nearest(r["transform"], src, tgt) == 1.0
    assert G.partners_are_nearest(G.IDENTITY12, src, tgt) < 0.01
    # asymmetric: the descriptors of the two halves of the surface do not match each other (a mirrored start would be another basin)
    T = r["transform"].astype(np.float64)
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = T[:9].reshape(3, 3), T[9:]
    assert np.linalg.norm(m - planted) < 1e-3
    import threecrate_amd as tc
    from oracle import oracle as O
    from tests.test_gpu_parity import FROB_TOL
    frob = lambda res: np.linalg.norm(O.isometry_to_matrix(res.transformation).astype(np.float64) - planted)
    alone = O.icp_point_to_point(src, tgt, None, 50, 1e-6, None)
    refined = O.icp_point_to_point(src, tgt, tc.rotation_to_isometry(r["transform"]), 50, 1e-6, None)
    print(f"oracle ICP from the identity: {frob(alone):.3f} from the planted pose; from the chain's pose: {frob(refined):.3e} (bound {FROB_TOL:.0e})")
    assert frob(alone) > 1.0 and frob(refined) <= FROB_TOL
