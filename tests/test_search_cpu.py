"""The inputs of tests/test_gpu_search_edges.py prove themselves without a GPU: on every family (a) the oracle's own answers --
the kd-tree (O.knn_batch, O.KdTree.find_radius_neighbors) and O.brute_knn -- pass tests/search_checker.py, so the checker agrees
with the reference; (b) the properties the family is there for hold; (c) the mutants of a correct answer fail the checker.

The reference's kd-tree has no rule for a query with a NaN or infinite coordinate (its comparisons visit whatever nodes come first
and return NaN distances); the backend's rule is "no neighbours", so the oracle is asked the finite queries only and the others'
counts are set to 0 here."""
import numpy as np
import pytest

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from tests import search_checker as S  # noqa: E402

KNN_CASES, MANY_CASES, RADIUS_ALL_CASES = S.knn_cases(), S.many_query_cases(), S.radius_all_cases()
FAMILIES = sorted({c.family for c in KNN_CASES})


def oracle_answer(c):
    """the kd-tree's (idx, dist, count) for a case: find_k_nearest, with a radius cut to the entries within it the way
    gpu_find_radius_neighbors truncates find_radius_neighbors to the k_max nearest"""
    pts, qs, b = S.case_input(c)
    fin = b.qfin
    idx, dist, cnt = np.zeros((len(qs), c.k), np.uint64), np.zeros((len(qs), c.k), np.float32), np.zeros(len(qs), np.uint32)
    idx[fin], dist[fin], cnt[fin] = O.knn_batch(pts, qs[fin], c.k)
    if c.radius is not None:
        r2 = S.radius_sq(c.radius)
        d2 = np.take_along_axis(b.d2, idx.astype(np.int64), axis=1)
        cnt = np.where(fin, ((d2 <= r2) & (np.arange(c.k)[None, :] < cnt[:, None])).sum(axis=1), 0) if r2 is not None else cnt * 0
    return idx, dist, cnt


@pytest.mark.parametrize("c", KNN_CASES + MANY_CASES[3::4], ids=S.case_id)
def test_kdtree_answer_passes_the_checker(c):
    pts, qs, b = S.case_input(c)
    rep = S.check_knn(pts, qs, c.k, *oracle_answer(c), c.radius, brute=b)
    assert rep.queries == len(qs)


@pytest.mark.parametrize("c", [c for c in KNN_CASES if c.radius is not None and c.family != "no_radius"][::2], ids=S.case_id)
def test_kdtree_radius_answer_passes_the_checker(c):
    """find_radius_neighbors itself (not find_k_nearest cut at the radius), truncated to the k_max nearest, on every 13th query"""
    pts, qs, b = S.case_input(c)
    sel = np.nonzero(b.qfin)[0][::13]
    tree = O.KdTree(pts)
    idx, dist, cnt = np.zeros((len(sel), c.k), np.int64), np.zeros((len(sel), c.k), np.float32), np.zeros(len(sel), np.int64)
    for row, t in enumerate(sel):
        oi, od = tree.find_radius_neighbors(qs[t], c.radius)
        m = min(len(oi), c.k)
        idx[row, :m], dist[row, :m], cnt[row] = oi[:m], od[:m], m
    S.check_knn(pts, qs[sel], c.k, idx, dist, cnt, c.radius, brute=b.rows(sel))


@pytest.mark.parametrize("family", FAMILIES)
def test_brute_force_oracle_passes_the_checker(family):
    """BruteForceSearch::find_k_nearest on the first and the last case of the family, every 29th finite query.  It sorts by the
    rounded distances, so among points whose d2 differ by an ulp and whose sqrt agree it may keep the farther one
    (ranked_by="dist"); test_brute_force_oracle_ranks_by_distance shows the case."""
    for c in [c for c in KNN_CASES if c.family == family and c.radius is None][::len(KNN_CASES)] + [c for c in KNN_CASES if c.family == family and c.radius is None][-1:]:
        pts, qs, b = S.case_input(c)
        sel = np.nonzero(b.qfin)[0][::29]
        idx, dist, cnt = np.zeros((len(sel), c.k), np.int64), np.zeros((len(sel), c.k), np.float32), np.zeros(len(sel), np.int64)
        for row, t in enumerate(sel):
            oi, od = O.brute_knn(pts, qs[t], c.k)
            idx[row, :len(oi)], dist[row, :len(oi)], cnt[row] = oi, od, len(oi)
        S.check_knn(pts, qs[sel], c.k, idx, dist, cnt, brute=b.rows(sel), ranked_by="dist")


def test_brute_force_oracle_ranks_by_distance():
    """placed queries, k = 300: where two d2 one ulp apart share a square root at the cut, BruteForceSearch keeps the lower
    INDEX, the kd-tree the lower d2.  Only the kd-tree's answer is a k-nearest set by d2."""
    c = [c for c in KNN_CASES if c.family == "placed" and c.k == 300][0]
    pts, qs, b = S.case_input(c)
    seen = 0
    for t in np.nonzero(b.qfin)[0][::29]:
        oi, od = O.brute_knn(pts, qs[t], 300)
        one = b.rows(slice(t, t + 1))
        S.check_knn(pts, qs[t:t + 1], 300, oi[None], od[None], [300], brute=one, ranked_by="dist")
        S.check_knn(pts, qs[t:t + 1], 300, *O.knn_batch(pts, qs[t:t + 1], 300), brute=one)
        try:
            S.check_knn(pts, qs[t:t + 1], 300, oi[None], od[None], [300], brute=one)
        except AssertionError as e:
            assert "not the 300 nearest" in str(e)
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("name,cloud,radius,nq", RADIUS_ALL_CASES, ids=[r[0] for r in RADIUS_ALL_CASES])
def test_kdtree_unbounded_radius_answer_passes_the_checker(name, cloud, radius, nq):
    pts, qs, b = S.case_input(S.Case(name, cloud, 0, radius, nq))
    tree = O.KdTree(pts)
    seg = [tree.find_radius_neighbors(q, radius) for q in qs]
    off = np.concatenate([[0], np.cumsum([len(i) for i, _ in seg])])
    total = S.check_radius_all(pts, qs, radius, off, np.concatenate([i for i, _ in seg]), np.concatenate([d for _, d in seg]), brute=b)
    assert total == off[-1]


# ---- (b) what each family is there for ------------------------------------------------------------------------------------------
def tie_share(c):
    pts, qs, b = S.case_input(c)
    rep = S.check_knn(pts, qs, c.k, *oracle_answer(c), c.radius, brute=b)
    return 1.0 - rep.no_tie / rep.queries


def test_uniform_cloud_has_no_tie_at_any_cut():
    """every query's set is unique at every list size: the checker's set comparison binds everywhere"""
    for c in KNN_CASES:
        if c.family in ("lists", "nq"):
            assert tie_share(c) == 0.0, S.case_id(c)


def test_lattices_cut_a_plateau():
    """Every k of LIST_KS below the cloud's size cuts a plateau for at least 80 % of the queries (the shells of queries near the
    boundary are cut off by it: k = 18 on both lattices, 33 and 256 on the plain one lie between 80 and 90 %, every other k above
    90 %) -- except k = 1 on the plain lattice, where a query ON a lattice point has itself as its one nearest (the 1331 cell
    centres tie eight ways: 43 %).  With every point stored three times k = 1 ties as well."""
    for c in KNN_CASES:
        if c.family in ("lattice", "lattice3") and c.k < len(S.case_input(c)[0]):
            share = tie_share(c)
            if (c.family, c.k) == ("lattice", 1):
                assert 0.40 < share < 0.50
            else:
                assert share >= (0.80 if (c.family, c.k) in (("lattice", 18), ("lattice3", 18), ("lattice", 33), ("lattice", 256)) else 0.90), (S.case_id(c), share)
    assert len(S.lattice(3)[0]) == 3 * 1728 and np.array_equal(S.lattice(3)[0][:1728], S.lattice(3)[0][1728:3456])
    assert np.array_equal(S.lattice()[0] * 8, np.round(S.lattice()[0] * 8))                  # multiples of 1/8: exact in f32


def test_duplicate_plateaus_are_larger_than_any_quota():
    pts, qs, b = S.case_input(KNN_CASES[[c.family for c in KNN_CASES].index("duplicates")])
    sites = b.rows(slice(0, 200))
    assert ((sites.sd2[:, :40] == 0).all() and (sites.sd2[:, 40] > 0).all())                  # 40 copies at distance 0
    for c in KNN_CASES:
        if c.family == "duplicates":
            plateau = (sites.sd2 == sites.sd2[:, c.k - 1:c.k]).sum(axis=1)
            assert (plateau >= 40).all() and (plateau > c.k % 40).all()
            assert tie_share(c) >= (0.90 if c.k % 40 else 0.0)


def test_small_clouds_lie_on_both_sides_of_k():
    for k in S.SMALL_KS:
        ns = [len(S.small(n)[0]) for n in S.small_sizes(k)]
        assert ns == [1, 2, k - 1, k, k + 1]
    for c in KNN_CASES:
        if c.family == "small":
            assert (oracle_answer(c)[2] == min(c.k, c.cloud[1][0])).all()


def test_degenerate_clouds_are_degenerate():
    ext = {kind: np.ptp(S.degenerate(kind)[0], axis=0) for kind in S.DEGENERATE_KINDS}
    assert (ext["identical"] == 0).all() and len(S.degenerate("identical")[0]) == 500
    assert ext["line_x"][0] > 0 and (ext["line_x"][1:] == 0).all() and (ext["line_diag"] > 0).all()
    d = S.degenerate("line_diag")[0]
    assert np.array_equal(d[:, 0], d[:, 1]) and np.array_equal(d[:, 0], d[:, 2]) and len(d) == 2000
    assert ext["plane"][2] == 0 and (ext["plane"][:2] > 0).all() and len(S.degenerate("plane")[0]) == 4000
    ball = S.degenerate("ball_far")[0]
    clamped, lo, hi = S.grid_box(ball)
    assert not clamped and np.array_equal(lo, ball.min(axis=0)) and np.array_equal(hi, ball.max(axis=0))     # the box stays exact
    assert np.ptp(ball[:3000], axis=0).max() <= 1.0 and ext["ball_far"].min() > 80.0
    # a query among the scattered points has most of its neighbours in the ball, tens of cells away
    far_rows = S.case_input(S.Case("degenerate", ("degenerate", ("ball_far",)), 9, None, None))[2].rows(slice(60, 90))
    assert (np.sqrt(far_rows.sd2[:, 8]) > 5.0).mean() > 0.5


def test_placed_queries_reach_every_place():
    pts, qs = S.placed_queries()
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    diag = np.linalg.norm(hi - lo)
    fin = np.all(np.isfinite(qs), axis=1)
    assert (~fin).sum() >= 20 and np.isnan(qs).any() and (qs == np.inf).any() and (qs == -np.inf).any()
    for a in range(0, len(qs) - 63, 64):                              # every wave of 64 queries holds finite and non-finite ones
        assert fin[a:a + 64].any() and (~fin[a:a + 64]).any()
    q = qs[fin]
    out = np.linalg.norm(np.maximum(np.maximum(lo - q, q - hi), 0), axis=1)
    on_face = (((q == lo) | (q == hi)).sum(axis=1) >= 1) & (out == 0)
    assert ((out == 0) & ~on_face).sum() >= 60 and on_face.sum() >= 40 and (((q == lo) | (q == hi)).all(axis=1)).sum() == 8
    for mult in (1.0, 1.0e3, 1.0e6):
        assert ((out > 0.9 * mult * diag) & (out < 1.6 * mult * diag)).sum() >= 13


def test_many_queries_differ_between_a_blocks_trips():
    pts, qs = S.many_queries()
    assert len(pts) == 300 and len(qs) == 70000 and S.NQ_LARGE == (65535, 65536, 65537, 70000) and S.NQ_LARGE_K > 129
    j = np.arange(70000 - 65536)
    assert (qs[j] != qs[j + 65536]).any(axis=1).all()
    cnt = oracle_answer(MANY_CASES[-1])[2].astype(np.int64)
    assert MANY_CASES[-1].radius == S.NQ_LARGE_RADIUS and MANY_CASES[-1].nq == 70000
    assert (cnt[j] != cnt[j + 65536]).mean() >= 0.90 and cnt.min() == 0 and cnt.max() == S.NQ_LARGE_K
    near = oracle_answer(MANY_CASES[3])[0]
    assert (near[j, 0] != near[j + 65536, 0]).mean() >= 0.90


def test_far_outlier_cloud_clamps_by_the_builders_rule():
    """grid_box restates the rule (four hashed sample boxes against the exact box); the input is
    test_far_outliers_clamped_grid_stays_exact's at 6000 points, which that test knows to clamp.  Nothing visible from Python
    says whether a built grid came out clamped, so this is the rule, not the library."""
    pts, qs = S.far_outliers()
    clamped, lo, hi = S.grid_box(pts)
    assert clamped and len(pts) == 6000
    assert (lo > pts.min(axis=0)).all() and (hi[[0, 2]] < pts.max(axis=0)[[0, 2]]).all()     # outliers beyond five of the box's six faces
    outside = ((pts < lo) | (pts > hi)).any(axis=1)
    assert 4 <= outside.sum() <= 5                                                # (two of the five draws may share a slot)
    q_out = ((qs < lo) | (qs > hi)).any(axis=1)
    assert q_out.sum() >= 8 and (~q_out).sum() >= 150
    assert not S.grid_box(S.uniform()[0])[0] and not S.grid_box(pts[:4095])[0]    # too few points: never clamped


def test_shifted_clouds_keep_every_difference():
    for kind in ("uniform", "lattice"):
        p0, q0 = S.shifted(kind, 0.0)
        b0 = S.Brute(p0, q0)
        for s in S.FAR_SHIFTS:
            p, q = S.shifted(kind, s)
            assert np.array_equal(p - np.float32(s), p0) and np.array_equal(q - np.float32(s), q0)
            assert p.min() >= s - 2 and np.array_equal(S.Brute(p, q).d2.view(np.uint32), b0.d2.view(np.uint32))
    assert np.array_equal(S.shifted("lattice", 0.0)[0], S.lattice()[0])


def test_shell_radii_sit_on_the_shells():
    """0.25 and 0.5 square exactly onto a shell; f32(0.25 sqrt 2) squares to 0.12499999, so the 12-point shell at 0.125 lies
    OUTSIDE it and inside one ulp more.  An interior lattice point has SHELL_COUNTS points within each radius."""
    pts, qs, b = S.case_input(S.Case("shell_radius", ("lattice", (1,)), 1, None, None))
    interior = np.nonzero(((qs[:1728] >= 0.5) & (qs[:1728] <= 2.25)).all(axis=1))[0]
    assert len(interior) == 8 ** 3
    for base, shell_d2, counts in zip(S.SHELL_RADII, (0.0625, 0.125, 0.25), S.SHELL_COUNTS):
        below, at, above = (S.radius_sq(r) for r in S.ulps(base))
        if base == S.SHELL_RADII[1]:
            assert below < at < shell_d2 <= above and at == np.nextafter(np.float32(0.125), np.float32(0))
        else:
            assert below < shell_d2 == at < above
        for r2, cnt in zip((below, at, above), counts):
            assert ((b.d2[interior] <= r2).sum(axis=1) == cnt).all()
        assert (b.d2[interior] == np.float32(shell_d2)).any()


def test_unbounded_radius_inputs():
    counts = {}
    for name, cloud, radius, nq in RADIUS_ALL_CASES:
        b = S.case_input(S.Case(name, cloud, 0, radius, nq))[2]
        r2 = S.radius_sq(radius)
        counts[name] = (b.d2 <= r2).sum(axis=1) if r2 is not None else np.zeros(len(b.d2), np.int64)
    gap = counts["every_second_empty-r0.1"]
    assert (gap[1::2] == 0).all() and (gap[0::2] > 0).mean() > 0.9 and len(gap) == 128
    assert (counts["whole_cloud-r10.0-nq129"] == 3000).all()                     # far beyond the k-NN kernels' lists (> 600)
    assert counts["clamped_wide-r2.5-nq64"].max() > 600
    assert [len(counts[f"nq-r0.12-nq{n}"]) for n in (127, 128, 129)] == [127, 128, 129]
    assert counts["no_radius-r0.0-nq129"].sum() == 0 and counts["no_radius-rnan-nq129"].sum() == 0


# ---- (c) mutants of a correct answer ----------------------------------------------------------------------------------------------
def _mutant(kind, c, b, idx, dist, cnt):
    """the answer with one thing wrong, or None where this case has no place for it"""
    idx, dist, cnt = idx.astype(np.int64).copy(), dist.copy(), cnt.astype(np.int64).copy()
    r2 = S.radius_sq(c.radius) if c.radius is not None else None
    rows = np.arange(len(cnt))
    if kind == "tie_partner_twice":                       # an index replaced by the neighbour that ties with it
        for t in rows[cnt >= 2]:
            j = np.nonzero(dist[t, 1:cnt[t]] == dist[t, :cnt[t] - 1])[0]
            if len(j):
                idx[t, j[0]] = idx[t, j[0] + 1]
                return idx, dist, cnt
    if kind == "next_farther":                            # the last index replaced by the nearest point beyond the answer
        for t in rows[cnt >= 1]:
            beyond = b.d2[t] > b.sd2[t, cnt[t] - 1]
            if beyond.any() and np.isfinite(b.d2[t][beyond]).any():
                idx[t, cnt[t] - 1] = np.argmin(np.where(beyond, b.d2[t], np.inf))
                return idx, dist, cnt
    if kind == "distances_swapped":
        for t in rows[cnt >= 2]:
            if dist[t, 0] != dist[t, cnt[t] - 1]:
                dist[t, [0, cnt[t] - 1]] = dist[t, [cnt[t] - 1, 0]]
                return idx, dist, cnt
    if kind in ("count_minus_one", "count_plus_one") and r2 is not None:      # at a radius that IS a neighbour's distance
        on = (b.sd2[:, :c.k] == r2).any(axis=1) & (cnt >= 1) & (cnt < c.k)
        if on.any():
            cnt[np.nonzero(on)[0][0]] += 1 if kind == "count_plus_one" else -1
            return idx, dist, cnt
    if kind == "strict_radius" and r2 is not None:        # d2 < r^2 for d2 <= r^2
        strict = np.where(b.qfin, (b.sd2[:, :min(c.k, b.nfin)] < r2).sum(axis=1), 0)
        if (strict != cnt).any():
            return idx, dist, strict
    return None


MUTANTS = ("tie_partner_twice", "next_farther", "distances_swapped", "count_minus_one", "count_plus_one", "strict_radius")


def mutant_table():
    """{mutant: {family: (cases where it applies, cases where the checker fails it)}}"""
    table = {m: {} for m in MUTANTS}
    for c in KNN_CASES:
        pts, qs, b = S.case_input(c)
        good = oracle_answer(c)
        for m in MUTANTS:
            bad = _mutant(m, c, b, *good)
            if bad is None:
                continue
            try:
                S.check_knn(pts, qs, c.k, *bad, c.radius, brute=b)
                caught = 0
            except AssertionError:
                caught = 1
            a, f = table[m].get(c.family, (0, 0))
            table[m][c.family] = (a + 1, f + caught)
    return table


def test_every_mutant_fails_the_checker_wherever_it_applies():
    table = mutant_table()
    for m in MUTANTS:
        assert table[m], m                                                      # it applies somewhere ...
        for family, (applies, fails) in table[m].items():
            assert fails == applies, (m, family, applies, fails)                # ... and never survives
    assert {"lattice", "lattice3", "duplicates"} <= set(table["tie_partner_twice"])
    assert set(table["next_farther"]) >= set(FAMILIES) - {"no_radius"}
    assert "shell_radius" in table["count_minus_one"] and "shell_radius" in table["strict_radius"]


def test_unbounded_radius_mutants_fail_the_checker():
    pts, qs, b = S.case_input(S.Case("shell", ("lattice", (1,)), 0, 0.25, None))
    tree = O.KdTree(pts)
    seg = [tree.find_radius_neighbors(q, 0.25) for q in qs[:200]]
    off = np.concatenate([[0], np.cumsum([len(i) for i, _ in seg])])
    idx, dist = np.concatenate([i for i, _ in seg]).astype(np.int64), np.concatenate([d for _, d in seg])
    b = b.head(200)
    S.check_radius_all(pts, qs[:200], 0.25, off, idx, dist, brute=b)
    strict = [(i[d < 0.25], d[d < 0.25]) for i, d in seg]                       # '<' for '<=' loses the shell at exactly 0.25
    with pytest.raises(AssertionError, match="count"):
        S.check_radius_all(pts, qs[:200], 0.25, np.concatenate([[0], np.cumsum([len(i) for i, _ in strict])]),
                           np.concatenate([i for i, _ in strict]), np.concatenate([d for _, d in strict]), brute=b)
    swapped = dist.copy()
    swapped[[0, off[1] - 1]] = swapped[[off[1] - 1, 0]]
    with pytest.raises(AssertionError, match="order"):
        S.check_radius_all(pts, qs[:200], 0.25, off, idx, swapped, brute=b)
    other = idx.copy()
    other[1] = int(np.argmax(b.d2[0]))
    with pytest.raises(AssertionError, match="set"):
        S.check_radius_all(pts, qs[:200], 0.25, off, other, dist, brute=b)


if __name__ == "__main__":                                                      # the table of STATE.md
    for m, row in mutant_table().items():
        print(m, {f: f"{fails}/{applies}" for f, (applies, fails) in sorted(row.items())})
