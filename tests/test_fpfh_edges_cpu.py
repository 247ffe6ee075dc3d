"""The cases of tests/fpfh_cases.py prove themselves on the checker alone (tests/fpfh_checker.py), without a GPU: (a) the road every
compared row takes and the facts each family is there for; (b) the condition that keeps the checker's loose bound from hiding
anything: every compared row strict in shells, far_pairs, unbounded, k_edges and shifted, at least 98 % in duplicates, blocks and
chunked, and no compared row anywhere bounded above 0.1; (c) mutants: the checker with one rule changed fails F.compare against the
real checker in the family named for it.  `python tests/test_fpfh_edges_cpu.py` prints the mutant table of STATE.md.

k_max (k = 2047 on 2 100 points, three rows) cannot be strict: a row's 2047 neighbours bring 4.2 million pairs, of which the theta
edge band (2e-6 of a bin, ten edges) flags about fifteen.  Its rows are held to the 0.1 cap (their bound is 0.001)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import fpfh_cases as C  # noqa: E402
from tests import fpfh_checker as F  # noqa: E402
from tests import search_checker as S  # noqa: E402

CASES, CHUNKED = C.cases(), C.chunked_cases()
ALL_STRICT = ("shells", "far_pairs", "unbounded", "k_edges", "shifted")
MOSTLY_STRICT = ("duplicates", "blocks", "chunked")


def _case(family, name=None, radius=None, k=None):
    hits = [c for c in CASES + CHUNKED if c.family == family and (name is None or c.name == name) and (k is None or c.k == k) and
            (radius is None or c.radius == radius or (np.isnan(radius) and np.isnan(c.radius)))]
    assert len(hits) == 1, (family, name, radius, k, len(hits))
    return hits[0]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- (b) the loose bound hides nothing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES + CHUNKED, ids=C.case_id)
def test_compared_rows_are_strict_and_bounded(c):
    ref = C.reference(c)
    assert len(ref["strict"]) > 0
    if c.family in ALL_STRICT:
        assert ref["strict"].all(), float(ref["strict"].mean())
    elif c.family in MOSTLY_STRICT:
        assert ref["strict"].mean() >= 0.98, float(ref["strict"].mean())
    else:
        assert c.family == "k_max" and not ref["strict"].any()          # (the module's docstring)
    assert ref["bound"].max() <= 0.1, float(ref["bound"].max())
    assert np.isfinite(ref["desc"]).all() and (ref["desc"] >= 0).all()


def test_the_table_holds_every_family():
    fam = {c.family for c in CASES + CHUNKED}
    assert fam == set(ALL_STRICT) | set(MOSTLY_STRICT) | {"k_max"}
    ids = [C.case_id(c) for c in CASES + CHUNKED + C.all_zero_cases()]
    assert len(set(ids)) == len(ids)
    # every call but the chunked ones is small
    for c in CASES:
        assert len(C.case_input(c)[0]) <= (2100 if c.k == C.K_MAX else 6100)


# ---- (a) shells -------------------------------------------------------------------------------------------------------------------
def test_shell_table_is_the_tie_free_part_of_the_candidates():
    """counts from the checker (k = 0: the list is the ball), and SHELL_KEPT = the candidates without a tie on any interior row; on the
    others EVERY row ties (k cuts a plateau)"""
    pos, nrm = C.lattice()
    rows = C.lattice_interior()
    assert len(rows) == 512
    for base, counts in zip(C.SHELL_BASES, C.shell_counts()):
        for r, cnt in zip(S.ulps(base), counts):
            assert (F.fpfh(pos, nrm, r, 0, rows)["nlist"] == cnt).all(), (r, cnt)
    assert C.shell_counts() == ((0, 6, 6), (6, 6, 18))
    kept = set()
    for b, w, r, k in C.shell_candidates():
        ref = F.fpfh(pos, nrm, r, k, rows)
        if not ref["tie"].any():
            kept.add((b, w, k))
        else:
            assert ref["tie"].all(), (b, w, k)
    assert kept == {(b, w, k) for (b, w), ks in C.SHELL_KEPT.items() for k in ks}
    assert {(0, 1, 7), (1, 2, 19), (0, 0, 1)} <= {(b, w, k) for b, w, _, k in C.shell_candidates()} - kept


def test_shell_roads_and_the_rows_that_must_differ():
    below, at, above = S.ulps(0.25)
    for c in CASES:
        if c.family == "shells":
            b, w = int(c.name[1]), "-=+".index(c.name[2])
            cnt = C.shell_counts()[b][w]
            nl = C.reference(c)["nlist"]
            assert (nl == (cnt if cnt >= c.k else c.k)).all()            # the radius road keeps the ball, the fallback k
    ref = {(r, k): C.reference(_case("shells", radius=r, k=k))["desc"] for r, k in ((at, 6), (below, 6), (above, 6), (at, 1), (at, 5))}
    # the ball (cnt == k: no fallback) and the fallback (the ball is empty) find the same six points: the same bits
    assert np.array_equal(_bits(ref[(at, 6)]), _bits(ref[(below, 6)])) and np.array_equal(_bits(ref[(at, 6)]), _bits(ref[(above, 6)]))
    assert np.array_equal(_bits(ref[(at, 1)]), _bits(ref[(at, 5)]))      # cnt >= k: k does not matter
    pos, nrm = C.lattice()
    rows = C.lattice_interior()
    seven = F.fpfh(pos, nrm, at, 7, rows)["desc"]                         # cnt = 6 < 7: a seventh point
    assert (np.abs(seven - ref[(at, 6)]).max(axis=1) > 1e-3).all()
    one_below = F.fpfh(pos, nrm, below, 1, rows)["desc"]                  # the ball is empty: one point instead of six
    assert (np.abs(one_below - ref[(at, 1)]).max(axis=1) > 1e-3).all()
    # the second shell: f32(0.25 sqrt 2) squares below 0.125, the next float holds the twelve
    r_at, r_above = S.ulps(C.SHELL_BASES[1])[1:]
    six, eighteen = C.reference(_case("shells", radius=r_at, k=6)), C.reference(_case("shells", radius=r_above, k=6))
    assert (six["nlist"] == 6).all() and (eighteen["nlist"] == 18).all()
    found = C.reference(_case("shells", radius=r_at, k=18))              # the fallback finds the shell the ball lost
    assert np.array_equal(_bits(found["desc"]), _bits(C.reference(_case("shells", radius=r_above, k=18))["desc"]))


# ---- far_pairs / clamped ------------------------------------------------------------------------------------------------------------
def test_far_pairs_clamp_the_grid_and_the_outliers_find_each_other():
    pos, nrm = C.far_pairs(True)
    clamped, lo, hi = S.grid_box(pos)
    assert clamped and len(pos) == C.FAR_N + C.FAR_OUT
    assert (lo >= -0.1).all() and (hi <= 1.1).all()                     # all six faces: the grid spans the cloud proper
    out = np.arange(C.FAR_N, len(pos))
    assert ((pos[out] < lo) | (pos[out] > hi)).any(axis=1).all()
    inside, _ = C.far_pairs(False)
    assert not S.grid_box(inside)[0] and np.array_equal(inside, pos[:C.FAR_N])
    o = lambda i: C.FAR_N + i                                              # noqa: E731
    d = lambda i, j: float(np.sqrt(F.d2_f32(pos[o(i)], pos[o(j)])))        # noqa: E731
    assert abs(d(*C.FAR_PAIR) - 0.03) < 1e-4 and abs(d(*C.FAR_HALF) - 0.5 * C.FAR_R) < 1e-4 and abs(d(*C.FAR_DISTANT) - 0.5 * C.FAR_R) < 1e-4
    assert max(d(4, 5), d(4, 6), d(5, 6)) < C.FAR_R
    diag = float(np.linalg.norm(hi - lo))
    assert pos[o(7), 0] > 0.9e6 * diag and pos[o(8), 0] == pos[o(7), 0]
    for k in C.FAR_KS:
        c = _case("far_pairs", "clamped", k=k)
        ref, rows = C.reference(c), C.case_input(c)[2]
        rows = np.arange(len(pos)) if rows is None else rows
        nl = dict(zip(rows.tolist(), ref["nlist"].tolist()))
        nb = F.Neighbours(pos, C.FAR_R, k, out)
        partner = {o(a): o(b) for a, b in (C.FAR_PAIR, C.FAR_PAIR[::-1], C.FAR_HALF, C.FAR_HALF[::-1], C.FAR_DISTANT, C.FAR_DISTANT[::-1])}
        for s, i in enumerate(out):
            if k == 1 and i in partner:
                assert nb.lists[s].tolist() == [partner[i]]              # one other point in the ball, k = 1: served by the ball walk
            if i in (o(4), o(5), o(6)):
                assert set(nb.lists[s][:2].tolist()) == {o(4), o(5), o(6)} - {i} and (k > 2 or len(nb.lists[s]) == 2)
        inball = {**{i: 1 for i in partner}, **{o(t): 2 for t in C.FAR_TRIPLE}}
        assert all(nl[i] == max(k, inball.get(i, 0)) for i in out if i in nl)      # the ball where it holds k, else the k nearest
        assert (ref["nlist"] > k).sum() > 4000 and (ref["nlist"] == k).sum() >= (1000 if k == 8 else 4)
        same = C.reference(_case("far_pairs", "exact", k=k))
        assert (same["nlist"] >= k).all()
    # the distant pair is compared where the ball walk serves it, and only there
    assert C.case_input(_case("far_pairs", "clamped", k=1))[2] is None
    assert not set(C.case_input(_case("far_pairs", "clamped", k=8))[2]) & {o(7), o(8)}


# ---- unbounded ----------------------------------------------------------------------------------------------------------------------
def test_unbounded_radii_and_roads():
    with np.errstate(over="ignore"):
        r2 = [np.float32(r) * np.float32(r) for r in C.UNBOUNDED_RADII]
    assert np.isinf(r2[0]) and np.isfinite(r2[1]) and r2[1] > np.float32(3.0e38) and r2[2] == np.float32(1e6)
    for c in CASES:
        if c.family == "unbounded":
            n = c.cloud[1][0]
            ref = C.reference(c)
            assert (ref["nlist"] == n - 1).all() and c.k in (5, n + 3)   # the whole cloud, by the ball (k = 5) or by the fallback
    a, b = C.reference(_case("unbounded", "n300", 1e20, 5)), C.reference(_case("unbounded", "n300", 1e20, 303))
    assert np.array_equal(_bits(a["desc"]), _bits(b["desc"]))


# ---- duplicates ---------------------------------------------------------------------------------------------------------------------
def test_duplicate_clouds():
    pos, _ = C.copies(200, 12, C.DUP_SEED)
    _, inv, cnt = np.unique(pos, axis=0, return_inverse=True, return_counts=True)
    assert len(cnt) == 200 and (cnt == 12).all()
    k8, k11, k12 = (C.reference(_case("duplicates", "x12", C.DUP_R, k)) for k in (8, 11, 12))
    assert (k8["nlist"] >= 11).all()                                     # more than k = 8 duplicates in every ball: not among its own k + 1 nearest
    assert (k11["nlist"] == 11).sum() >= 100 and (k11["nlist"] > 11).sum() >= 1000      # cnt == k exactly: no fallback
    assert np.array_equal(_bits(k8["desc"]), _bits(k11["desc"]))
    full = F.fpfh(pos, C.copies(200, 12, C.DUP_SEED)[1], C.DUP_R, 12)
    assert (full["tie"] == (full["nlist"] == 12)).all() and 100 <= full["tie"].sum() == len(pos) - len(k12["nlist"])   # cnt == k - 1
    k23 = C.reference(_case("duplicates", "x12", C.NAN, 23))
    assert (k23["nlist"] == 23).all() and not k23["tie"].any()
    nb = F.Neighbours(pos, C.NAN, 23, np.arange(24))
    for i, l in enumerate(nb.lists):
        assert (F.d2_f32(pos[l[:11]], pos[i][None]) == 0).all() and len(np.unique(pos[l[11:]], axis=0)) == 1
    ident = C.reference(_case("duplicates", "identical"))
    assert (ident["desc"] == 0).all() and (ident["nlist"] == 499).all()
    for r in (0.02, 0.005):
        two = C.reference(_case("duplicates", "two_sites", r))
        assert (two["nlist"] == (599 if r == 0.02 else 299)).all()
        for site in (0, 1):
            rows = _bits(two["desc"][site::2])
            assert (rows == rows[0]).all()
        if r == 0.02:
            assert (two["desc"].max(axis=1) > 0).all()
        else:
            assert (two["desc"] == 0).all()                              # only its own copies in the ball
    for c in C.all_zero_cases():
        pos, nrm, _ = C.case_input(c)
        ref = F.fpfh(pos, nrm, c.radius, c.k)
        assert (ref["desc"] == 0).all() and (ref["nlist"] == c.k).all() and ref["tie"].all()
        nb = F.Neighbours(pos, c.radius, c.k)
        assert all((F.d2_f32(pos[l], pos[i][None]) == 0).all() for i, l in enumerate(nb.lists))


# ---- k_edges ------------------------------------------------------------------------------------------------------------------------
def test_k_edges_sit_on_both_sides_of_every_list_size():
    assert {k + 1 for k in C.K_EDGES} == {9, 10, 17, 18, 33, 34, 65, 66, 129, 130, 256, 257}
    for c in CASES:
        if c.family in ("k_edges", "k_max"):
            n = c.cloud[1][0]
            assert np.isnan(c.radius) and (C.reference(c)["nlist"] == min(c.k, n - 1)).all()
    assert _case("k_edges", "n150").k == 2047 > 150 and _case("k_max", "n2100").k == 2047 < 2100


# ---- blocks -------------------------------------------------------------------------------------------------------------------------
def test_blocks_mix_the_three_modes():
    assert C.BLOCK_NS == (127, 128, 129, 255, 256, 257, 513)
    for n in C.BLOCK_NS:
        c = _case("blocks", f"n{n}")
        pos, _, _ = C.case_input(c)
        ref = C.reference(c)
        bad = np.array([0, n // 2, n - 1])
        fin = np.isfinite(pos).all(axis=1)
        assert (~fin).sum() == 3 and not fin[bad].any() and np.isnan(pos[0]).any() and np.isinf(pos[n // 2]).any()
        assert (ref["nlist"][bad] == 0).all() and (ref["desc"][bad] == 0).all()
        dense, sparse = np.arange(1, n // 2), np.arange(n // 2 + 1, n - 1)
        assert (pos[dense] <= 0.1).all() and (ref["nlist"][dense] > c.k).all()          # the radius road
        assert (ref["nlist"][sparse] == c.k).mean() >= 0.95                              # the fallback


# ---- shifted ------------------------------------------------------------------------------------------------------------------------
def test_shifted_clouds_keep_every_difference():
    p0, n0 = C.shifted(0.0)
    base = C.reference(_case("shifted", "by0"))
    rows = C.case_input(_case("shifted", "by0"))[2]
    assert len(rows) >= 5000 and (base["nlist"] == 8).sum() >= 500 and (base["nlist"] > 8).sum() >= 3000
    assert np.array_equal(p0 * 128, np.round(p0 * 128))
    for s in C.SHIFTS[1:]:
        c = _case("shifted", f"by{int(s)}")
        p, _, r = C.case_input(c)
        assert np.array_equal(p - np.float32(s), p0) and p.min() >= s and np.array_equal(r, rows)
        assert np.array_equal(_bits(C.reference(c)["desc"]), _bits(base["desc"]))          # the checker's rows do not move


# ---- chunked ------------------------------------------------------------------------------------------------------------------------
def test_chunked_clouds_need_two_chunks_and_the_face_rows_read_the_second():
    """the checker's neighbour rule over all 1.9 M points: counts within the narrowed and the widened radius, the f32 relation where
    the two differ.  The device lists its fallback points in the order their blocks arrive, which follows the cell order (z-major)
    to within the blocks in flight (256 CUs x 4 blocks x 256 lanes = 2^18 points): a fallback point whose rank by z is beyond
    2^20 + 2^18 is in the second chunk."""
    from scipy.spatial import cKDTree
    c = _case("chunked", "mixed")
    pos, _, rows = C.case_input(c)
    assert C.CHUNK_LISTS == 1 << 20 and len(pos) == C.CHUNK_SPARSE + C.CHUNK_DENSE
    p64 = pos.astype(np.float64)
    tree = cKDTree(p64)
    r, r2 = float(np.float32(C.CHUNK_R)), np.float32(C.CHUNK_R) * np.float32(C.CHUNK_R)
    slack = 1e-5 * r + 8.0 * 2.0 ** -24 * (1.0 + r)
    wide = tree.query_ball_point(p64, r + slack, return_length=True, workers=8) - 1
    narrow = tree.query_ball_point(p64, r - slack, return_length=True, workers=8) - 1
    cnt = narrow.copy()
    for i in np.nonzero((narrow < c.k) & (wide >= c.k))[0]:
        cand = np.array(tree.query_ball_point(p64[i], r + slack))
        cand = cand[cand != i]
        cnt[i] = (F.d2_f32(pos[cand], pos[i][None]) <= r2).sum()
    fb = cnt < c.k
    nf = int(fb.sum())
    assert C.CHUNK_LISTS < nf <= 2 * C.CHUNK_LISTS and nf % 128 != 0 and nf == 1506860, nf
    assert fb[:C.CHUNK_SPARSE].mean() > 0.98 and fb[C.CHUNK_SPARSE:].mean() < 0.1
    ref = C.reference(c)
    went = fb[rows]                                                       # the road of every compared row
    assert (ref["nlist"][went] == c.k).all() and (ref["nlist"][~went] >= c.k).all()
    assert (ref["nlist"][~went] >= narrow[rows][~went]).all() and (ref["nlist"][~went] <= wide[rows][~went]).all()
    assert (ref["nlist"][:300] == c.k).sum() >= 290 and (ref["nlist"][300:600] > c.k).sum() >= 250
    rank = np.full(len(pos), -1, np.int64)
    order = np.argsort(pos[fb, 2], kind="stable")
    rank[np.nonzero(fb)[0][order]] = np.arange(nf)
    late = 0
    for s in np.nonzero(ref["nlist"][600:] > c.k)[0]:
        i = rows[600 + s]
        near = np.array(tree.query_ball_point(p64[i], r - slack))
        late += bool((rank[near] > C.CHUNK_LISTS + (1 << 18)).any())
    assert late >= 40, late
    # all_fallback: the last chunk holds one query
    c = _case("chunked", "all_fallback")
    assert len(C.case_input(c)[0]) == C.CHUNK_LISTS + 1 and np.isnan(c.radius) and (C.reference(c)["nlist"] == c.k).all()


# ---- (c) mutants ------------------------------------------------------------------------------------------------------------------
def _swap_lists(lists):
    """rows 600 .. 699 of `mixed` (the face rows) summed from the lists of rows 0 .. 99 (sparse rows: first-chunk queries)"""
    return lists[:600] + lists[:100]


MUTANTS = {
    # name: (rule changed, the cases it must fail in).  `d2 < r^2` at k = 6 on the 0.25 shell is no case: the emptied ball falls back
    # and the fallback finds the same six points (test_shell_roads_and_the_rows_that_must_differ)
    "d2 < r^2": (dict(within=lambda d2, r2: d2 < r2), [("shells", None, 0.25, 1), ("shells", None, 0.25, 5)]),
    "the fallback keeps the query": (dict(fallback_list=lambda cc, i, k: cc[:k]), [("k_edges", "n600", C.NAN, 8), ("k_edges", "n600", C.NAN, 256),
                                                                                 ("duplicates", "x12", C.NAN, 23)]),
    "the fallback keeps k + 1": (dict(fallback_list=lambda cc, i, k: cc[: k + 2][cc[: k + 2] != i]), [("k_edges", "n600", C.NAN, 8), ("k_edges", "n600", C.NAN, 129),
                                                                                                   ("duplicates", "x12", C.NAN, 23)]),
    "weight 1 / d^2": (dict(weight=lambda dist: np.float32(1) / (dist * dist)), [("k_edges", "n600", C.NAN, 16), ("far_pairs", "exact", C.FAR_R, 8),
                                                                                ("blocks", "n257", C.BLOCK_R, C.BLOCK_K)]),
    "a skipped pair counted in valid": (dict(count_skipped=True), [("duplicates", "x12", C.DUP_R, 8), ("duplicates", "x12", C.DUP_R, 12)]),
    "the sum divided by the list length": (dict(divide_by_length=True), [("k_edges", "n600", C.NAN, 16), ("unbounded", "n64", 1e3, 5),
                                                                         ("duplicates", "x12", C.DUP_R, 8)]),
    "the outlier pair not found": (dict(lists_hook=lambda lists: [l if i not in (C.FAR_N + C.FAR_HALF[0], C.FAR_N + C.FAR_HALF[1]) else l[:0]
                                                                   for i, l in enumerate(lists)]), [("far_pairs", "clamped", C.FAR_R, 1)]),
    "second-chunk rows summed from first-chunk lists": (dict(lists_hook=_swap_lists), [("chunked", "mixed", C.CHUNK_R, C.CHUNK_K)]),
    # one of this file's own: the farthest neighbour (the smallest weight of the row) replaced by the nearest, named twice
    "the last entry of a list replaced by its first": (dict(lists_hook=lambda lists: [l if len(l) < 2 else np.concatenate([l[:-1], l[:1]]) for l in lists]),
                                                      [("k_edges", "n600", C.NAN, 8), ("k_edges", "n600", C.NAN, 256), ("unbounded", "n300", 1e20, 5)]),
}
# Two rules have no mutant, because no descriptor can show them:
# * "cnt <= k falls back": with cnt == k the k nearest ARE the ball, in the same (d2, index) order (test_no_descriptor_shows_a_fallback_at_cnt_equal_k).
#   What shows it is the launch count: the GPU file's test_the_intended_code_ran finds no fallback search at duplicates-x12-k11, where 336
#   rows have cnt == k and no row has less.
# * "a query with more than k duplicates of itself loses a neighbour" has no mutant: whatever such a query's list holds or lacks is a
# copy of the query, and a copy is a skipped pair in the SPFH and in the sum.  No descriptor can show it; the all-zero cases pin what
# can be seen (test_duplicate_clouds, the GPU file's test_more_than_k_duplicates_everywhere_gives_zero_rows).


def test_no_descriptor_shows_a_fallback_at_cnt_equal_k():
    for family, name, radius, k in (("shells", None, 0.25, 6), ("shells", None, S.ulps(C.SHELL_BASES[1])[2], 18), ("duplicates", "x12", C.DUP_R, 11)):
        c = _case(family, name, radius, k)
        pos, nrm, rows = C.case_input(c)
        bad = F.fpfh(pos, nrm, c.radius, c.k, rows, rules=dict(falls_back=lambda cnt, k: cnt <= k))
        assert np.array_equal(_bits(bad["desc"]), _bits(C.reference(c)["desc"])) and (C.reference(c)["nlist"] == c.k).any()


def mutant_table():
    """{mutant: [(case id, failed, compared rows that moved by more than 1e-5, compared rows)]}"""
    table = {}
    for name, (rules, where) in MUTANTS.items():
        table[name] = []
        for family, cname, radius, k in where:
            c = _case(family, cname, radius, k)
            pos, nrm, rows = C.case_input(c)
            real = C.reference(c)
            bad = F.fpfh(pos, nrm, c.radius, c.k, rows, rules=rules)["desc"]
            moved = int((np.abs(bad - real["desc"]).max(axis=1) > 1e-5).sum())
            try:
                F.compare(bad, real)
                failed = False
            except AssertionError:
                failed = True
            table[name].append((C.case_id(c), failed, moved, len(bad)))
    return table


def test_every_mutant_fails_in_its_family():
    table = mutant_table()
    assert set(table) == set(MUTANTS)
    for name, rows in table.items():
        assert rows and all(failed for _, failed, _, _ in rows), (name, rows)
    # and the real checker passes itself
    for c in (_case("shells", radius=0.25, k=6), _case("duplicates", "x12", C.DUP_R, 12), _case("chunked", "mixed")):
        assert F.compare(C.reference(c)["desc"], C.reference(c)) >= 0.98


if __name__ == "__main__":                                                      # the table of STATE.md
    for name, rows in mutant_table().items():
        print(f"{name}: " + ", ".join(f"{cid} {'fails' if failed else 'SURVIVES'} ({moved} of {n} rows move)" for cid, failed, moved, n in rows))
