"""The cases of tests/shot_cases.py proven on the checker alone (tests/shot_checker.py): every case reaches what it is meant to reach, at
least 98 % of its compared rows are clean (margin >= 1e-6, so the margin hides nothing), and every mutant of the rule is told apart by a
case the GPU file runs, or is listed as invisible with the reason.  `python tests/test_shot_cpu.py` prints the mutant table and the share of
rows that the reference's f32 arithmetic moves by more than 1e-5 (STATE.md).

Why 1e-6 is sound: f64 sums taken in another order differ by ~1e-15 relative; the eigenvector's angle moves by that over the relative
eigen-gap, so by at most ~1e-9 on a clean row, and a dot product with dv / r by as much.  That is three orders inside the margin: on a clean
row no vote, no bin and no branch of the frame can differ between the device and the checker."""
import numpy as np
import pytest

from tests import fpfh_checker as FC
from tests import shot_cases as CASES
from tests import shot_checker as SC

DEGENERATE = ("degenerate_identical", "degenerate_line", "degenerate_plane")     # margin 0 by construction: only the not-clean guarantees apply


def test_the_constants_are_the_kernels():
    assert (CASES.K_WAVE, CASES.K_STAGE, CASES.K_KNN_ENTRIES) == (64, 512, 1 << 25)
    assert SC.DESC_TOL == 2.0 ** -23 and SC.FRAME_TOL == 1e-6 and SC.CLEAN == 1e-6 and CASES.MIN_CLEAN == 0.98


@pytest.mark.parametrize("variant", CASES.VARIANTS)
@pytest.mark.parametrize("name", [n for n in CASES.CASES if n not in DEGENERATE])
def test_at_least_98_percent_of_the_compared_rows_are_clean(name, variant):
    e = CASES.expected(name, variant)
    share = float(e["clean"].mean())
    print(f"{name} {variant}: {len(e['rows'])} rows, clean {share:.4f}, x-vote ties {float(((e['flags'] & SC.X_TIE) != 0).mean()):.3f}")
    assert share >= CASES.MIN_CLEAN and not SC.invariants(e["desc"])


@pytest.mark.parametrize("name", DEGENERATE)
def test_the_degenerate_cases_are_degenerate(name):
    e = CASES.expected(name, "shot")
    assert not e["clean"].any() and not SC.invariants(e["desc"])
    if name == "degenerate_identical":
        assert not e["desc"].any() and ((e["flags"] & SC.ZERO_COV) != 0).all() and (e["length"] == 499).all()


def test_the_three_clouds_reach_both_roads_and_the_ties():
    road = lambda e: np.bincount(e["flags"] & 3, minlength=3)
    a, b, c = (CASES.expected(n, "shot") for n in ("bumpy", "bumpy_mixed", "volume"))
    assert road(a)[1] <= 10 and road(c)[1] == 0 and min(road(b)[:2]) >= 500     # (a few corner points of the surface fall back at r = 0.12)
    for e in (a, b, c):
        assert ((e["flags"] & SC.X_TIE) != 0).mean() >= 0.02    # tie rows are compared like any other


def test_list_lengths_sit_on_every_threshold():
    c, e = CASES.case("list_lengths"), CASES.expected("list_lengths", "shot")
    W, S = CASES.K_WAVE, CASES.K_STAGE
    assert c["lengths"] == [W - 1, W, W + 1, 2 * W + 1, S - 1, S, S + 1]
    assert sorted(set(e["length"].tolist())) == sorted(c["lengths"]) and (e["flags"] & 3 == SC.ROAD_BALL).all()
    assert np.array_equal(np.bincount(e["length"])[c["lengths"]], np.array(c["lengths"]) + 1)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_blocks_hold_both_roads_and_the_bad_rows(n):
    c, e = CASES.case(f"blocks_{n}"), CASES.expected(f"blocks_{n}", "shot")
    assert len(c["np6"]) == n
    fl = e["flags"]
    if n == 1:
        assert fl.tolist() == [SC.ROAD_FALLBACK | SC.EMPTY] and not e["desc"].any() and not e["lrf"].any()
        return
    if n == 2:
        assert (e["length"] == 1).all() and (fl & 3 == SC.ROAD_FALLBACK).all()
        return
    assert (fl[[0, n // 2, n - 1]] == SC.ROAD_INERT).all() and (fl & 3 == SC.ROAD_INERT).sum() == 3
    assert not e["desc"][[0, n // 2, n - 1]].any() and not e["lrf"][[0, n // 2, n - 1]].any()
    assert (fl & 3 == SC.ROAD_BALL).sum() >= n // 2 - 2 and (fl & 3 == SC.ROAD_FALLBACK).sum() >= n // 8
    np6 = c["np6"]
    for q in (1, 2, n - 2, n - 3):                              # a zero and a NaN normal: z = (0, 0, 1) before the vote
        assert not np6[q, 3:].any() or np.isnan(np6[q, 3:]).all()
        assert abs(e["lrf"][q, 8]) == 1.0 and not e["lrf"][q, 6:8].any()
    nb = FC.Neighbours(np.ascontiguousarray(np6[:, :3]), np.float32(c["radius"]), c["k"])
    for q in (1, 2, n - 2, n - 3):                              # ... and they are somebody's neighbour
        assert any(q in lst for lst in nb.lists)


@pytest.mark.parametrize("k1", [34, 65, 66, 129, 130, 257])
def test_fallback_lists_vote_beyond_the_radius(k1):
    c, e = CASES.case(f"fallback_k{k1 - 1}"), CASES.expected(f"fallback_k{k1 - 1}", "shot")
    assert len(c["np6"]) == 600 and (e["flags"] & 3 == SC.ROAD_FALLBACK).all() and (e["length"] == k1 - 1).all()
    pos = np.ascontiguousarray(c["np6"][:, :3])
    r2 = np.float32(c["radius"]) ** 2
    ball = np.array([(FC.d2_f32(pos, pos[i][None, :]) <= r2).sum() - 1 for i in range(600)])
    assert ball.max() <= 0.8 * (k1 - 1), ball.max()             # a fifth of every list or more lies beyond the radius
    assert ball.mean() >= 4 and (e["counts"].sum(axis=1) == ball).all()           # they vote, and are in no bin


def test_fallback_counts():
    e = CASES.expected("fallback_k33", "usc")
    c = CASES.case("fallback_k33")
    pos = np.ascontiguousarray(c["np6"][:, :3])
    r2 = np.float32(c["radius"]) ** 2
    ball = np.array([(FC.d2_f32(pos, pos[i][None, :]) <= r2).sum() - 1 for i in range(600)])
    assert (e["counts"].sum(axis=1) == ball).all()              # what lies beyond the radius is in no bin


def test_exact_edges_sit_on_the_boundaries_themselves():
    c = CASES.case("exact_edges")
    np6, r = c["np6"], np.float32(c["radius"])
    assert r == 0.25 and np.array_equal(np6[:, :3] * 1024, np.round(np6[:, :3] * 1024))
    for t, q in enumerate(c["queries"]):
        partners = np6[c["n_base"] + 4 * t: c["n_base"] + 4 * t + 4, :3]
        dv = partners - np6[q, :3][None, :]
        dist = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        assert dist.dtype == np.float32 and dist.tolist() == [0.25, 0.125, 0.0625, 0.1875]
        assert FC.d2_f32(partners[:1], np6[q, :3][None, :])[0] == r * r       # d2 <= r^2 and not dist > r, on the boundary
        assert (dist / r * np.float32(4)).tolist() == [4.0, 2.0, 1.0, 3.0]     # USC's shell edges
    for v in CASES.VARIANTS:
        assert CASES.expected("exact_edges", v)["clean"].mean() >= CASES.MIN_CLEAN


def test_chunked_reaches_a_second_chunk_of_lists():
    c = CASES.case("chunked")
    n, k = len(c["np6"]), c["k"]
    assert k + 1 == CASES.K_MAX and n == 16400 and CASES.chunk_lists(k) == 16384 < n and len(c["rows"]) == 300
    e = CASES.expected("chunked", "shot")
    assert (e["flags"] & 3 == SC.ROAD_FALLBACK).all() and (e["length"] == k).all()


def test_the_shifted_clouds_are_exact():
    base = CASES.snapped()
    for s in CASES.SHIFTS:
        moved = CASES.shifted(s)
        assert np.array_equal((moved[:, :3].astype(np.float64) - s), base[:, :3].astype(np.float64))


# ---- the reference's f32 arithmetic against the contract's f64 ----
F32_CASES = ("bumpy", "bumpy_mixed", "volume")


def f32_share(name, variant="shot"):
    a, b = CASES.expected(name, variant), CASES.expected(name, variant, "f32")
    moved = np.abs(a["desc"].astype(np.float64) - b["desc"].astype(np.float64)).max(axis=1) > 1e-5
    return float(moved.mean()), float((moved & a["clean"]).mean())


@pytest.mark.parametrize("name", F32_CASES)
def test_f32_arithmetic_moves_few_rows(name):
    share, clean_share = f32_share(name)
    print(f"{name}: rows moved by more than 1e-5 in arith='f32': {share:.4%}, clean ones among them: {clean_share:.4%}")
    assert share <= 0.01                                        # the project's usual 1 % of rows


# ---- mutants ----
_keep_query = lambda cc, i, k: cc[:k]
_keep_k1 = lambda cc, i, k: cc[: k + 2][cc[: k + 2] != i][: k + 1]
MUTANTS = {
    "d2 < r^2": dict(within=lambda d2, r2: d2 < r2),
    "the fallback keeps the query": dict(fallback_list=_keep_query),
    "the fallback keeps k + 1": dict(fallback_list=_keep_k1),
    "z not voted": dict(vote_z=False),
    "x not voted": dict(vote_x=False),
    "weights 1 for r - dist": dict(weight=lambda r, dist: np.ones_like(dist)),
    "beyond-radius neighbours left out of the votes": dict(votes_beyond=False),
    "beyond-radius neighbours binned": dict(bins_beyond=True),
    "dist < r/2": dict(inner=lambda dist, half: dist < half),
    "lz <= 0 north": dict(south=lambda lz: lz <= 0),
    "azimuth without + pi": dict(azimuth_pi=False),
    "volume index transposed": dict(volume=lambda rb, eb, ab: ab * 4 + eb * 2 + rb),
    "per-volume division dropped": dict(per_volume=False),
    "L2 dropped": dict(l2=False),
    "USC's bin order transposed": dict(usc_bin=lambda ab, eb, rb: rb * 32 + eb * 8 + ab),
    "USC divided by the list length": dict(usc_by_length=True),
}
INVISIBLE = {
    "lz <= 0 north": "differs only where lz is exactly 0, and such a row has margin 0 (|z . dv| / r): it is never a compared clean row",
    "USC divided by the list length": "the L2 normalisation that follows divides the factor out again; the rows agree to a rounding",
}
MUTANT_CASES = ("exact_edges", "fallback_k33", "blocks_257", "bumpy_mixed")


def seen_by(rules):
    """the first (case, variant) of the GPU file's cases whose comparison tells the mutant from the rule"""
    for name in MUTANT_CASES:
        c = CASES.case(name)
        for v in CASES.VARIANTS:
            want = CASES.expected(name, v)
            got = SC.describe(c["np6"], c["radius"], c["k"], v, "f64", c["rows"], rules)
            if SC.compare(got["desc"], got["lrf"], got["flags"], want):
                return name, v
    return None


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_every_mutant_is_seen_or_listed(mutant):
    seen = seen_by(MUTANTS[mutant])
    print(mutant, "->", seen or "invisible: " + INVISIBLE.get(mutant, "?"))
    assert (seen is None) == (mutant in INVISIBLE)


def test_the_rule_itself_is_not_a_mutant():
    assert seen_by({}) is None


if __name__ == "__main__":                                      # the tables of STATE.md
    for m in MUTANTS:
        s = seen_by(MUTANTS[m])
        print(f"{m:50s} {'seen by ' + s[0] + ' / ' + s[1] if s else 'invisible: ' + INVISIBLE[m]}")
    for n in F32_CASES:
        print(n, "f32 against f64: share of rows moved by more than 1e-5, and of clean rows: %.4f %.4f" % f32_share(n))
    for n in CASES.CASES:
        for v in CASES.VARIANTS:
            e = CASES.expected(n, v)
            print(f"{n:22s} {v:4s} rows {len(e['rows']):5d} clean {e['clean'].mean():.4f} ties {((e['flags'] & SC.X_TIE) != 0).mean():.3f}")
