"""The cases of tests/filter_cases.py prove themselves on the checkers alone (tests/outlier_checker.py, tests/cluster_checker.py),
without a GPU: (a) what every family is there for -- the faces search_checker.grid_box() calls clamped, the far pairs and triples
and what each filter must make of them, the plateau an outlier 10^6 box diagonals out sees and that the checker's widening ends,
k + 1 above the finite count, the block counts of the statistics, component sizes, shell counts; (b) that the checkers, made
faster for these cases, still give the parent's answers on the existing inputs; (c) mutants: a checker with one rule changed differs
from the real one on a named case that tests/test_gpu_filter_edges.py runs.  `python tests/test_filter_edges_cpu.py` prints the
mutant table of STATE.md.

Nothing is left out of any comparison: means depend on the distance multiset, kept sets and partitions are unique."""
import math
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import cluster_checker as K  # noqa: E402
from tests import filter_cases as C  # noqa: E402
from tests import outlier_checker as OC  # noqa: E402
from tests import search_checker as SC  # noqa: E402

CASES = C.cases()
BY_ID = {C.case_id(c): c for c in CASES}
FAR, CONTROL = ("clamped_far", True), ("clamped_far", False)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_the_table():
    assert len(BY_ID) == len(CASES)
    assert {c.family for c in CASES} == {"clamped_far", "block_edges", "stats_edges", "shifted", "cluster_sizes", "lattice_shells"}
    for c in CASES:                                                  # every call but the statistics' is small
        assert len(C.case_input(c)) <= (6100 if c.family != "stats_edges" else 262144 + 257)
    assert [c.params[0] for c in CASES if c.family == "clamped_far" and c.op == "sor" and c.cloud == FAR] == list(C.FAR_KS)
    assert [k + 1 for k in C.FAR_KS] == [2, 3, 9, 17, 33, 65, 129, 130, 301]        # lists 9, 9, 9, 17, 33, 65, 129; buffers 512, 4096


# ---- (b) the checkers give the parent's answers -------------------------------------------------------------------------------------
def _parent_mean_distances(pos, k):
    """outlier_checker.mean_distances as the parent commit had it"""
    from scipy.spatial import cKDTree
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    fin = np.all(np.isfinite(pos), axis=1)
    pf = pos[fin]
    nfin = len(pf)
    K1 = min(int(k) + 1, nfin)
    d2 = np.zeros((nfin, K1), np.float32)
    if nfin:
        tree = cKDTree(pf.astype(np.float64))
        rows = np.arange(nfin)
        width = min(nfin, K1 + 16)
        while len(rows):
            d64, idx = tree.query(pf[rows].astype(np.float64), k=width)
            d64, idx = d64.reshape(len(rows), -1), idx.reshape(len(rows), -1)
            c = np.sort(OC.d2_f32(pf[rows][:, None, :], pf[idx]), axis=1)
            d2[rows] = c[:, :K1]
            if width >= nfin:
                break
            unsafe = (d64[:, -1] ** 2 <= c[:, K1 - 1].astype(np.float64) * (1.0 + 1e-5)) & (c[:, K1 - 1] > 0)
            rows = rows[unsafe]
            width = min(nfin, 2 * width)
    dist = np.sqrt(d2)
    use = d2 > 0
    s = np.zeros(len(d2), np.float32)
    for j in range(d2.shape[1]):
        s = s + np.where(use[:, j], dist[:, j], np.float32(0))
    cnt = use.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(cnt > 0, s / cnt.astype(np.float32), np.float32(0)).astype(np.float32)
    out = np.full(len(pos), np.nan, np.float32)
    out[fin] = m
    return out


def _existing_outlier_inputs():
    from tests import test_gpu_outliers as T          # (its clouds are plain numpy; nothing of it runs here)
    return T


def test_faster_checkers_give_the_parents_answers_on_the_existing_inputs():
    T = _existing_outlier_inputs()
    for name, k in [("uniform", 1), ("uniform", 17), ("uniform", 300), ("lattice", 6), ("lattice", 140), ("far", 8), ("far", 200), ("dup6", 4),
                    ("dup2", 4), ("five", 8), ("five", 200), ("one", 1), ("nonfinite", 8), ("nonfinite", 150)]:
        assert _same(OC.mean_distances(T.cloud(name), k), _parent_mean_distances(T.cloud(name), k)), (name, k)
    for n, k in OC.SOR_CASES[:2]:
        assert _same(OC.mean_distances(OC.sor_cloud(n), k), _parent_mean_distances(OC.sor_cloud(n), k)), (n, k)
    # the radius filter: every pair of a small cloud against the parent's kd-tree candidates (tree_road: the parent's code as it was)
    for name, radius in [("one", 1.0), ("far", 0.1), ("far", 1.5), ("nonfinite", 0.12), ("nonfinite", 1e19), ("nonfinite", 1.8e19), ("dup6", 1e-30),
                         ("dup2", 1e-30), ("uniform", 0.07), ("lattice", 0.25), ("lattice", 0.5), ("far", np.inf), ("far", np.nan)]:
        assert len(T.cloud(name)) <= OC.BRUTE_MAX
        assert np.array_equal(OC.radius_counts(T.cloud(name), radius), OC.radius_counts(T.cloud(name), radius, tree_road=True)), (name, radius)
    big = OC.sor_cloud(20000)
    assert np.array_equal(OC.radius_counts(big, 0.05), OC.radius_counts(big, 0.05, tree_road=True))         # above BRUTE_MAX: the same road
    pts = np.concatenate([K.sphere_cloud((0, 0, 0), 0.3, 200, 1), K.sphere_cloud((10, 0, 0), 0.3, 150, 2)])
    i, j = K.f32_pairs(pts, 0.5)
    for got, want in zip(K.clusters(pts, 0.5, 50, 10000), K.from_pairs(len(pts), i, j, 50, 10000)):
        assert np.array_equal(got, want)


# ---- (a) which inputs the builder clamps ------------------------------------------------------------------------------------------
def test_which_existing_inputs_the_builder_clamps():
    """search_checker.grid_box() on the inputs of test_gpu_outliers.py and test_gpu_clusters.py, so that nobody has to recompute it:
    of the outlier filters' inputs only sor_cloud(20000) is clamped (cloud("far") has 3 005 points: below the builder's 4 096, exact
    box); of the cluster inputs only test_exact_blobs_with_far_outliers, whose outliers touch nothing"""
    from threecrate_amd import synth
    T = _existing_outlier_inputs()
    for name in ("uniform", "lattice", "far", "dup6", "dup2", "five", "one", "nonfinite"):
        assert not SC.grid_box(T.cloud(name))[0], name
    assert len(T.cloud("far")) == 3005
    assert SC.grid_box(OC.sor_cloud(20000))[0] and not SC.grid_box(OC.sor_cloud(2000))[0]
    rng = np.random.default_rng(11)
    blobs = np.concatenate([K.sphere_cloud((0, 0, 0), 1.0, 20000, 1), K.sphere_cloud((3, 0, 0), 0.5, 5000, 2),
                            rng.uniform(-1e5, 1e5, (50, 3)).astype(np.float32)])
    blobs = blobs[rng.permutation(len(blobs))]
    assert SC.grid_box(blobs)[0]
    i, j = K.f32_pairs(blobs, 0.05)
    far = np.nonzero(np.abs(blobs).max(axis=1) > 10)[0]
    assert len(far) >= 45 and not np.isin(i, far).any() and not np.isin(j, far).any()          # no edge outside the box
    others = {"uniform 100k": synth.uniform_cloud(100_000, seed=5), "kitti": synth.kitti_shaped_cloud(), "tum": synth.tum_shaped_cloud(step=2),
              "lattice": K.lattice((40, 30, 20), 0.5), "uniform 50k": synth.uniform_cloud(50000, seed=8)}
    for name, pts in others.items():
        assert not SC.grid_box(pts)[0], name


# ---- (a) clamped_far --------------------------------------------------------------------------------------------------------------
def test_clamped_far_is_clamped_on_every_face_and_its_control_is_not():
    p, rows = C.clamped_far(True)
    base, _ = C.clamped_far(False)
    assert len(base) == C.FAR_N >= 4096 and len(p) == C.FAR_N + 45 and len(rows) == 21
    clamped, lo, hi = SC.grid_box(p)
    assert clamped and (lo > -0.1).all() and (hi < 1.1).all()             # all six faces: the grid spans the cloud proper
    assert (p.min(axis=0) < -1e6).all() and (p.max(axis=0) > 1e6).all()
    assert not SC.grid_box(base)[0]
    out = np.concatenate(rows)
    i = out.astype(np.uint64)
    assert ((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)) != 0).all()       # no sample draws an outlier
    mask = np.ones(len(p), bool)
    mask[out] = False
    assert np.array_equal(p[mask], base)                                   # inserted, not appended: the base keeps its order
    assert out.min() < 10 and out.max() > len(p) - 10 and sorted(len(r) for r in rows) == [2] * 18 + [3] * 3
    for (di, mi, pts), r in zip(C.far_sites(), rows):
        assert np.array_equal(p[r], pts)
        d = np.linalg.norm(pts[0].astype(np.float64) - 0.5) / math.sqrt(3.0)
        assert abs(d / C.FAR_DISTS[mi] - 1) < 0.05
        assert OC.d2_f32(pts[0], pts[1]) == C.FAR_PAIR_D2
        if len(pts) == 3:
            assert OC.d2_f32(pts[0], pts[2]) == C.FAR_PAIR_D2 and OC.d2_f32(pts[1], pts[2]) == C.FAR_THIRD_D2


def test_clamped_far_what_the_filters_make_of_the_pairs_and_triples():
    p, rows = C.clamped_far(True)
    out = np.concatenate(rows)
    pair_rows = np.concatenate([r for r in rows if len(r) == 2])
    triple_rows = np.concatenate([r for r in rows if len(r) == 3])
    # SOR: at k = 1 an outlier's mean is its partner's distance, to the bit
    m1 = C.ref_mean(FAR, 1)
    assert (_bits(m1[out]) == _bits(np.sqrt(C.FAR_PAIR_D2))).all()
    # radius filter: pairs kept at 1 and dropped at 2, triples kept at 2 and dropped at 3
    cnt = C.ref_counts(FAR, C.FAR_RADIUS)
    assert (cnt[pair_rows] == 2).all() and (cnt[triple_rows] == 3).all()
    keep = [set(OC.keep_of_counts(cnt, m).tolist()) for m in (1, 2, 3)]
    assert set(out) <= keep[0] and not set(pair_rows) & keep[1] and set(triple_rows) <= keep[1] and not set(out) & keep[2]
    wide = C.ref_counts(FAR, C.FAR_WIDE_RADIUS)
    near = np.concatenate([r for (_, mi, _), r in zip(C.far_sites(), rows) if mi == 0])
    assert wide.max() == C.FAR_N + len(near) and (wide[np.setdiff1d(out, near)] <= 3).all()         # an interior walk covers everything near
    # clusters: every pair and triple is a component at the tolerance that squares onto 2^-5, a singleton one float below
    t, below = np.float32(C.FAR_TOL), np.float32(C.FAR_TOL_BELOW)
    assert t * t >= C.FAR_PAIR_D2 > below * below and np.float32(np.sqrt(C.FAR_PAIR_D2)) == below
    n = len(p)
    labels, members, offsets = C.ref_clusters(FAR, C.FAR_TOL, 2, n)
    sizes = np.diff(offsets.astype(np.int64))
    assert sizes.tolist() == [C.FAR_N] + [3] * 3 + [2] * 18                   # the base is one component; then by size, then by index
    lists = K.cluster_lists(labels, members, offsets)
    assert sorted(tuple(l) for l in lists[1:]) == sorted(tuple(r) for r in rows)
    assert [l[0] for l in lists[1:4]] == sorted(l[0] for l in lists[1:4]) and [l[0] for l in lists[4:]] == sorted(l[0] for l in lists[4:])
    assert len(C.ref_clusters(FAR, C.FAR_TOL, 3, n)[2]) == 1 + 1 + 3 and len(C.ref_clusters(FAR, C.FAR_TOL, 2, 2)[2]) == 1 + 18
    lb, _, ob = C.ref_clusters(FAR, C.FAR_TOL_BELOW, 2, n)
    assert len(ob) == 2 and (lb[out] == K.NONE).all()


def test_far_plateaus_and_the_checkers_widening_ends():
    """10^6 diagonals out a float32 d2 steps by 2^18: every point of the cloud lies on one of a few plateaus, and the k + 1 nearest
    cut one.  The checker widens those rows to the whole cloud and stops; the time is printed."""
    p, rows = C.clamped_far(True)
    far6 = np.concatenate([r for (_, mi, _), r in zip(C.far_sites(), rows) if mi == 2])
    assert len(far6) == 15
    for i in far6:
        d2 = OC.d2_f32(p[i], p)
        assert len(np.unique(d2[d2 > 1])) <= 40, len(np.unique(d2[d2 > 1]))
    for k in (8, 300):
        widths = []
        t0 = time.perf_counter()
        OC.nearest_d2(p, k + 1, widths)
        dt = time.perf_counter() - t0
        print(f"clamped_far k = {k}: widening {widths}, {dt:.2f} s")
        assert widths[-1][0] == len(p) and 1 <= widths[-1][1] <= 15 and len(widths) <= 12 and dt < 10     # only outlier rows get that far
        assert widths[-1][1] == 15 or k < 300


# ---- (a) block_edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.BLOCK_NS)
def test_block_edges(n):
    p = C.block_cloud(n)
    fin = np.isfinite(p).all(axis=1)
    nfin = int(fin.sum())
    assert nfin == (n - 3 if n >= 63 else n) and n + 3 + 1 > nfin                      # K1 > nfin at k = n + 3
    if n >= 63:
        assert np.isnan(p[0, 0]) and p[n // 2, 1] == np.inf and p[n - 1, 2] == -np.inf
        m = C.ref_mean(("block", n), n + 3)
        assert np.isnan(m[[0, n // 2, n - 1]]).all() and np.isfinite(m[fin]).all()
        keep = OC.keep_of_counts(C.ref_counts(("block", n), C.BLOCK_RADIUS), C.block_min_neighbors(n))
        cube = np.nonzero(fin[:n // 2])[0]
        rest = np.setdiff1d(keep, cube)
        assert set(cube) <= set(keep) and len(rest) < (n - n // 2) / 2, (len(rest), n)   # keeps the cube, drops most of the rest
        labels, _, _ = C.ref_clusters(("block", n), C.BLOCK_TOL, 1, n)
        assert (np.bincount(labels)[labels[~fin]] == 1).all()                        # inert rows are singletons


def test_triples130():
    p = C.triples130()
    labels, members, offsets = C.ref_clusters(("triples130",), 0.05, 1, 390)
    assert len(p) == 390 and np.diff(offsets.astype(np.int64)).tolist() == [3] * 130
    assert [l.tolist() for l in K.cluster_lists(labels, members, offsets)] == [[c, c + 130, c + 260] for c in range(130)]
    assert len(C.ref_clusters(("triples130",), 0.05, 4, 390)[2]) == 1                # n_clusters == 0


# ---- (a) stats_edges --------------------------------------------------------------------------------------------------------------
def test_stat_block_counts():
    assert [C.stat_blocks(n) for n in C.STAT_NS] == [255, 255, 256, 257, 1024, 1024, 1024, 1024]
    assert [n > 1024 * 256 for n in C.STAT_NS] == [False] * 6 + [True, True]          # the last two have strided elements
    assert C.STAT_NS[6] - 1024 * 256 == 1 and C.STAT_NS[7] - 1024 * 256 == 257        # thread 0 of block 0; block 0 and thread 0 of block 1
    p = C.stat_cloud(C.STAT_NAN_N)
    assert int(np.isnan(p[:, 0]).sum()) == 2621


def _t_f64(mean, mult, mean_div=None, var_div=None):
    mf = np.asarray(mean, np.float32)
    mf = [float(x) for x in mf[~np.isnan(mf)]]
    m64 = math.fsum(mf) / (mean_div or len(mf))
    v64 = math.fsum((x - m64) ** 2 for x in mf) / (var_div or len(mf))
    return np.float32(m64 + float(mult) * math.sqrt(v64))


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.uint32)) - int(np.float32(b).view(np.uint32)))


def test_stats_checker_time_and_thresholds():
    """the checker's time for 262 144 points at k = 1 (printed), and the two threshold mutants against the rule the GPU test holds
    the device to (one ulp from the exactly summed threshold)"""
    n = 262144
    t0 = time.perf_counter()
    m = C.ref_mean(("stat", n), 1)
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    t_ref, t_f64 = OC.thresholds(m, 1.0)
    print(f"stats_edges n = {n}: mean_distances {dt:.2f} s, thresholds {time.perf_counter() - t1:.2f} s, t_f64 = {t_f64!r}, t_ref = {t_ref!r}")
    assert dt < 8 and _t_f64(m, 1.0) == t_f64


# ---- (a) shifted ------------------------------------------------------------------------------------------------------------------
def test_shifted_answers_are_the_unmoved_ones():
    base = C.shifted_cloud(0.0)
    assert len(base) - len(np.unique(base, axis=0)) >= 1                               # the snapped cloud holds exact duplicates
    for s in C.SHIFTS[1:]:
        cloud = ("shifted", s)
        assert np.array_equal(C.shifted_cloud(s) - np.float32(s), base)
        for k in C.SHIFT_KS:
            assert _same(C.ref_mean(cloud, k), C.ref_mean(("shifted", 0.0), k))
        assert np.array_equal(C.ref_counts(cloud, C.SHIFT_RADIUS), C.ref_counts(("shifted", 0.0), C.SHIFT_RADIUS))
        for a, b in zip(C.ref_clusters(cloud, C.SHIFT_TOL, 1, 3000), C.ref_clusters(("shifted", 0.0), C.SHIFT_TOL, 1, 3000)):
            assert np.array_equal(a, b)
    cnt = C.ref_counts(("shifted", 0.0), C.SHIFT_RADIUS)
    d2 = OC.d2_f32(base[:, None, :], base[None, :, :])
    assert int((d2 == np.float32(C.SHIFT_RADIUS) ** 2).sum()) > 0 and cnt.max() > 10   # the relation is met with equality somewhere
    assert 2 < len(C.ref_clusters(("shifted", 0.0), C.SHIFT_TOL, 2, 3000)[2]) < 1500


# ---- (a) cluster_sizes ------------------------------------------------------------------------------------------------------------
def test_cluster_sizes():
    p, comp = C.sized_components()
    labels, members, offsets = C.ref_clusters(("sized",), C.SIZE_TOL, 1, len(p))
    assert sorted(np.bincount(comp).tolist()) == [1] * 6 + [4] * 5 + [5] * 5 + [6] * 5
    assert all(len(set(comp[l])) == 1 for l in K.cluster_lists(labels, members, offsets)) and len(offsets) == 22
    want = {(5, 5): 5, (4, 6): 15, (5, 6): 10, (4, 5): 10, (6, 6): 5, (7, 7): 0}
    for (mn, mx), nc in want.items():
        labels, members, offsets = C.ref_clusters(("sized",), C.SIZE_TOL, mn, mx)
        lists = K.cluster_lists(labels, members, offsets)
        assert len(lists) == nc
        keys = [(-len(l), int(l[0])) for l in lists]
        assert keys == sorted(keys) and all((np.diff(l) > 0).all() for l in lists)   # size descending, then smallest index
        firsts = [int(l[0]) for l in lists if len(l) == 5]
        assert len(set(firsts)) == len(firsts)
    # the components' smallest indices are not in site order: ranking by index differs from ranking by position
    first = [int(np.nonzero(comp == c)[0][0]) for c in range(20) if (comp == c).sum() == 5]
    assert first != sorted(first)


# ---- (a) lattice_shells -----------------------------------------------------------------------------------------------------------
def test_lattice_shell_counts_come_from_the_checker():
    cloud = ("lattice", False)
    for base, counts in zip(SC.SHELL_RADII, SC.SHELL_COUNTS):
        for r, cnt in zip(SC.ulps(base), counts):
            assert C.ref_counts(cloud, r).max() == cnt, (r, cnt)
    ncomp = [len(C.ref_clusters(cloud, r, 1, 1728)[2]) - 1 for r in SC.ulps(0.25)]
    assert ncomp == [1728, 1, 1]
    p = C.lattice_cloud(True)
    rows = C.lattice_pair_rows()
    clamped, lo, hi = SC.grid_box(p)
    assert len(p) == 17 ** 3 + 2 >= 4096 and clamped and hi[0] < 4.5 and np.array_equal(p[rows], C.LATTICE_FAR_PAIR)
    assert [C.ref_counts(("lattice", True), r)[rows].tolist() for r in SC.ulps(0.25)] == [[1, 1], [2, 2], [2, 2]]
    assert [len(C.ref_clusters(("lattice", True), r, 2, len(p))[2]) - 1 for r in SC.ulps(0.25)] == [0, 2, 2]


# ---- (c) mutants ------------------------------------------------------------------------------------------------------------------
def _lists_of(cloud, k):
    p = C.BUILDERS[cloud[0]](*cloud[1:])
    return OC.nearest_d2(p, k + 1), np.isfinite(p).all(axis=1)


def _scatter(fin, m):
    out = np.full(len(fin), np.nan, np.float32)
    out[fin] = m
    return out


def _mean_mutant(d2, rule, k):
    dist, use = np.sqrt(d2), d2 > 0
    s = np.zeros(len(d2), np.float32)
    for j in range(d2.shape[1]):
        s = s + np.where(use[:, j], dist[:, j], np.float32(0))
    cnt = use.sum(1)
    if rule == "self":
        cnt = cnt + 1
    elif rule == "duplicates":
        cnt = cnt + np.maximum((~use).sum(1) - 1, 0)
    elif rule == "by_k":
        cnt = np.full(len(d2), k)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, s / cnt.astype(np.float32), np.float32(0)).astype(np.float32)


def _differs(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return int(((_bits(a) != _bits(b)) & ~(np.isnan(a) & np.isnan(b))).sum())
    return int(a.shape != b.shape or (a != b).any()) if a.shape != b.shape else int((a != b).sum())


def _strict_counts(cloud, radius):
    p = C.BUILDERS[cloud[0]](*cloud[1:])
    fin = np.isfinite(p).all(axis=1)
    r2 = np.float32(radius) * np.float32(radius)
    cnt = np.zeros(len(p), np.int64)
    idx = np.nonzero(fin)[0]
    for s in range(0, len(idx), 256):
        cnt[idx[s:s + 256]] = (OC.d2_f32(p[idx[s:s + 256], None, :], p[None, idx, :]) < r2).sum(axis=1)
    return cnt


def _kept_differs(ref, mut, mins):
    return sum(int(not np.array_equal(OC.keep_of_counts(ref, m), OC.keep_of_counts(mut, m))) for m in mins), len(mins)


def _clusters_differ(a, b):
    return int(any(x.shape != y.shape or (x != y).any() for x, y in zip(a, b)))


def _rank_by_largest(n, i, j, mn, mx):
    """cluster_checker.from_pairs with equal sizes ranked by their LARGEST index"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    ncomp, comp = connected_components(coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n)), directed=False)
    size = np.bincount(comp, minlength=ncomp)
    last = np.zeros(ncomp, np.int64)
    last[comp] = np.arange(n)
    keep = np.nonzero((size >= mn) & (size <= mx))[0]
    order = keep[np.lexsort((last[keep], -size[keep]))]
    rank = np.full(ncomp, K.NONE, np.uint64)
    rank[order] = np.arange(len(order), dtype=np.uint64)
    return rank[comp].astype(np.uint32)


def mutant_table():
    """[(mutant, case id, what the real checker says that the mutant does not)]; every entry names a case of the table"""
    rows = []

    def add(mutant, cid, differs, of, note=""):
        assert cid in BY_ID, cid
        rows.append((mutant, cid, differs, of, note))

    far_p, far_rows = C.clamped_far(True)
    out = np.concatenate(far_rows)
    # d2 < r^2 on a shell radius
    c = BY_ID["lattice_shells-clamped-r0.25-radius"]
    ref, mut = C.ref_counts(c.cloud, 0.25), _strict_counts(c.cloud, 0.25)
    add("`d2 < r^2` (radius filter)", C.case_id(c), *_kept_differs(ref, mut, C.radius_mins(c)), "kept sets over min_neighbors")
    c = BY_ID["lattice_shells-r0.25-cluster"]
    strict = K.f32_pairs(C.case_input(c), float(np.nextafter(np.float32(0.25), np.float32(0))))      # d2 < 0.0625: nothing on a 0.25 lattice
    assert len(strict[0]) == 0
    add("`d2 < r^2` (clusters)", C.case_id(c), _differs(K.from_pairs(1728, *strict, 1, 1728)[0], C.ref_clusters(c.cloud, 0.25, 1, 1728)[0]), 1728, "labels")
    # the far pair not counted / not adjacent
    c = BY_ID["clamped_far-r0.3-radius"]
    ref = C.ref_counts(FAR, C.FAR_RADIUS)
    mut = ref.copy()
    mut[out] = 1
    add("the far pair not counted (radius filter)", C.case_id(c), *_kept_differs(ref, mut, (1, 2, 3)), "kept sets over min_neighbors = 1, 2, 3")
    c = BY_ID["clamped_far-tol_on-cluster"]
    i, j = C.ref_pairs(FAR, C.FAR_TOL)
    cut = ~(np.isin(i, out) & np.isin(j, out))
    n = len(far_p)
    add("the far pair not adjacent (clusters)", C.case_id(c), _differs(K.from_pairs(n, i[cut], j[cut], 2, n)[0], C.ref_clusters(FAR, C.FAR_TOL, 2, n)[0]), n, "labels")
    # the rules of the mean
    d2, fin = _lists_of(FAR, 8)
    real = C.ref_mean(FAR, 8)
    assert _same(_scatter(fin, _mean_mutant(d2, None, 8)), real)
    add("the point itself counted in the mean", "clamped_far-k8-sor", _differs(_scatter(fin, _mean_mutant(d2, "self", 8)), real), len(real), "means")
    cloud = ("shifted", 0.0)
    d2, fin = _lists_of(cloud, 8)
    add("exact duplicates counted in the mean", "shifted-by0-k8-sor", _differs(_scatter(fin, _mean_mutant(d2, "duplicates", 8)), C.ref_mean(cloud, 8)), len(fin),
        "means (the rows that have a twin)")
    cloud = ("block", 63)
    d2, fin = _lists_of(cloud, 66)
    add("the mean divided by k", "block_edges-n63-k66-sor", _differs(_scatter(fin, _mean_mutant(d2, "by_k", 66)), C.ref_mean(cloud, 66)), len(fin), "means")
    d2, fin = _lists_of(cloud, 8)
    add("the mean divided by k", "block_edges-n63-k8-sor", _differs(_scatter(fin, _mean_mutant(d2, "by_k", 8)), C.ref_mean(cloud, 8)), len(fin),
        "means: INVISIBLE where every list is full and free of twins (k == the non-zero count)")
    # count >= min_neighbors
    ref = C.ref_counts(FAR, C.FAR_RADIUS)
    add("`count >= min_neighbors` (self counted)", "clamped_far-r0.3-radius", *_kept_differs(ref, ref + 1, (1, 2, 3)), "kept sets over min_neighbors = 1, 2, 3")
    # the statistics
    m = C.ref_mean(("stat", C.STAT_NAN_N), 1)
    t = OC.thresholds(m, 1.0)[1]
    add("the statistics divided by n, not the finite count", f"stats_edges-n{C.STAT_NAN_N}-nan-stats", int(_ulps(_t_f64(m, 1.0, len(m), len(m)), t) > 1), 1,
        f"threshold {_ulps(_t_f64(m, 1.0, len(m), len(m)), t)} ulps from the exact one (the rule allows 1)")
    for n in (65281, 262144):
        m = C.ref_mean(("stat", n), 1)
        t = OC.thresholds(m, 1.0)[1]
        u = _ulps(_t_f64(m, 1.0, None, len(m) - 1), t)
        add("sample variance", f"stats_edges-n{n}-stats", int(u > 1), 1, f"threshold {u} ulps from the exact one (the rule allows 1)")
    # sizes and ranks
    cloud = ("sized",)
    i, j = C.ref_pairs(cloud, C.SIZE_TOL)
    n = len(C.sized_components()[0])
    for name, dmn, dmx in (("size filter `size > min`", 1, 0), ("size filter `size < max`", 0, -1)):
        bad = sum(_clusters_differ(K.from_pairs(n, i, j, mn + dmn, mx + dmx) if mn + dmn <= mx + dmx else K.from_pairs(n, i, j, n + 1, n + 1),
                                   C.ref_clusters(cloud, C.SIZE_TOL, mn, mx)) for mn, mx in C.SIZE_WINDOWS)
        add(name, "cluster_sizes-windows-cluster", bad, len(C.SIZE_WINDOWS), "windows with another answer ((7, 7) is empty either way)")
    bad = sum(int((_rank_by_largest(n, i, j, mn, mx) != C.ref_clusters(cloud, C.SIZE_TOL, mn, mx)[0]).any()) for mn, mx in C.SIZE_WINDOWS)
    add("equal sizes ranked by largest index", "cluster_sizes-windows-cluster", bad, len(C.SIZE_WINDOWS), "windows with other labels")
    # a non-finite point joined to its neighbour in index order
    cloud = ("block", 63)
    i, j = C.ref_pairs(cloud, C.BLOCK_TOL)
    inert = np.nonzero(~np.isfinite(C.block_cloud(63)).all(axis=1))[0]
    lo, hi = np.minimum(inert, (inert + 1) % 63), np.maximum(inert, (inert + 1) % 63)
    add("a non-finite point joined to a neighbour", "block_edges-n63-cluster",
        _differs(K.from_pairs(63, np.concatenate([i, lo]), np.concatenate([j, hi]), 1, 63)[0], C.ref_clusters(cloud, C.BLOCK_TOL, 1, 63)[0]), 63, "labels")
    # a neighbour one plateau farther, 10^6 diagonals out: from the whole cloud, which is what the checker widens these rows to
    far6 = np.concatenate([r for (_, mi, _), r in zip(C.far_sites(), far_rows) if mi == 2])
    for k in C.FAR_KS:
        real = C.ref_mean(FAR, k)
        moved = 0
        for r in far6:
            full = np.sort(OC.d2_f32(far_p[r], far_p))
            lst = full[:k + 1].copy()
            assert _bits(OC.means_of_lists(lst[None]))[0] == _bits(real[r:r + 1])[0]
            beyond = full[full > lst[-1]]
            lst[-1] = beyond[0]
            moved += int(_bits(OC.means_of_lists(lst[None]))[0] != _bits(real[r:r + 1])[0])
        note = "outlier rows with another mean" + ("" if moved else ": INVISIBLE, one ulp of one term is absorbed by the f32 sum")
        add("a neighbour one plateau farther, 10^6 diagonals out", f"clamped_far-k{k}-sor", moved, len(far6), note)
    return rows


def test_every_mutant_is_failed_by_a_named_case():
    rows = mutant_table()
    shown = {}
    for mutant, cid, differs, of, note in rows:
        print(f"{mutant} | {cid}: {differs} / {of} {note}")
        shown[mutant] = shown.get(mutant, 0) + int(differs > 0)
    assert all(v > 0 for v in shown.values()), {m: v for m, v in shown.items() if v == 0}
    assert len(shown) == 15
    # the two that a case cannot show are stated, not dropped
    by = {(m, cid): d for m, cid, d, _, _ in rows}
    assert by[("the mean divided by k", "block_edges-n63-k8-sor")] == 0 and by[("the mean divided by k", "block_edges-n63-k66-sor")] > 0
    assert by[("a neighbour one plateau farther, 10^6 diagonals out", "clamped_far-k2-sor")] > 0
    assert by[("the far pair not counted (radius filter)", "clamped_far-r0.3-radius")] == 2           # at min_neighbors 1 and 2
    assert by[("`count >= min_neighbors` (self counted)", "clamped_far-r0.3-radius")] >= 2


if __name__ == "__main__":
    print("| mutant | case | differs |")
    print("|---|---|---|")
    for mutant, cid, differs, of, note in mutant_table():
        print(f"| {mutant} | `{cid}` | {differs} / {of} {note} |")
