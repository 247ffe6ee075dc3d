"""Checker for the neighbour-search exports (nearest_neighbor.rs:177-298), shared by test_search_cpu.py and
test_gpu_search_edges.py: the contract in numpy, the input families, and a restatement of the index builder's box rule.

Distances are d2 = (dx*dx + dy*dy) + dz*dz in float32 with dx = p - q (nearest_neighbor.rs:162-167; numpy rounds every operation
and never fuses), for every cloud point with three finite coordinates; a point with a non-finite coordinate is inert (the backend's
documented deviation) and counts as infinitely far, and so does every point for a query with a non-finite coordinate.

check_knn judges a k-NN / radius-among-the-k-nearest result without caring which tie was chosen:
  count       min(k, finite points); with a radius the number of the k nearest with d2 <= f32(radius) * f32(radius), 0 unless
              radius > 0 (nearest_neighbor.rs:255-257; a NaN radius compares false everywhere); 0 for a non-finite query;
  distances   dist[:count] is sqrt of the count smallest d2, ascending, bit for bit -- a multiset no tie-break can change;
  indices     idx[:count] distinct, in range, naming finite points, sqrt(d2[idx[j]]) with the bits of dist[j], and the d2 of the
              named points are, as a multiset, the count smallest (sqrt maps two neighbouring d2 to one float: the distances
              alone would let a point one ulp too far through).  ranked_by="dist" drops this last clause and calls equal
              DISTANCES at the cut a tie: BruteForceSearch (nearest_neighbor.rs:340-362) sorts by sqrt(d2), the kd-tree and the
              kernels rank by d2;
  no tie      where the count-th and the next d2 differ the index set is THE brute-force set; the report counts these queries.
check_radius_all judges the unbounded radius search: per query the index set exact, the segment ascending, distances bit for bit.

Entries past count are never read."""
import collections
import functools

import numpy as np

from threecrate_amd import synth

U32 = np.uint32
Report = collections.namedtuple("Report", "queries finite_queries no_tie")


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


class Brute:
    """d2 (nq, n) of every query to every point and the same rows sorted; computed once per (cloud, queries) and shared"""

    def __init__(self, points, queries, _parts=None):
        if _parts is not None:
            self.fin, self.nfin, self.qfin, self.d2, self.sd2 = _parts
            return
        p, q = _f32(points), _f32(queries)
        self.fin = np.all(np.isfinite(p), axis=1)
        self.nfin = int(self.fin.sum())
        self.qfin = np.all(np.isfinite(q), axis=1)
        self.d2 = np.empty((len(q), len(p)), np.float32)
        step = max(1, (1 << 22) // max(len(p), 1))
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for a in range(0, len(q), step):
                dx = p[None, :, 0] - q[a:a + step, None, 0]
                dy = p[None, :, 1] - q[a:a + step, None, 1]
                dz = p[None, :, 2] - q[a:a + step, None, 2]
                self.d2[a:a + step] = (dx * dx + dy * dy) + dz * dz
        self.d2[:, ~self.fin] = np.inf
        self.d2[~self.qfin, :] = np.inf
        self.sd2 = np.sort(self.d2, axis=1)

    def rows(self, sel):
        """the queries `sel` (a slice or an index array)"""
        return Brute(None, None, (self.fin, self.nfin, self.qfin[sel], self.d2[sel], self.sd2[sel]))

    def head(self, nq):
        """the first nq queries"""
        return self.rows(slice(0, nq))


def radius_sq(radius):
    """f32(radius) * f32(radius), or None when the radius admits nothing (radius <= 0, NaN)"""
    r = np.float32(radius)
    return r * r if r > 0 else None


def _first(mask):
    return tuple(int(v) for v in np.argwhere(mask)[0])


def check_knn(points, queries, k, idx, dist, count, radius=None, brute=None, ranked_by="d2"):
    b = brute if brute is not None else Brute(points, queries)
    nq, n = b.d2.shape
    k = int(k)
    count = np.asarray(count).reshape(-1).astype(np.int64)
    assert len(count) == nq, (len(count), nq)
    K1 = min(k, b.nfin)
    head = b.sd2[:, :K1]
    if radius is None:
        m = np.full(nq, K1, np.int64)
    else:
        r2 = radius_sq(radius)
        m = (head <= r2).sum(axis=1).astype(np.int64) if r2 is not None else np.zeros(nq, np.int64)
    m[~b.qfin] = 0
    bad = count != m
    assert not bad.any(), f"count: query {_first(bad)[0]} has {count[bad][0]}, expected {m[bad][0]} ({int(bad.sum())} queries differ)"
    nofin = int(b.qfin.sum())
    if K1 == 0 or not m.any():
        return Report(nq, nofin, nq)
    idx = np.asarray(idx).reshape(nq, -1)[:, :K1].astype(np.int64)
    dist = np.ascontiguousarray(np.asarray(dist, np.float32).reshape(nq, -1)[:, :K1])
    live = np.arange(K1)[None, :] < m[:, None]
    # distances: the m smallest, ascending, bit for bit
    bad = live & (dist.view(U32) != np.sqrt(head).view(U32))
    assert not bad.any(), f"dist: (query, rank) {_first(bad)}: {dist[bad][0]!r}, expected {np.sqrt(head)[bad][0]!r} ({int(bad.sum())} entries)"
    # indices: in range, finite points, distinct
    bad = live & ((idx < 0) | (idx >= n))
    assert not bad.any(), f"idx out of range at (query, rank) {_first(bad)}: {idx[bad][0]}"
    safe = np.where(live, idx, 0)
    bad = live & ~b.fin[safe]
    assert not bad.any(), f"idx names a non-finite point at (query, rank) {_first(bad)}"
    member = np.zeros((nq, n + 1), bool)
    np.put_along_axis(member, np.where(live, idx, n), True, axis=1)
    member = member[:, :n]
    bad = member.sum(axis=1) != m
    assert not bad.any(), f"idx: query {_first(bad)[0]} names a point twice"
    # every named point lies where its distance says, and the named d2 are the m smallest
    g = np.take_along_axis(b.d2, safe, axis=1)
    bad = live & (np.sqrt(g).view(U32) != dist.view(U32))
    assert not bad.any(), f"idx/dist: (query, rank) {_first(bad)}: point {idx[bad][0]} is {np.sqrt(g)[bad][0]!r} away, dist says {dist[bad][0]!r}"
    for t in np.nonzero((live & (g.view(U32) != head.view(U32))).any(axis=1))[0] if ranked_by == "d2" else ():     # as multisets
        assert np.array_equal(np.sort(g[t, :m[t]]), head[t, :m[t]]), f"idx: query {t}: the named points are not the {m[t]} nearest"
    # no tie at the cut: the set is the brute-force set
    tie = np.zeros(nq, bool)
    if K1 < n:
        tie = (m == K1) & ((b.sd2[:, K1 - 1] == b.sd2[:, K1]) if ranked_by == "d2" else (np.sqrt(b.sd2[:, K1 - 1]) == np.sqrt(b.sd2[:, K1])))
    sure = ~tie & (m > 0)
    cut = b.sd2[np.arange(nq), np.maximum(m, 1) - 1]
    bad = sure & (member != (b.d2 <= cut[:, None])).any(axis=1)
    assert not bad.any(), f"set: query {_first(bad)[0]} has no tie at the cut and not the brute-force set"
    return Report(nq, nofin, int((~tie).sum()))


def check_radius_all(points, queries, radius, offsets, idx, dist, brute=None):
    b = brute if brute is not None else Brute(points, queries)
    nq, n = b.d2.shape
    offsets = np.asarray(offsets).astype(np.int64)
    idx, dist = np.asarray(idx).astype(np.int64), np.asarray(dist, np.float32)
    assert len(offsets) == nq + 1 and offsets[0] == 0 and offsets[-1] == len(idx) == len(dist), (len(offsets), nq, len(idx), len(dist))
    r2 = radius_sq(radius)
    total = 0
    for t in range(nq):
        want = np.nonzero(b.d2[t] <= r2)[0] if r2 is not None else np.zeros(0, np.int64)
        got, seg = idx[offsets[t]:offsets[t + 1]], dist[offsets[t]:offsets[t + 1]]
        assert len(got) == len(want), f"count: query {t} has {len(got)}, expected {len(want)}"
        assert np.array_equal(np.sort(got), want), f"set: query {t}"
        assert np.all(seg[1:] >= seg[:-1]), f"order: query {t} is not ascending"
        assert np.array_equal(seg.view(U32), np.sqrt(b.d2[t, got]).view(U32)), f"dist: query {t}"
        total += len(want)
    return total


# ---- the index builder's box rule, restated (grid.hip: bbox_kernel's samples, cloud_bbox_impl's comparison) ---------------------
def grid_box(points):
    """(clamped, lo, hi): the box the grid of an index over `points` spans.  Per axis the exact range of the finite points, unless
    the cloud has at least 4096 points and the third-lowest minimum / third-highest maximum of four sample boxes say that the exact
    range is more than 1.3 x wider than the cloud proper: then the sampled range + 5 %.  Sample s holds the points with index = s
    mod 4 whose hash (index * 2654435761 mod 2^32) >> 28 is zero."""
    p = _f32(points)
    i = np.arange(len(p), dtype=np.uint64)
    fin = np.all(np.abs(p) <= np.float32(3.0e38), axis=1)
    lo, hi = p[fin].min(axis=0), p[fin].max(axis=0)
    clamped = False
    if len(p) < 4096:
        return clamped, lo, hi
    drawn = fin & ((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)) == 0)
    smin = np.full((4, 3), np.inf, np.float32)
    smax = np.full((4, 3), -np.inf, np.float32)
    for s in range(4):
        sel = p[drawn & ((i & np.uint64(3)) == s)]
        if len(sel):
            smin[s], smax[s] = sel.min(axis=0), sel.max(axis=0)
    lo, hi = lo.copy(), hi.copy()
    for c in range(3):
        slo, shi = np.sort(smin[:, c])[2], np.sort(smax[:, c])[::-1][2]
        if not (slo <= shi) or not np.isfinite(slo) or not np.isfinite(shi):
            continue
        ext, full = np.float32(shi - slo), np.float32(hi[c] - lo[c])
        if not (full > np.float32(1.3) * ext) or not (full > 0):
            continue
        lo[c] = max(lo[c], np.float32(slo - np.float32(0.05) * ext))
        hi[c] = min(hi[c], np.float32(shi + np.float32(0.05) * ext))
        clamped = True
    return clamped, lo, hi


# ---- the input families ---------------------------------------------------------------------------------------------------------
# Every builder returns (points, queries), float32, read-only, built once.
LIST_KS = (1, 9, 10, 17, 18, 33, 34, 65, 66, 129, 130, 256, 257, 2048)        # either side of every list size, and the ends
SHELL_RADII = (0.25, float(np.float32(0.25) * np.sqrt(np.float32(2.0))), 0.5)  # lattice shells of 6, 12 and 6 points (8 more at 0.25 sqrt(3))
# points within (one ulp below, the radius, one ulp above) of an interior lattice point, itself included: 0.25 and 0.5 square onto
# their shells; f32(0.25 sqrt 2) squares to 0.12499999, one ulp BELOW the shell's 0.125, and only the next float holds the shell
SHELL_COUNTS = ((1, 7, 7), (7, 7, 19), (27, 33, 33))
FAR_SHIFTS = (2.0 ** 10, 2.0 ** 13, 2.0 ** 16)
FAR_KS = (10, 66, 130, 300)
DUP_KS = (17, 65, 129, 130, 300)
SMALL_KS = (9, 129, 130, 257)
NQ_SMALL = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257)
NQ_SMALL_KS = (8, 40, 100)
NQ_LARGE = (65535, 65536, 65537, 70000)
NQ_LARGE_K, NQ_LARGE_RADIUS = 130, 0.55
CLAMPED_KS = (9, 17, 33, 65, 129, 130, 300)      # every register list with the clamped box, and both block-per-query buffers
CLAMPED_RADIUS = 0.2
DEGENERATE_KS = (9, 33, 129, 130, 300)


def _ro(*arrays):
    out = tuple(np.ascontiguousarray(a, np.float32) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def ulps(x):
    """(one ulp below, x, one ulp above) in float32"""
    x = np.float32(x)
    return float(np.nextafter(x, np.float32(0))), float(x), float(np.nextafter(x, np.float32(np.inf)))


@functools.lru_cache(maxsize=None)
def uniform():
    """3000 uniform points; queries inside, around (up to one box edge outside) and on the points"""
    pts = synth.uniform_cloud(3000, seed=2)
    return _ro(pts, np.concatenate([synth.uniform_cloud(200, seed=12), synth.uniform_cloud(60, seed=13) * 3.0 - 1.0, pts[:40]]))


def _lattice_points(m=12, spacing=0.25):
    g = np.arange(m, dtype=np.float32) * np.float32(spacing)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def lattice(copies=1):
    """12 x 12 x 12 points, spacing 0.25 (exact in f32), each stored `copies` times; queries: the lattice points and the cell centres.
    Every shell around either kind of query holds several equidistant points."""
    pts = _lattice_points()
    centres = _lattice_points(11) + np.float32(0.125)
    return _ro(np.tile(pts, (copies, 1)), np.concatenate([pts, centres]))


@functools.lru_cache(maxsize=None)
def duplicates():
    """200 sites, 40 exact copies each, shuffled; queries: the sites and 100 other places"""
    sites = synth.uniform_cloud(200, seed=41)
    pts = np.repeat(sites, 40, axis=0)[np.random.default_rng(3).permutation(8000)]
    return _ro(pts, np.concatenate([sites, synth.uniform_cloud(100, seed=42) * 1.5 - 0.25]))


@functools.lru_cache(maxsize=None)
def small(n):
    """n uniform points; queries on them, inside and around"""
    pts = synth.uniform_cloud(n, seed=7)
    return _ro(pts, np.concatenate([pts[:10], synth.uniform_cloud(30, seed=8), synth.uniform_cloud(24, seed=9) * 4.0 - 1.5]))


def small_sizes(k):
    return (1, 2, k - 1, k, k + 1)


@functools.lru_cache(maxsize=None)
def degenerate(kind):
    """identical: 500 copies of one point (a box without extent); line_x / line_diag: 2000 points, spacing 1/64, along x / along the
    diagonal; plane: 4000 points with z = 0.5; ball_far: 3000 points in a ball of diameter 1 and 30 spread over 100 diameters"""
    t = np.arange(2000, dtype=np.float32) / np.float32(64)
    around = synth.uniform_cloud(40, seed=19) * 3.0 - 1.0
    if kind == "identical":
        one = np.array([0.3, -1.25, 2.0], np.float32)
        return _ro(np.tile(one, (500, 1)), np.concatenate([one[None], one[None] + np.float32(0.5), around, around * 50.0]))
    if kind == "line_x":
        pts = np.stack([t, np.full_like(t, 0.5), np.full_like(t, -0.25)], axis=1)
        return _ro(pts, np.concatenate([pts[::37], pts[::41] + np.float32(1 / 128), around * [10.0, 1.0, 1.0]]))
    if kind == "line_diag":
        pts = np.stack([t, t, t], axis=1)
        return _ro(pts, np.concatenate([pts[::37], pts[::41] + np.float32(1 / 128), around * 10.0]))
    if kind == "plane":
        pts = synth.uniform_cloud(4000, seed=23)
        pts[:, 2] = 0.5
        return _ro(pts, np.concatenate([pts[:60], synth.uniform_cloud(60, seed=24), around]))
    assert kind == "ball_far"
    u = synth.uniform_cloud(12000, seed=27) - np.float32(0.5)
    ball = u[np.sum(u.astype(np.float64) ** 2, axis=1) <= 0.25][:3000]
    far = (synth.uniform_cloud(30, seed=28) - np.float32(0.5)) * np.float32(100.0)
    assert len(ball) == 3000
    return _ro(np.concatenate([ball, far]), np.concatenate([ball[:60], far, (synth.uniform_cloud(80, seed=29) - np.float32(0.5)) * np.float32(100.0)]))


DEGENERATE_KINDS = ("identical", "line_x", "line_diag", "plane", "ball_far")
NONFINITE_QUERIES = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.nan, np.nan], [np.inf, -np.inf, np.nan]], np.float32)


@functools.lru_cache(maxsize=None)
def placed_queries():
    """the uniform cloud; queries inside it, on its box faces and corners, 1 / 10^3 / 10^6 box diagonals outside in 13 directions, and
    a NaN / +-inf query after every sixth finite one"""
    pts = uniform()[0]
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    inside = synth.uniform_cloud(64, seed=31) * (hi - lo) + lo
    faces = inside[:36].copy()
    for j in range(36):
        faces[j, j % 3] = (lo, hi)[(j // 3) % 2][j % 3]
    corners = np.array([[(lo, hi)[(c >> a) & 1][a] for a in range(3)] for c in range(8)], np.float32)
    dirs = np.array([d for d in np.ndindex(3, 3, 3) if d != (1, 1, 1)][::2], np.float32) - 1.0
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    diag = np.float32(np.linalg.norm(hi - lo))
    outside = np.concatenate([(lo + hi) / 2 + dirs * (diag * np.float32(mult)) for mult in (1.5, 1.0e3, 1.0e6)])
    finite = np.concatenate([inside, faces, corners, outside]).astype(np.float32)
    rows = []
    for j, q in enumerate(finite):
        rows.append(q)
        if j % 6 == 5:
            rows.append(NONFINITE_QUERIES[(j // 6) % len(NONFINITE_QUERIES)])
    return _ro(pts, np.array(rows, np.float32))


@functools.lru_cache(maxsize=None)
def many_queries():
    """300 points and 70 000 queries around them: more queries than the block-per-query kernel has blocks (65 536); query j and query
    j + 65 536 are unrelated draws"""
    return _ro(synth.uniform_cloud(300, seed=51), synth.uniform_cloud(70000, seed=52) * 2.0 - 0.5)


@functools.lru_cache(maxsize=None)
def far_outliers():
    """the 6000-point input of test_far_outliers_clamped_grid_stays_exact (five far outliers stretch the exact box; the grid spans the
    cloud proper), with more inlier queries"""
    n = 6000
    rng = np.random.default_rng(5)
    pts = synth.uniform_cloud(n, 31, (4.0, 3.0, 1.0)).copy()
    out = np.array([[120, 1.5, 0.5], [120.004, 1.5, 0.5], [2, -300, 0.4], [1, 2, 90], [-50, -60, -70]], np.float32)
    where = rng.integers(0, n, len(out))
    pts[where] = out
    qs = np.concatenate([pts[where], pts[rng.integers(0, n, 40)], np.array([[300, 300, 300], [121, 1.5, 0.5], [2, 1, -40]], np.float32),
                         synth.uniform_cloud(150, 32, (4.0, 3.0, 1.0)), synth.uniform_cloud(60, 33, (8.0, 6.0, 2.0)) - np.float32(1.0)])
    return _ro(pts, qs)


@functools.lru_cache(maxsize=None)
def shifted(kind, shift):
    """`kind` ("uniform": snapped to the grid of the binade of `shift` first, so the sums below are exact; "lattice") moved by `shift`
    along every axis; shift 0: the snapped cloud where it was.  Differences between points and queries are the same at every shift."""
    pts, qs = uniform() if kind == "uniform" else lattice()
    if kind == "uniform":
        step = np.float32(2.0 ** 16 * 2.0 ** -23)                # one ulp in [2^16, 2^17): exact at every smaller shift too
        pts, qs = np.round(pts / step) * step, np.round(qs / step) * step
    return _ro(pts + np.float32(shift), qs + np.float32(shift))


# ---- the cases: what test_search_cpu.py proves on the oracle and test_gpu_search_edges.py runs on the device ----------------------
# cloud: the builder call as (function name, arguments); nq: the first nq queries only (None: all); radius None: k-NN
Case = collections.namedtuple("Case", "family cloud k radius nq")


def case_id(c):
    return "-".join([c.family, *(str(a) for a in c.cloud[1]), f"k{c.k}"] + ([f"r{c.radius!r}"] if c.radius is not None else []) +
                    ([f"nq{c.nq}"] if c.nq is not None else []))


def case_input(c):
    """(points, queries, Brute) of a case; the Brute of a cloud is computed once and cut to the case's queries"""
    pts, qs = globals()[c.cloud[0]](*c.cloud[1])
    b = _brute(c.cloud)
    return (pts, qs, b) if c.nq is None else (pts, qs[:c.nq], b.head(c.nq))


@functools.lru_cache(maxsize=None)
def _brute(cloud):
    return Brute(*globals()[cloud[0]](*cloud[1]))


def knn_cases():
    out = []
    out += [Case("lists", ("uniform", ()), k, None, None) for k in LIST_KS]
    out += [Case("lattice", ("lattice", (1,)), k, None, None) for k in LIST_KS]
    out += [Case("lattice3", ("lattice", (3,)), k, None, None) for k in LIST_KS]
    out += [Case("duplicates", ("duplicates", ()), k, None, None) for k in DUP_KS]
    out += [Case("small", ("small", (n,)), k, None, None) for k in SMALL_KS for n in small_sizes(k)]
    out += [Case("degenerate", ("degenerate", (kind,)), k, None, None) for kind in DEGENERATE_KINDS for k in DEGENERATE_KS]
    out += [Case("placed", ("placed_queries", ()), k, None, None) for k in DEGENERATE_KS]
    out += [Case("nq", ("uniform", ()), k, None, nq) for k in NQ_SMALL_KS for nq in NQ_SMALL]
    out += [Case("clamped", ("far_outliers", ()), k, r, None) for r in (None, CLAMPED_RADIUS) for k in CLAMPED_KS]
    out += [Case("shifted", ("shifted", (kind, s)), k, None, None) for kind in ("uniform", "lattice") for s in FAR_SHIFTS for k in FAR_KS]
    for base, counts in zip(SHELL_RADII, SHELL_COUNTS):           # k_max below, at and above the true count
        out += [Case("shell_radius", ("lattice", (1,)), k, r, None) for r, cnt in zip(ulps(base), counts) for k in (cnt - 1, cnt, cnt + 1) if k]
    out += [Case("no_radius", ("lattice", (1,)), 8, r, None) for r in (0.0, -1.0, float("nan"))]
    return out


def many_query_cases():
    return [Case("many_queries", ("many_queries", ()), NQ_LARGE_K, r, nq) for r in (None, NQ_LARGE_RADIUS) for nq in NQ_LARGE]


def radius_all_cases():
    """(id, cloud, radius, nq) of the unbounded radius search"""
    out = [("shell", ("lattice", (1,)), r, None) for base in SHELL_RADII for r in ulps(base)]
    out += [("nq", ("uniform", ()), 0.12, nq) for nq in (127, 128, 129)]
    out += [("every_second_empty", ("gapped_queries", ()), 0.1, None), ("whole_cloud", ("uniform", ()), 10.0, 129),
            ("clamped", ("far_outliers", ()), 0.2, None), ("clamped_wide", ("far_outliers", ()), 2.5, 64),
            ("no_radius", ("uniform", ()), 0.0, 129), ("no_radius", ("uniform", ()), float("nan"), 129)]
    return [(f"{name}-r{r!r}" + (f"-nq{nq}" if nq else ""), cloud, r, nq) for name, cloud, r, nq in out]


@functools.lru_cache(maxsize=None)
def gapped_queries():
    """the uniform cloud; every second query lies 5 units away from it: zero-length segments between filled ones"""
    pts, qs = uniform()
    qs = qs[:128].copy()
    qs[1::2] += np.float32(5.0)
    return _ro(pts, qs)
