"""One table of edge cases for the statistical filter, the radius filter and cluster extraction, read by tests/test_filter_edges_cpu.py
(which proves on the checkers alone what every case is there for) and by tests/test_gpu_filter_edges.py (which runs them on the
device).  The contracts are tests/outlier_checker.py and tests/cluster_checker.py; their answers are computed once per process.

Which kernel a case reaches.  sor_device() picks by k + 1: <= 9 sor_mean_kernel<9, 256>, <= 17 <17, 256>, <= 33 <33, 128>, <= 65
<65, 64>, <= 129 <129, 64>, <= 256 sor_mean_coop_kernel<512>, else <4096>; the EXT argument (and radius_keep_kernel<EXT>,
clu_hook_kernel<EXT>) is true when the index builder clamps the grid's box, which search_checker.grid_box() restates: nothing visible
from Python names the instantiation.  So FAR_KS = 1, 2, 8 | 16 | 32 | 64 | 128 | 129 | 300 is every list and both block buffers.
The statistics run min(ceil(n / 256), 1024) blocks of 256 (stat_blocks()).

Families: clamped_far (6 000 uniform points + pairs and triples 1.5 / 10^3 / 10^6 box diagonals out in seven directions, inserted at
rows the builder's hashed samples do not draw; the cloud without them is the exact-box control), block_edges (n either side of 64,
128, 256, 512 with inert rows; 130 interleaved components of three), stats_edges (the threshold's partial sums at 255 / 256 / 257
blocks and at the first strided elements), shifted (search_checker.shifted's clouds), cluster_sizes (components of 4, 5, 6 under size
windows that touch them) and lattice_shells (radii on and next to the shells of a lattice, plain and with a far pair)."""
import collections
import functools
import math

import numpy as np

from tests import cluster_checker as K
from tests import outlier_checker as OC
from tests import search_checker as SC

Case = collections.namedtuple("Case", "family name op cloud params")
# op "sor": params (k,); "stats": (k,), every multiplier of OC.SOR_MULTIPLIERS; "radius": (radius, mins or None = derived_mins());
# "cluster": (tolerance, ((min, max), ...))


def _ro(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


def undrawn_rows(n, want):
    """`want` rows spread over [0, n) that the index builder's four hashed sample boxes do not draw (search_checker.grid_box)"""
    i = np.arange(n, dtype=np.uint64)
    drawn = (((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(28)) == 0
    rows = []
    for r in np.linspace(1, n - 2, want).astype(np.int64):
        while drawn[r] or (rows and r <= rows[-1]):
            r += 1
        rows.append(int(r))
    assert len(rows) == want and rows[-1] < n
    return np.array(rows, np.int64)


def insert_rows(base, rows, extra):
    """a cloud of len(base) + len(extra) points with extra[j] at index rows[j] and the base points, in order, everywhere else"""
    n = len(base) + len(extra)
    out = np.empty((n, 3), np.float32)
    mask = np.zeros(n, bool)
    mask[rows] = True
    out[rows] = extra
    out[~mask] = base
    return out


# ---- 1. clamped_far ---------------------------------------------------------------------------------------------------------------
FAR_SEED = 0                                        # the first seed at which grid_box() clamps all six faces (with these rows: any)
FAR_N = 6000
FAR_DIRS = ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1))
FAR_DISTS = (1.5, 1.0e3, 1.0e6)                     # box diagonals from the cloud's centre
FAR_TRIPLES = ((1, 0), (4, 1), (3, 2))              # (direction, distance): -x at 1.5, +z at 10^3, -y at 10^6
FAR_KS = (1, 2, 8, 16, 32, 64, 128, 129, 300)
FAR_CONTROL_KS = (8, 64, 300)
FAR_STEP = np.float32(0.125)                        # one ulp at 10^6 diagonals: every outlier coordinate is a multiple of it
FAR_PAIR_D2 = np.float32(2.0 * 0.125 ** 2)          # partner = site + 0.125 along two axes across the outward one: d2 = 2^-5 exactly
FAR_THIRD_D2 = np.float32(0.25 ** 2)                # the third point mirrors the partner: 0.25 from it, sqrt(2^-5) from the site
FAR_RADIUS = 0.3                                    # pair and triple inside one ball, 0.5 r = 0.15 < 0.177 < 0.25 < r
FAR_WIDE_RADIUS = float(np.float32(2.0 * math.sqrt(3.0)))       # two box diagonals: an interior point's walk covers the grid


def _tol_on(d2):
    """the smallest float32 t with t * t >= d2 in float32 (f32(sqrt(2^-5)) squares to one ulp below 2^-5)"""
    t = np.float32(np.sqrt(np.float32(d2)))
    while t * t >= np.float32(d2):
        t = np.nextafter(t, np.float32(0))
    while t * t < np.float32(d2):
        t = np.nextafter(t, np.float32(np.inf))
    return float(t)


FAR_TOL = _tol_on(FAR_PAIR_D2)
FAR_TOL_BELOW = float(np.nextafter(np.float32(FAR_TOL), np.float32(0)))


@functools.lru_cache(None)
def far_sites():
    """[(direction, distance index, (site, partner[, third]) as float32 rows)]"""
    out = []
    centre, diag = np.full(3, 0.5), math.sqrt(3.0)
    for di, d in enumerate(FAR_DIRS):
        u = np.array(d, np.float64) / np.linalg.norm(d)
        for mi, mult in enumerate(FAR_DISTS):
            site = (np.round((centre + u * (diag * mult)) / 0.125) * 0.125).astype(np.float32)
            assert np.array_equal(site.astype(np.float64), np.round(site.astype(np.float64) / 0.125) * 0.125)
            if sum(map(abs, d)) == 1:
                b, c = [a for a in range(3) if d[a] == 0]
                e1, e2 = np.zeros(3, np.float32), np.zeros(3, np.float32)
                e1[[b, c]] = FAR_STEP
                e2[b], e2[c] = FAR_STEP, -FAR_STEP
            else:
                e1 = np.array([FAR_STEP, -FAR_STEP, 0], np.float32)
                e2 = None
            pts = [site, site + e1]
            if (di, mi) in FAR_TRIPLES:
                pts.append(site + e2)
            out.append((di, mi, np.array(pts, np.float32)))
    return out


@functools.lru_cache(None)
def clamped_far(outliers=True):
    """-> (points, rows): rows[s] = the indices of site s's points (far_sites() order); without outliers: the 6 000 base points"""
    base = np.random.default_rng(FAR_SEED).random((FAR_N, 3), dtype=np.float32)
    if not outliers:
        return _ro(base), ()
    extra = np.concatenate([p for _, _, p in far_sites()])
    where = undrawn_rows(FAR_N + len(extra), len(extra))
    rows, at = [], 0
    for _, _, p in far_sites():
        rows.append(where[at:at + len(p)])
        at += len(p)
    return _ro(insert_rows(base, where, extra)), tuple(rows)


# ---- 2. block_edges ---------------------------------------------------------------------------------------------------------------
BLOCK_NS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
BLOCK_RADIUS = 0.18                                 # above the cube's diagonal (0.1 sqrt 3): every cube point sees the whole cube
BLOCK_TOL = 0.05


@functools.lru_cache(None)
def block_cloud(n):
    """first half in a cube of edge 0.1, second half uniform in the unit cube; NaN / +inf / -inf rows at 0, n // 2, n - 1 (n >= 63)"""
    rng = np.random.default_rng(100 + n)
    half = n // 2
    p = np.concatenate([rng.random((half, 3), dtype=np.float32) * np.float32(0.1) + np.float32(0.45), rng.random((n - half, 3), dtype=np.float32)])
    if n >= 63:
        p[0, 0], p[n // 2, 1], p[n - 1, 2] = np.nan, np.inf, -np.inf
    return _ro(p)


def block_min_neighbors(n):
    return max(1, n // 4)


@functools.lru_cache(None)
def triples130():
    """130 components of three points 0.03 apart (tolerance 0.05) on sites 0.5 apart; component c is the points c, c + 130, c + 260"""
    sites = np.array([s for s in np.ndindex(6, 6, 4)][:130], np.float32) * np.float32(0.5)
    p = np.concatenate([sites + np.array([j * 0.03, 0, 0], np.float32) for j in range(3)])
    return _ro(p)


# ---- 3. stats_edges ---------------------------------------------------------------------------------------------------------------
STAT_NS = (65279, 65280, 65281, 65537, 262143, 262144, 262145, 262144 + 257)
STAT_NAN_N = 262145                                 # this one carries 1 % NaN rows: the divisor is the finite count


def stat_blocks(n):
    return min((n + 255) // 256, 1024)


@functools.lru_cache(None)
def stat_cloud(n):
    p = np.random.default_rng(7).random((n, 3), dtype=np.float32)
    if n == STAT_NAN_N:
        p[50::100, 0] = np.nan
    return _ro(p)


# ---- 4. shifted -------------------------------------------------------------------------------------------------------------------
SHIFTS = (0.0,) + SC.FAR_SHIFTS                     # 0, 2^10, 2^13, 2^16; the cloud is snapped to 2^-7
SHIFT_KS = (8, 130)
SHIFT_RADIUS = 0.125                                # 16 steps of the snapped grid: d2 == r2 happens and is exact at every shift
SHIFT_TOL = 0.0625


def shifted_cloud(shift):
    return SC.shifted("uniform", shift)[0]


# ---- 5. cluster_sizes -------------------------------------------------------------------------------------------------------------
SIZE_WINDOWS = ((5, 5), (4, 6), (5, 6), (4, 5), (6, 6), (7, 7))
SIZE_TOL = 0.05
SIZE_COUNTS = {1: 6, 4: 5, 5: 5, 6: 5}              # component size: how many


@functools.lru_cache(None)
def sized_components():
    """-> (points, component id per point): chains 0.03 apart on sites 1.0 apart, the points shuffled (seed 0) so that every
    component's indices are spread over the cloud"""
    pts, comp = [], []
    sizes = [s for k in range(6) for s in (4, 5, 6, 1) if k < SIZE_COUNTS[s]]
    for c, s in enumerate(sizes):
        site = np.array([c % 5, c // 5, 0], np.float32)
        for j in range(s):
            pts.append(site + np.array([0, j * 0.03, 0], np.float32))
            comp.append(c)
    order = np.random.default_rng(0).permutation(len(pts))
    return _ro(np.array(pts, np.float32)[order]), np.array(comp)[order]


# ---- 6. lattice_shells ------------------------------------------------------------------------------------------------------------
def shell_radii():
    """the nine floats on and either side of the three shells, without 0.25 and 0.5 themselves for the radius filter's existing test"""
    return [r for base in SC.SHELL_RADII for r in SC.ulps(base)]


LATTICE_FAR_PAIR = np.array([[7000.0, 2.0, 2.0], [7000.0, 2.25, 2.0]], np.float32)     # 10^3 box diagonals along x, one spacing apart


@functools.lru_cache(None)
def lattice_cloud(clamped):
    if not clamped:
        return _ro(OC.lattice(12))
    base = OC.lattice(17)                           # 4 913 points: with the pair the smallest cube above the builder's 4 096
    return _ro(insert_rows(base, undrawn_rows(len(base) + 2, 4)[1:3], LATTICE_FAR_PAIR))


def lattice_pair_rows():
    return undrawn_rows(17 ** 3 + 2, 4)[1:3]


# ---- the table --------------------------------------------------------------------------------------------------------------------
BUILDERS = {"clamped_far": lambda outliers: clamped_far(outliers)[0], "block": block_cloud, "triples130": triples130, "stat": stat_cloud,
            "shifted": shifted_cloud, "sized": lambda: sized_components()[0], "lattice": lattice_cloud}


def case_input(c):
    return BUILDERS[c.cloud[0]](*c.cloud[1:])


def case_id(c):
    return f"{c.family}-{c.name}-{c.op}"


@functools.lru_cache(None)
def cases():
    out = []
    far, ctl = ("clamped_far", True), ("clamped_far", False)
    nfar = FAR_N + sum(len(p) for _, _, p in far_sites())
    for k in FAR_KS:
        out.append(Case("clamped_far", f"k{k}", "sor", far, (k,)))
    for k in FAR_CONTROL_KS:
        out.append(Case("clamped_far", f"control-k{k}", "sor", ctl, (k,)))
    for cloud, tag in ((far, ""), (ctl, "control-")):
        out.append(Case("clamped_far", tag + "r0.3", "radius", cloud, (FAR_RADIUS, (1, 2, 3))))
        out.append(Case("clamped_far", tag + "r2diag", "radius", cloud, (FAR_WIDE_RADIUS, None)))
        out.append(Case("clamped_far", tag + "tol_on", "cluster", cloud, (FAR_TOL, ((2, nfar), (3, nfar), (2, 2), (3, 3), (1, nfar)))))
        out.append(Case("clamped_far", tag + "tol_below", "cluster", cloud, (FAR_TOL_BELOW, ((2, nfar), (1, nfar)))))
    for n in BLOCK_NS:
        cloud = ("block", n)
        out.append(Case("block_edges", f"n{n}-k8", "sor", cloud, (8,)))
        out.append(Case("block_edges", f"n{n}-k{n + 3}", "sor", cloud, (n + 3,)))
        out.append(Case("block_edges", f"n{n}", "radius", cloud, (BLOCK_RADIUS, (block_min_neighbors(n), 1))))
        out.append(Case("block_edges", f"n{n}", "cluster", cloud, (BLOCK_TOL, ((1, n), (2, max(n, 2))))))
    out.append(Case("block_edges", "triples130", "cluster", ("triples130",), (0.05, ((1, 390), (2, 390), (3, 3), (4, 390)))))
    for n in STAT_NS:
        out.append(Case("stats_edges", f"n{n}" + ("-nan" if n == STAT_NAN_N else ""), "stats", ("stat", n), (1,)))
    for s in SHIFTS:
        cloud = ("shifted", s)
        for k in SHIFT_KS:
            out.append(Case("shifted", f"by{int(s)}-k{k}", "sor", cloud, (k,)))
        out.append(Case("shifted", f"by{int(s)}", "radius", cloud, (SHIFT_RADIUS, None)))
        out.append(Case("shifted", f"by{int(s)}", "cluster", cloud, (SHIFT_TOL, ((1, 3000), (2, 3000)))))
    out.append(Case("cluster_sizes", "windows", "cluster", ("sized",), (SIZE_TOL, SIZE_WINDOWS)))
    for clamped in (False, True):
        cloud, tag = ("lattice", clamped), ("clamped-" if clamped else "")
        n = len(lattice_cloud(clamped))
        for r in (shell_radii() if not clamped else SC.ulps(0.25)):
            if clamped or r not in (0.25, 0.5):
                out.append(Case("lattice_shells", f"{tag}r{r!r}", "radius", cloud, (r, None)))
            out.append(Case("lattice_shells", f"{tag}r{r!r}", "cluster", cloud, (r, ((1, n), (2, n)))))
    return tuple(out)


# ---- the checkers' answers, once per process ---------------------------------------------------------------------------------------
@functools.lru_cache(None)
def ref_mean(cloud, k):
    m = OC.mean_distances(BUILDERS[cloud[0]](*cloud[1:]), k)
    m.setflags(write=False)
    return m


@functools.lru_cache(None)
def ref_counts(cloud, radius):
    c = OC.radius_counts(BUILDERS[cloud[0]](*cloud[1:]), radius)
    c.setflags(write=False)
    return c


@functools.lru_cache(None)
def ref_pairs(cloud, tol):
    return K.f32_pairs(BUILDERS[cloud[0]](*cloud[1:]), tol)


def ref_clusters(cloud, tol, mn, mx):
    n = len(BUILDERS[cloud[0]](*cloud[1:]))
    return K.from_pairs(n, *ref_pairs(cloud, tol), mn, mx)


def derived_mins(counts):
    """min_neighbors at and either side of the smallest, the median and the largest neighbour count of the finite points"""
    nb = np.sort(counts[counts >= 1]) - 1
    if len(nb) == 0:
        return (1,)
    picks = {1}
    for v in (int(nb[0]), int(nb[len(nb) // 2]), int(nb[-1])):
        picks |= {v, v + 1}
    return tuple(sorted(m for m in picks if m >= 1))


def radius_mins(c):
    return c.params[1] if c.params[1] is not None else derived_mins(ref_counts(c.cloud, c.params[0]))
