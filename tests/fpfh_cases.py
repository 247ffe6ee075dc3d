"""The FPFH edge cases: one table, read by tests/test_fpfh_edges_cpu.py (which proves on the checker alone what every case is there
for) and by tests/test_gpu_fpfh_edges.py (which runs them on the device).  The checker is tests/fpfh_checker.py.

A case is (family, name, cloud, radius, k, rows): `cloud` names a builder of this module and its arguments, -> (positions,
normals), float32, read-only, built once; `rows` says which rows are compared (ROWS below).  reference(c) is the checker's answer
for those rows, computed once per process.

Clouds are drawn as rng = default_rng(seed), positions rng.random((n, 3)), normals unit(rng.normal(size=(n, 3))), as in
test_gpu_fpfh.py.  The seeds are the first ones at which the checker calls the compared rows strict (test_fpfh_edges_cpu.py holds
that); nothing else about them is chosen."""
import collections
import functools

import numpy as np

from tests import fpfh_checker as F
from tests import search_checker as S

Case = collections.namedtuple("Case", "family name cloud radius k rows")
NAN = float("nan")


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _ro(*arrays):
    out = tuple(np.ascontiguousarray(a, np.float32) for a in arrays)
    for a in out:
        a.setflags(write=False)
    return out


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 3)).astype(np.float32)
    return pos, unit(rng.normal(size=(n, 3)))


@functools.lru_cache(maxsize=None)
def uniform(n, seed):
    return _ro(*_uniform(n, seed))


# ---- shells: the 12^3 lattice of the search tests, radii on and next to its shells ----------------------------------------------
LATTICE_SEED = 1
SHELL_BASES = S.SHELL_RADII[:2]                     # 0.25 (6 points at d2 = 0.0625) and f32(0.25 sqrt 2) (12 more at 0.125)


@functools.lru_cache(maxsize=None)
def lattice():
    pos = S._lattice_points()
    return _ro(pos, unit(np.random.default_rng(LATTICE_SEED).normal(size=(len(pos), 3))))


def lattice_interior():
    """the 512 rows whose lattice coordinates lie in [2, 9]: their neighbours and THEIR neighbours (two shells each) are interior"""
    c = np.stack(np.unravel_index(np.arange(1728), (12, 12, 12)), 1)
    return np.nonzero(((c >= 2) & (c <= 9)).all(axis=1))[0]


def shell_counts():
    """others within (one ulp below, the radius, one ulp above) of an interior point, per base: S.SHELL_COUNTS without the point"""
    return tuple(tuple(c - 1 for c in row) for row in S.SHELL_COUNTS[:2])


def shell_candidates():
    """(base, which, radius, k): per radius k = the count inside it and that count +- 1, k = 1, and the counts of the base's other
    two radii (the fallback then has to find the shell the ball lost)"""
    out = []
    for b, (base, counts) in enumerate(zip(SHELL_BASES, shell_counts())):
        for w, (r, cnt) in enumerate(zip(S.ulps(base), counts)):
            for k in sorted({cnt - 1, cnt, cnt + 1, 1, *counts} - {-1}):
                out.append((b, w, r, k))
    return out


# the candidates the checker calls tie-free on every interior row (test_shell_table_is_the_tie_free_part_of_the_candidates); the
# others cut a plateau: every row ties
SHELL_KEPT = {(0, 0): (0, 6), (0, 1): (0, 1, 5, 6), (0, 2): (0, 1, 5, 6),
              (1, 0): (1, 5, 6, 18), (1, 1): (1, 5, 6, 18), (1, 2): (1, 6, 17, 18)}


# ---- far_pairs / clamped ------------------------------------------------------------------------------------------------------------
FAR_SEED, FAR_R, FAR_KS = 1, 0.08, (1, 2, 8)
FAR_N, FAR_OUT = 6000, 30
# rows of the outlier block: a pair 0.03 apart, a pair 0.5 r apart, a triple inside one radius, a point 10^6 box diagonals out along
# x and its partner 0.5 r from it along y (along x a float there is 0.125 wide)
FAR_PAIR, FAR_HALF, FAR_TRIPLE, FAR_DISTANT = (0, 1), (2, 3), (4, 5, 6), (7, 8)


def _far_cloud(seed, outliers):
    rng = np.random.default_rng(seed)
    pos = rng.random((FAR_N, 3)).astype(np.float32)
    out = rng.normal(0.0, 100.0, (FAR_OUT, 3)).astype(np.float32)
    nrm = unit(rng.normal(size=(FAR_N + FAR_OUT, 3)))
    h = np.float32(0.5 * FAR_R)
    out[1] = out[0] + np.array([0.03, 0, 0], np.float32)
    out[3] = out[2] + np.array([0, h, 0], np.float32)
    out[5] = out[4] + np.array([0.03, 0, 0], np.float32)
    out[6] = out[4] + np.array([0, 0.03, 0.02], np.float32)
    out[7] = np.array([np.sqrt(3.0) * 1.0e6, 0.5, 0.5], np.float32)
    out[8] = out[7] + np.array([0, h, 0], np.float32)
    if not outliers:
        return pos, nrm[:FAR_N]
    return np.concatenate([pos, out]), nrm


@functools.lru_cache(maxsize=None)
def far_pairs(outliers=True):
    return _ro(*_far_cloud(FAR_SEED, outliers))


@functools.lru_cache(maxsize=None)
def shifted(shift):
    """the far_pairs interior cloud snapped to 2^-7 (exact at 2^13 too: one ulp there is 2^-10) and moved along every axis"""
    pos, nrm = far_pairs(False)
    step = np.float32(2.0 ** -7)
    return _ro(np.round(pos / step) * step + np.float32(shift), nrm)


SHIFTS = (0.0, 2.0 ** 10, 2.0 ** 13)

# ---- unbounded ----------------------------------------------------------------------------------------------------------------------
UNBOUNDED_SEED = {64: 100, 300: 100}
UNBOUNDED_RADII = (1e20, 1.8e19, 1e3)         # r^2 infinite; finite and above 3.0e38; a finite ball that holds everything

# ---- duplicates ---------------------------------------------------------------------------------------------------------------------
DUP_SEED, DUP_R = 1, 0.15


@functools.lru_cache(maxsize=None)
def copies(sites, each, seed):
    """`sites` uniform sites stored `each` times (every copy with a normal of its own), shuffled"""
    rng = np.random.default_rng(seed)
    at = rng.random((sites, 3)).astype(np.float32)
    pos = np.repeat(at, each, axis=0)[rng.permutation(sites * each)]
    return _ro(pos, unit(rng.normal(size=(len(pos), 3))))


@functools.lru_cache(maxsize=None)
def identical():
    rng = np.random.default_rng(DUP_SEED)
    return _ro(np.tile(np.array([[0.3, -1.25, 2.0]], np.float32), (500, 1)), unit(rng.normal(size=(500, 3))))


@functools.lru_cache(maxsize=None)
def two_sites():
    """two sites 0.01 apart, 300 copies each, interleaved; the copies of a site share its normal, so the checker's rows of a site are
    equal bit for bit"""
    rng = np.random.default_rng(DUP_SEED)
    at = np.array([[0.5, 0.5, 0.5], [0.5, 0.51, 0.5]], np.float32)
    n2 = unit(rng.normal(size=(2, 3)))
    site = np.arange(600) % 2
    return _ro(at[site], n2[site])


# ---- k_edges ------------------------------------------------------------------------------------------------------------------------
K_EDGE_SEED = 0
K_EDGES = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 255, 256)     # k + 1 either side of every list size of launch_knn
K_MAX = 2047
K_MAX_SEED = {150: 0, 2100: 0}

# ---- blocks -------------------------------------------------------------------------------------------------------------------------
BLOCK_NS = (127, 128, 129, 255, 256, 257, 513)
BLOCK_SEED, BLOCK_R, BLOCK_K = 1, 0.1, 8


@functools.lru_cache(maxsize=None)
def blocks(n):
    """first half in a cube of edge 0.1 (every ball of radius 0.1 holds a good part of it), second half uniform in the unit cube
    (about one point per ball); a NaN / +inf / -inf coordinate at indices 0, n // 2, n - 1"""
    pos, nrm = _uniform(n, BLOCK_SEED + n)
    pos[:n // 2] *= np.float32(0.1)
    pos[0, 0], pos[n // 2, 1], pos[n - 1, 2] = np.nan, np.inf, -np.inf
    return _ro(pos, nrm)


# ---- chunked ------------------------------------------------------------------------------------------------------------------------
CHUNK_K, CHUNK_R, CHUNK_SEED = 31, 0.006, 0
CHUNK_LISTS = (1 << 25) // (CHUNK_K + 1)                          # fallback lists held at once: 2^20
CHUNK_SPARSE, CHUNK_DENSE = 1500000, 400000
CHUNK_LO, CHUNK_EDGE = np.array([0.4, 0.4, 0.79], np.float32), np.float32(0.2)     # the dense cube: the top of the z range, where the
CHUNK_ALL_N = (1 << 20) + 1                                                      # cell order (z-major) puts the LAST fallback points


@functools.lru_cache(maxsize=None)
def mixed():
    """CHUNK_SPARSE points uniform in the unit cube (about one other point in a ball of CHUNK_R: they fall back), then CHUNK_DENSE in
    the dense cube (about 45 per ball: most do not)"""
    rng = np.random.default_rng(CHUNK_SEED)
    sparse = rng.random((CHUNK_SPARSE, 3)).astype(np.float32)
    dense = CHUNK_LO + CHUNK_EDGE * rng.random((CHUNK_DENSE, 3)).astype(np.float32)
    pos = np.concatenate([sparse, dense])
    return _ro(pos, unit(rng.normal(size=(len(pos), 3)).astype(np.float32)))


def mixed_rows():
    """300 sparse rows, 300 dense rows, 100 dense rows within CHUNK_R of the cube's top face"""
    pos, _ = mixed()
    rng = np.random.default_rng(CHUNK_SEED + 1)
    top = CHUNK_SPARSE + np.nonzero(pos[CHUNK_SPARSE:, 2] >= CHUNK_LO[2] + CHUNK_EDGE - np.float32(CHUNK_R))[0]
    return np.concatenate([rng.choice(CHUNK_SPARSE, 300, replace=False), CHUNK_SPARSE + rng.choice(CHUNK_DENSE, 300, replace=False),
                           rng.choice(top, 100, replace=False)])


# ---- the table ----------------------------------------------------------------------------------------------------------------------
# rows: None = every row; otherwise a key of ROWS
ROWS = {
    "interior": lambda c: lattice_interior(),
    # the distant pair falls back at k >= 2, and 1.7e6 away every other point is one of a few float32 distances: its list is decided
    # by the tie order.  It is compared at k = 1, where the ball walk serves it
    "not_distant": lambda c: np.delete(np.arange(FAR_N + FAR_OUT), [FAR_N + i for i in FAR_DISTANT]),
    # an isolated site has 11 others in its ball and takes the 12th from the twelve equal copies of the nearest other site: a true
    # tie, with other normals behind every choice.  Compared: the rows the checker bounds by 0.1 or less
    "bounded": lambda c: np.nonzero(reference(c._replace(rows=None))["bound"] <= 0.1)[0],
    # snapped to 2^-7 a tenth of the rows tie at the cut; compared: the rows the checker calls strict where the cloud was
    "strict_unmoved": lambda c: np.nonzero(reference(c._replace(cloud=("shifted", (0.0,)), rows=None))["strict"])[0],
    "first3": lambda c: np.arange(3),
    "mixed": lambda c: mixed_rows(),
    "sample500": lambda c: np.random.default_rng(CHUNK_SEED + 2).choice(CHUNK_ALL_N, 500, replace=False),
}


def cases():
    out = []
    for (b, w), ks in sorted(SHELL_KEPT.items()):
        r = S.ulps(SHELL_BASES[b])[w]
        out += [Case("shells", f"b{b}{'-=+'[w]}", ("lattice", ()), r, k, "interior") for k in ks]
    out += [Case("far_pairs", "clamped", ("far_pairs", (True,)), FAR_R, k, None if k == 1 else "not_distant") for k in FAR_KS]
    out += [Case("far_pairs", "exact", ("far_pairs", (False,)), FAR_R, k, None) for k in FAR_KS]
    out += [Case("unbounded", f"n{n}", ("uniform", (n, UNBOUNDED_SEED[n])), r, k, None)
            for n in (64, 300) for r in UNBOUNDED_RADII for k in (5, n + 3)]
    out += [Case("duplicates", "x12", ("copies", (200, 12, DUP_SEED)), DUP_R, k, "bounded" if k == 12 else None) for k in (8, 11, 12)]
    # every point falls back and takes its 11 copies and the 12 of the nearest other site: k + 1 = 24 ends on a plateau's edge
    out += [Case("duplicates", "x12", ("copies", (200, 12, DUP_SEED)), NAN, 23, None)]
    out += [Case("duplicates", "identical", ("identical", ()), DUP_R, 8, None)]
    out += [Case("duplicates", "two_sites", ("two_sites", ()), r, 8, None) for r in (0.02, 0.005)]
    out += [Case("k_edges", "n600", ("uniform", (600, K_EDGE_SEED)), NAN, k, None) for k in K_EDGES]
    out += [Case("k_edges", "n150", ("uniform", (150, K_MAX_SEED[150])), NAN, K_MAX, None)]
    out += [Case("k_max", "n2100", ("uniform", (2100, K_MAX_SEED[2100])), NAN, K_MAX, "first3")]
    out += [Case("blocks", f"n{n}", ("blocks", (n,)), BLOCK_R, BLOCK_K, None) for n in BLOCK_NS]
    out += [Case("shifted", f"by{int(s)}", ("shifted", (s,)), FAR_R, 8, "strict_unmoved") for s in SHIFTS]
    return out


def all_zero_cases():
    """every point has more than k exact duplicates and every point falls back: whichever k of them the search names, every pair is a
    skipped one, so every row is zero.  The checker calls the lists tied; the rows are asserted exactly instead"""
    return [Case("duplicates", "identical", ("identical", ()), NAN, 8, None), Case("duplicates", "two_sites", ("two_sites", ()), NAN, 8, None)]


def chunked_cases():
    return [Case("chunked", "mixed", ("mixed", ()), CHUNK_R, CHUNK_K, "mixed"),
            Case("chunked", "all_fallback", ("uniform", (CHUNK_ALL_N, CHUNK_SEED)), NAN, CHUNK_K, "sample500")]


def case_id(c):
    return "-".join([c.family, c.name, f"r{c.radius!r}", f"k{c.k}"])


def case_input(c):
    """(positions, normals, rows or None)"""
    pos, nrm = globals()[c.cloud[0]](*c.cloud[1])
    return pos, nrm, (None if c.rows is None else ROWS[c.rows](c))


@functools.lru_cache(maxsize=None)
def reference(c):
    """the checker's answer for the compared rows of a case; never written to"""
    pos, nrm, rows = case_input(c)
    ref = F.fpfh(pos, nrm, c.radius, c.k, rows)
    for v in ref.values():
        v.setflags(write=False)
    return ref
