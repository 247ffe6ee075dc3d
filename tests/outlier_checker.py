"""Checker for the outlier removal filters (filtering.rs:167-395), shared by test_outliers_cpu.py and test_gpu_outliers.py.

Distances are d2 = dx*dx + dy*dy + dz*dz in float32, left to right (numpy rounds every operation and never fuses).  The k + 1
nearest of a point come from a cKDTree query in float64 that is WIDER than k + 1 and are re-ranked by the f32 d2; a row is accepted
when the farthest f64 candidate, shaved by 1e-5, is no nearer than the (k + 1)-th f32 value -- then no record outside the candidates
can change the multiset of the k + 1 smallest -- and is queried again with twice the width otherwise (a plateau of exact ties).

mean_distances: per point the sequential f32 sum of sqrt(d2) over the ascending list with the d2 == 0 entries dropped (the point
itself and its exact duplicates, filtering.rs:287), divided by their count; 0 when none is left (:291-293).  A point with a
non-finite coordinate is inert (the backend's documented deviation): never a neighbour, mean NaN, outside the statistics.

thresholds: t_ref follows the reference's sequential f32 sums (:300-309); t_f64 is the exactly summed mean and population variance
(math.fsum) with one rounding to f32 at the end, which is what the backend approximates with its fixed-order f64 sums.

radius_keep: the f32 relation d2 <= r * r counted with the point itself, minus one, >= min_neighbors (:197-208)."""
import math

import numpy as np


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _finite(pos):
    return np.all(np.isfinite(pos), axis=1)


def d2_f32(a, b):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return dx * dx + dy * dy + dz * dz


def nearest_d2(pos, k1, widths=None):
    """(nfin, min(k1, nfin)) float32: per finite point the ascending f32 d2 of its k1 nearest finite points (itself included).
    widths: a list that receives (candidate width, rows asked at that width) per round of the widening"""
    from scipy.spatial import cKDTree
    pf = _f32(pos)
    pf = pf[_finite(pf)]
    nfin = len(pf)
    K1 = min(int(k1), nfin)
    out = np.zeros((nfin, K1), np.float32)
    if nfin == 0:
        return out
    tree = cKDTree(pf.astype(np.float64))
    rows = np.arange(nfin)
    width = min(nfin, K1 + 16)
    while len(rows):
        if widths is not None:
            widths.append((width, len(rows)))
        d64, idx = tree.query(pf[rows].astype(np.float64), k=width, workers=8)         # (threads: the same answer, sooner)
        d64, idx = d64.reshape(len(rows), -1), idx.reshape(len(rows), -1)
        d2 = np.sort(d2_f32(pf[rows][:, None, :], pf[idx]), axis=1)
        out[rows] = d2[:, :K1]
        if width >= nfin:
            break
        unsafe = d64[:, -1] ** 2 <= d2[:, K1 - 1].astype(np.float64) * (1.0 + 1e-5)       # a plateau may run past the candidates
        unsafe &= d2[:, K1 - 1] > 0                                                       # (an all-zero list cannot improve)
        rows = rows[unsafe]
        width = min(nfin, 2 * width)
    return out


def mean_distances(pos, k):
    """(n,) float32 mean distance to the k nearest, NaN for points with a non-finite coordinate"""
    pos = _f32(pos)
    fin = _finite(pos)
    out = np.full(len(pos), np.nan, np.float32)
    out[fin] = means_of_lists(nearest_d2(pos, int(k) + 1))
    return out


def means_of_lists(d2):
    """(rows,) float32: the mean of every ascending d2 list (a row of nearest_d2)"""
    dist = np.sqrt(d2)                          # float32, correctly rounded
    use = d2 > 0
    s = np.zeros(len(d2), np.float32)
    for j in range(d2.shape[1]):                # sequential, in list order; + 0.0 leaves an f32 sum as it is
        s = s + np.where(use[:, j], dist[:, j], np.float32(0))
    cnt = use.sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(cnt > 0, s / cnt.astype(np.float32), np.float32(0)).astype(np.float32)


def thresholds(mean, mult):
    """(t_ref, t_f64) as float32 scalars, over the non-NaN means"""
    mf = np.asarray(mean, np.float32)
    mf = mf[~np.isnan(mf)]
    n = len(mf)
    mult = np.float32(mult)
    if n == 0:
        return np.float32(np.nan), np.float32(np.nan)
    with np.errstate(all="ignore"):
        gm = np.cumsum(mf, dtype=np.float32)[-1] / np.float32(n)             # sequential f32 (:300)
        dev = mf - gm
        var = np.cumsum(dev * dev, dtype=np.float32)[-1] / np.float32(n)     # :302-306
        t_ref = np.float32(gm + mult * np.sqrt(var))                         # :308-309
        m64 = math.fsum(float(x) for x in mf) / n
        v64 = math.fsum((float(x) - m64) ** 2 for x in mf) / n
        t_f64 = np.float32(m64 + float(mult) * math.sqrt(v64))
    return t_ref, t_f64


def sor_keep(mean, threshold):
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.asarray(mean, np.float32) <= np.float32(threshold))[0]


BRUTE_MAX = 8192        # up to here radius_counts compares every pair (a ball that holds the cloud makes the tree's lists n^2 long)


def radius_counts(pos, radius, tree_road=False):
    """(n,) int64: per point the finite points with d2 <= r * r in f32, itself included (0 for inert points; every finite point
    when r * r is infinite).  The same relation on every pair of a small cloud, on the candidates of a kd-tree ball (in f64, widened)
    of a larger one or when tree_road asks for it: the same counts (tests/test_filter_edges_cpu.py)"""
    from scipy.spatial import cKDTree
    pos = _f32(pos)
    fin = _finite(pos)
    fidx = np.nonzero(fin)[0]
    with np.errstate(over="ignore", under="ignore"):
        r2 = np.float32(radius) * np.float32(radius)
    counts = np.zeros(len(pos), np.int64)
    if np.isnan(r2) or len(fidx) == 0:
        return counts
    if np.isinf(r2):
        counts[fidx] = len(fidx)
        return counts
    pf = pos[fidx]
    if len(pf) <= BRUTE_MAX and not tree_road:
        for s in range(0, len(pf), 256):
            counts[fidx[s:s + 256]] = (d2_f32(pf[s:s + 256, None, :], pf[None, :, :]) <= r2).sum(axis=1)
        return counts
    tree = cKDTree(pf.astype(np.float64))
    lists = tree.query_ball_point(pf.astype(np.float64), math.sqrt(float(r2)) * (1.0 + 1e-5) + 1e-20)
    lens = np.fromiter((len(l) for l in lists), np.int64, len(lists))
    src = np.repeat(np.arange(len(pf)), lens)
    dst = np.fromiter((j for l in lists for j in l), np.int64, int(lens.sum()))
    ok = d2_f32(pf[src], pf[dst]) <= r2
    counts[fidx] = np.bincount(src[ok], minlength=len(pf))
    return counts


def radius_keep(pos, radius, min_neighbors):
    return keep_of_counts(radius_counts(pos, radius), min_neighbors)


def keep_of_counts(c, min_neighbors):
    return np.array([i for i in range(len(c)) if c[i] >= 1 and int(c[i]) - 1 >= int(min_neighbors)], np.int64)


# ---- inputs shared by the CPU precondition and the GPU test ------------------------------------------
SOR_CASES = [(2000, 4), (20000, 8), (20000, 20)]        # (n, k)
SOR_MULTIPLIERS = [1.0, 2.0]


def sor_cloud(n, seed=0):
    """uniform [0, 1)^3 in f32 with 1 % of the points displaced by up to +-2"""
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3), dtype=np.float32)
    out = rng.choice(n, n // 100, replace=False)
    p[out] += rng.uniform(-2.0, 2.0, (len(out), 3)).astype(np.float32)
    return p


def lattice(side, scale=0.25):
    g = np.arange(side, dtype=np.float32) * np.float32(scale)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
