"""Checker for Euclidean cluster extraction (segmentation.rs:396-455), shared by test_clusters_cpu.py and
test_gpu_clusters.py.

Adjacency: i != j and d2 <= tol * tol, with d2 = dx*dx + dy*dy + dz*dz in float32, left to right (numpy float32 arrays
round every operation and never fuse).  Components by scipy; kept when min <= size <= max; ranked by size descending,
then smallest original index ascending; members of a cluster in ascending index."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

NONE = 0xFFFFFFFF


def _d2(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return _d2_raw(a, b)


def _d2_raw(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return dx * dx + dy * dy + dz * dz


def f32_pairs(pts, tol):
    """(i, j) with i < j and the float32 relation."""
    pts = np.ascontiguousarray(pts, np.float32)
    n = len(pts)
    r2 = np.float32(tol) * np.float32(tol)
    if not (r2 <= r2) or n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    if n <= 20000:
        ii, jj = [], []
        for s in range(0, n, 256):
            e = min(n, s + 256)
            d2 = _d2(pts[s:e, None, :], pts[None, :, :])
            a, b = np.nonzero(d2 <= r2)
            a = a + s
            keep = b > a
            ii.append(a[keep]); jj.append(b[keep])
        return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)
    from scipy.spatial import cKDTree
    fin = np.nonzero(np.all(np.isfinite(pts), axis=1))[0]
    p = pts[fin].astype(np.float64)
    amax = float(np.abs(p).max()) if len(p) else 0.0
    r = float(tol) * (1.0 + 1e-5) + 4.0 * 2.0 ** -24 * amax
    pr = cKDTree(p).query_pairs(r, output_type="ndarray")
    i, j = fin[pr[:, 0]], fin[pr[:, 1]]
    keep = _d2(pts[i], pts[j]) <= r2
    i, j = i[keep], j[keep]
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    return lo.astype(np.int64), hi.astype(np.int64)


def clusters(pts, tol, min_size, max_size):
    """-> (labels uint32 (n,), members uint32 (m,), offsets uint64 (nc + 1,)) -- the library's output contract."""
    return from_pairs(len(pts), *f32_pairs(pts, tol), min_size, max_size)


def from_pairs(n, i, j, min_size, max_size):
    """the output contract from the adjacent pairs (i, j)"""
    g = coo_matrix((np.ones(len(i), np.int8), (i, j)), shape=(n, n))
    ncomp, comp = connected_components(g, directed=False)
    size = np.bincount(comp, minlength=ncomp)
    _, first = np.unique(comp, return_index=True)          # smallest index of every component (components are 0..ncomp-1)
    keep = np.nonzero((size >= min_size) & (size <= max_size))[0]
    order = keep[np.lexsort((first[keep], -size[keep]))]
    rank = np.full(ncomp, NONE, np.uint64)
    rank[order] = np.arange(len(order), dtype=np.uint64)
    labels = rank[comp].astype(np.uint32)
    key = np.where(labels == NONE, len(order), labels.astype(np.int64))
    members = np.argsort(key, kind="stable")[: int(size[order].sum())].astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(size[order])]).astype(np.uint64)
    return labels, members, offsets


def cluster_lists(labels, members, offsets):
    return [members[int(offsets[k]):int(offsets[k + 1])].astype(np.int64) for k in range(len(offsets) - 1)]


def lattice(shape, spacing):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij"), -1).reshape(-1, 3)
    return (g * np.float32(spacing)).astype(np.float32)


def sphere_cloud(center, radius, n, seed):
    """A blob of n points inside a sphere (the reference tests' make_sphere_cloud: random points in a ball)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    r = radius * rng.random(n) ** (1.0 / 3.0)
    return (np.asarray(center, np.float64) + v * r[:, None]).astype(np.float32)
