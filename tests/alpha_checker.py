"""A numpy restatement of the contract of include/threecrate_hip_alpha.h, written from alpha_shape.rs (generate_triangles_quality,
is_triangle_geometrically_valid, filter_simplices): every operation in f32 with one rounding, in the header's order.  It takes the
neighbour loop as the reference has it (every j against every i) and is vectorised per point.  Test infrastructure: the device is
compared with it bit for bit and in order (tests/test_gpu_alpha.py); tests/test_alpha_cpu.py pins it by hand-computable cases."""
import numpy as np

F = np.float32
BOUNDARY, FULL = 0, 1
REFERENCE_CAP = 50000


class AlphaError(Exception):
    def __init__(self, kind, message):
        super().__init__(message)
        self.kind, self.message = kind, message


def norm_sq(v):
    """|v|^2 = (vx*vx + vy*vy) + vz*vz, rows of an (m, 3) f32 array"""
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def neighbours(points, i, alpha):
    """(1): every j != i with |p_i - p_j| <= alpha, ascending"""
    with np.errstate(over="ignore", invalid="ignore"):
        near = np.sqrt(norm_sq(points[i] - points)) <= F(alpha)
    near[i] = False
    return np.flatnonzero(near)


def triple_terms(pi, pj, pk):
    """(3) for rows of triples: candidate mask, R2, area"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        a2, b2, c2 = norm_sq(pj - pi), norm_sq(pk - pj), norm_sq(pi - pk)
        u, v = pj - pi, pk - pi
        x = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        X = norm_sq(x)
        area_sq = X * F(0.25)
        R2 = ((a2 * b2) * c2) / (F(16.0) * area_sq)
        area = np.sqrt(X) * F(0.5)
        per = (np.sqrt(a2) + np.sqrt(b2)) + np.sqrt(c2)
        quality = (F(4.0) * area) / (per * per)
        eps = F(1e-20)
        guards = (a2 >= eps) & (b2 >= eps) & (c2 >= eps) & (area_sq >= eps) & ~(R2 == F(np.inf))
    return guards, R2, area, per, quality


def candidates(points, alpha, min_triangle_area=1e-8, max_triangles=REFERENCE_CAP):
    """(2), (3), (4): the remaining candidates as (T, 3) indices in order, their R2 and area, and whether the cap cut any off"""
    points = np.ascontiguousarray(points, F)
    n = len(points)
    tri, r2s, areas, total, capped = [], [], [], 0, False
    for i in range(n):
        if max_triangles and total >= max_triangles:
            # the reference breaks here; whether anything was cut off needs the rest of the enumeration
            capped = capped or _has_candidate_from(points, i, alpha, min_triangle_area)
            break
        t, R2, area = candidates_of_point(points, i, alpha, min_triangle_area)
        sel = np.arange(len(t))
        if max_triangles and total + len(sel) > max_triangles:
            sel, capped = sel[:max_triangles - total], True
        total += len(sel)
        tri.append(t[sel]); r2s.append(R2[sel]); areas.append(area[sel])
    if not tri:
        return np.zeros((0, 3), np.int64), np.zeros(0, F), np.zeros(0, F), capped
    return np.concatenate(tri), np.concatenate(r2s), np.concatenate(areas), capped


def _has_candidate_from(points, start, alpha, min_triangle_area):
    for i in range(start, len(points)):
        if len(candidates_of_point(points, i, alpha, min_triangle_area)[0]):
            return True
    return False


def candidates_of_point(points, i, alpha, min_triangle_area):
    """(2) and (3) for one i: its candidates (i, j, k) in lexicographic order, their R2 and area"""
    nb = neighbours(points, i, alpha)
    nb = nb[nb > i]
    if len(nb) < 2:
        return np.zeros((0, 3), np.int64), np.zeros(0, F), np.zeros(0, F)
    a, b = np.triu_indices(len(nb), 1)
    j, k = nb[a], nb[b]
    guards, R2, area, per, quality = triple_terms(np.broadcast_to(points[i], (len(j), 3)), points[j], points[k])
    with np.errstate(invalid="ignore"):
        cand = guards & (area >= F(min_triangle_area)) & (per >= F(1e-10)) & (quality > F(0.01))
    sel = np.flatnonzero(cand)
    return np.stack([np.full(len(sel), i, np.int64), j[sel], k[sel]], axis=1), R2[sel], area[sel]


def boundary_flags(tri):
    """(5): a candidate is a boundary candidate when one of its edges lies on no other candidate"""
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [0, 2]]])
    keys = (e.min(axis=1).astype(np.uint64) << np.uint64(32)) | e.max(axis=1).astype(np.uint64)
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    single = (counts[inverse] == 1).reshape(3, len(tri))
    return single.any(axis=0)


def alpha_shape(points, alpha, mode=BOUNDARY, min_triangle_area=1e-8, max_triangles=REFERENCE_CAP):
    """faces (m, 3) uint32 in order and the stats; AlphaError("InvalidData" | "Algorithm", message) as the header says"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    if n == 0:
        raise AlphaError("InvalidData", "Point cloud is empty")
    if n < 3:
        raise AlphaError("InvalidData", "Need at least 3 points for triangulation")
    if mode not in (BOUNDARY, FULL):
        raise AlphaError("InvalidData", "mode")
    if not (F(alpha) > 0 and np.isfinite(F(alpha))):
        raise AlphaError("InvalidData", "alpha")
    if not F(min_triangle_area) >= 0:
        raise AlphaError("InvalidData", "min_triangle_area")
    if not np.isfinite(points).all():
        raise AlphaError("InvalidData", "a coordinate is not finite")
    tri, R2, area, capped = candidates(points, alpha, min_triangle_area, max_triangles)
    if len(tri) == 0:
        raise AlphaError("Algorithm", "No candidate triangles generated")
    bnd = boundary_flags(tri)
    with np.errstate(over="ignore"):
        keep = (R2 <= F(alpha) * F(alpha)) & (area >= F(min_triangle_area))
    if mode == BOUNDARY:
        keep &= bnd
    if not keep.any():
        raise AlphaError("Algorithm", "No triangles survived alpha filtering")
    return {"faces": tri[keep].astype(np.uint32), "candidates": len(tri), "boundary_candidates": int(bnd.sum()), "n_faces": int(keep.sum()),
            "capped": int(capped)}


def estimate_optimal_alpha(points, k):
    """estimate_optimal_alpha (alpha_shape.rs), brute force: f32 distances, the k-th smallest to the other points, the median by [len/2]"""
    points = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = len(points)
    if n == 0:
        raise AlphaError("InvalidData", "Point cloud is empty")
    sample = min(max(n // 10, 50), 500)
    step = max(max(n, 1) // max(sample, 1), 1)
    dist = []
    for i in range(0, n, step):
        d = np.sort(np.delete(np.sqrt(norm_sq(points[i] - points)), i))
        if len(d) >= k:
            dist.append(d[k - 1])
    if not dist:
        return F(1.0)
    dist.sort()
    return F(dist[len(dist) // 2] * F(1.8))
