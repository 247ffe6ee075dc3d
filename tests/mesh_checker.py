"""The contract of include/threecrate_hip_mesh.h in numpy f32, one operation per line: mesh_smoothing.rs restated with the summation
order fixed to ascending neighbour index.  The device must equal it bit for bit.  No Rust toolchain runs the reference here; its unit
tests are literals in tests/test_mesh_cpu.py.
RULES names the rules a mutant changes (tests/test_mesh_cpu.py holds every mutant to a named case of tests/mesh_cases.py that tells
it apart); smooth(..., rules={name}) computes the mutant."""
import numpy as np

F = np.float32
LAPLACIAN, TAUBIN, HC = 0, 1, 2
DEFAULTS = {"iterations": 10, "lambda_": 0.5, "mu": -0.53, "alpha": 0.0, "beta": 0.5}
RULES = {
    "descending_fold": "the ring is summed in descending neighbour index",
    "pairwise_sum": "the ring is summed pairwise (np.add.reduce) instead of by a sequential fold",
    "fused_step": "v + d * t with one rounding (computed in f64, rounded once)",
    "reciprocal_division": "sum * (1 / deg) instead of sum / deg",
    "no_self_neighbour": "a face that repeats an index does not make the vertex its own neighbour",
    "duplicates_in_degree": "deg counts every directed pair, not the distinct ones",
    "f64_one_minus_alpha": "q * (1 - alpha) with 1 - alpha kept in f64",
    "mu_first": "Taubin takes the mu step before the lambda step",
    "avg_over_qbar": "HC averages qbar over the ring instead of b",
    "isolated_to_origin": "a vertex with no neighbour gets the centroid (0, 0, 0) instead of keeping its position",
}


def adjacency(n_vertices, faces, rules=()):
    """-> offsets (n + 1,) uint32, neighbors (offsets[-1],) uint32: the distinct j of every i, ascending"""
    f = np.asarray(faces, np.uint64).reshape(-1, 3)
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    frm = np.concatenate([a, a, b, b, c, c])
    to = np.concatenate([b, c, a, c, a, b])
    if "no_self_neighbour" in rules:
        keep = frm != to
        frm, to = frm[keep], to[keep]
    keys = np.unique((frm << np.uint64(32)) | to)
    frm, to = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    offsets = np.searchsorted(frm, np.arange(n_vertices + 1)).astype(np.uint32)
    return offsets, to


def _pair_counts(n_vertices, faces):
    """directed pairs per vertex, duplicates included (the duplicates_in_degree mutant)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return 2 * np.bincount(f.reshape(-1), minlength=n_vertices)


def ring_sums(x, offsets, neighbors, rules=()):
    """the fold of x[j] over every vertex's ring, ascending, from +0, per component.  Vertices are grouped by degree, so a hub of
    thousands of neighbours costs one pass over its own ring and nothing for the rest.  np.add.accumulate is a sequential fold."""
    n = len(offsets) - 1
    deg = np.diff(offsets.astype(np.int64))
    out = np.zeros((n, 3), F)
    for d in np.unique(deg):
        if d == 0:
            continue
        who = np.nonzero(deg == d)[0]
        idx = neighbors[offsets[who].astype(np.int64)[:, None] + np.arange(d)[None, :]]
        ring = x[idx]                                                       # (vertices, d, 3)
        if "descending_fold" in rules:
            ring = ring[:, ::-1]
        if "pairwise_sum" in rules:
            out[who] = np.add.reduce(np.ascontiguousarray(ring.transpose(0, 2, 1)), axis=2, dtype=F)
            continue
        zero = np.zeros((len(who), 1, 3), F)
        out[who] = np.add.accumulate(np.concatenate([zero, ring], axis=1), axis=1, dtype=F)[:, -1]
    return out


def _divide(s, fdeg, rules):
    if "reciprocal_division" in rules:
        r = F(1.0) / fdeg
        return s * r
    return s / fdeg


def centroid(x, offsets, neighbors, deg, rules=()):
    """-> (centroid where deg > 0, has) ; deg is what the division uses"""
    s = ring_sums(x, offsets, neighbors, rules)
    has = np.diff(offsets.astype(np.int64)) > 0
    fdeg = np.where(has, deg, 1).astype(F)[:, None]
    c = _divide(s, fdeg, rules)
    return c, has


def laplacian_step(v, offsets, neighbors, deg, t, rules=()):
    c, has = centroid(v, offsets, neighbors, deg, rules)
    if "isolated_to_origin" in rules:
        c, has = np.where(has[:, None], c, F(0.0)), np.ones_like(has)
    if "fused_step" in rules:
        out = (v.astype(np.float64) + (c - v).astype(np.float64) * np.float64(F(t))).astype(F)
    else:
        d = c - v
        m = d * F(t)
        out = v + m
    return np.where(has[:, None], out, v)


def hc_iteration(p, q, offsets, neighbors, deg, alpha, beta, rules=()):
    c, has = centroid(q, offsets, neighbors, deg, rules)
    if "isolated_to_origin" in rules:
        c, has = np.where(has[:, None], c, F(0.0)), np.ones_like(has)
    qbar = np.where(has[:, None], c, q)
    w = F(1.0) - F(alpha)
    pa = p * F(alpha)
    qw = (q.astype(np.float64) * (1.0 - np.float64(F(alpha)))).astype(F) if "f64_one_minus_alpha" in rules else q * w
    blend = pa + qw
    b = qbar - blend
    s = ring_sums(qbar if "avg_over_qbar" in rules else b, offsets, neighbors, rules)
    real = np.diff(offsets.astype(np.int64)) > 0
    fdeg = np.where(real, deg, 1).astype(F)[:, None]
    avg = np.where(real[:, None], _divide(s, fdeg, rules), F(0.0))
    u = F(1.0) - F(beta)
    bb = b * F(beta)
    au = avg * u
    corr = bb + au
    return qbar - corr


def smooth(vertices, faces, method, iterations=10, lambda_=0.5, mu=-0.53, alpha=0.0, beta=0.5, rules=()):
    """-> the smoothed vertices (n, 3) float32.  The parameters are taken as valid (the header's checks are the library's)."""
    rules = set(rules)
    assert rules <= set(RULES)
    v = np.array(vertices, F).reshape(-1, 3)
    n = len(v)
    faces = np.asarray(faces).reshape(-1, 3)
    assert n > 0 and len(faces) > 0 and faces.max() < n
    offsets, neighbors = adjacency(n, faces, rules)
    deg = _pair_counts(n, faces) if "duplicates_in_degree" in rules else np.diff(offsets.astype(np.int64))
    with np.errstate(all="ignore"):
        if method == HC:
            p, q = v, v.copy()
            for _ in range(iterations):
                q = hc_iteration(p, q, offsets, neighbors, deg, alpha, beta, rules)
            return q
        steps = [lambda_] if method == LAPLACIAN else ([mu, lambda_] if "mu_first" in rules else [lambda_, mu])
        for _ in range(iterations):
            for t in steps:
                v = laplacian_step(v, offsets, neighbors, deg, t, rules)
        return v
