"""The contract of include/threecrate_hip_simplify.h in numpy (test infrastructure): f64 and f32 arithmetic as pinned, one rounding per
operation (numpy rounds every array operation once), math.pow for the cell size, and cosf called through ctypes on libm so that the
checker and the library use the same function.  `simplify` is the checker; `literal` restates the uniform road of
threecrate-simplification/src/clustering.rs with Python dicts and sets, cluster order as the HashMap would give it in insertion order;
`literal_in_contract_order` sorts its clusters by cell key, which is the one freedom step 6 of the contract removes.

`mutant` names one rule to change; tests/test_simplify_cpu.py shows that each changes the result of a named case."""
import ctypes
import ctypes.util
import math

import numpy as np

OK, INVALID_DATA, UNSUPPORTED = 0, 1, 4      # tc_status, include/threecrate_hip.h
NO_VERTEX = 0xFFFFFFFF
DEFAULT_ANGLE = float(np.float32(45.0) * (np.float32(np.pi) / np.float32(180.0)))        # 45.0f32.to_radians()

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cosf.restype, _libm.cosf.argtypes = ctypes.c_float, [ctypes.c_float]


def cosf(x):
    return np.float32(_libm.cosf(ctypes.c_float(float(np.float32(x)))))


class CheckFailed(Exception):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def cell_size(mn, mx, n, ratio, mutant=None):
    """step 2 -> (cell, dim)"""
    size = mx.astype(np.float64) - mn.astype(np.float64)
    if mutant == "target_f64":
        target = max((1.0 - float(np.float32(ratio))) * float(n), 1.0)
    else:
        target = float(max((np.float32(1.0) - np.float32(ratio)) * np.float32(n), np.float32(1.0)))
    extents = [float(s) for s in size if (s >= 1e-6 if mutant == "extent_ge" else s > 1e-6)]
    if not extents:
        return 1.0, 0
    product = 1.0
    for e in extents:
        product *= e
    return math.pow(product / target, 1.0 / len(extents)), len(extents)


def face_normals(v, f):
    """step 3's face normal, f32"""
    with np.errstate(all="ignore"):
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        a, b = v1 - v0, v2 - v0
        nx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        ny = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        nz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        good = ln > np.float32(1e-12)
        safe = np.where(good, ln, np.float32(1.0))
        out = np.stack([nx / safe, ny / safe, nz / safe], axis=1)
        out[~good] = (0.0, 0.0, 1.0)
    return out.astype(np.float32)


def edge_classes(v, f, threshold, mutant=None):
    """step 3 -> boundary, feature (bool per vertex)"""
    n = len(v)
    ends = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2)       # edge 3 f + k
    lo, hi = ends.min(1), ends.max(1)
    key = lo * n + hi
    order = np.argsort(key, kind="stable")                                                     # faces ascending inside a run
    ks = key[order]
    head = np.r_[True, ks[1:] != ks[:-1]]
    start = np.flatnonzero(head)
    count = np.diff(np.r_[start, len(ks)])
    boundary, feature = np.zeros(n, bool), np.zeros(n, bool)
    one = start[count <= 2] if mutant == "boundary_le2" else start[count == 1]
    boundary[lo[order[one]]] = True
    boundary[hi[order[one]]] = True
    two = start[count == 2]
    if len(two):
        fn = face_normals(v, f)
        a, b = fn[order[two] // 3], fn[order[two + 1] // 3]
        dot = (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
        c = cosf(threshold)
        sharp = two[dot <= c] if mutant == "dot_le" else two[dot < c]
        feature[lo[order[sharp]]] = True
        feature[hi[order[sharp]]] = True
    return boundary, feature


def _fold(values, members, starts, counts, dtype):
    """per cluster the sequential fold from +0 over its members in order, one rounding per add; vectorised over the clusters"""
    acc = np.zeros((len(starts),) + values.shape[1:], dtype)
    live = np.arange(len(starts))
    for k in range(int(counts.max()) if len(counts) else 0):
        live = live[counts[live] > k]
        acc[live] = acc[live] + values[members[starts[live] + k]].astype(dtype)
    return acc


def check(v, f, ratio, strategy, preserve_boundary, threshold):
    """checks 2 to 6 of the header (1 is about pointers), in order"""
    n, m = len(v), len(f)
    if n == 0 or m == 0:
        raise CheckFailed(INVALID_DATA, "Mesh is empty")
    if strategy not in (0, 1) or preserve_boundary not in (0, 1):
        raise CheckFailed(INVALID_DATA, "strategy / preserve_boundary")
    if not (0.0 <= np.float32(ratio) <= 1.0):
        raise CheckFailed(INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0")
    if not np.isfinite(np.float32(threshold)):
        raise CheckFailed(INVALID_DATA, "feature_angle_threshold is not finite")
    if (f >= n).any():
        raise CheckFailed(INVALID_DATA, "a face index is >= n_vertices")
    if not np.isfinite(v).all():
        raise CheckFailed(INVALID_DATA, "a vertex coordinate is not finite")


def simplify(vertices, faces, ratio, strategy=0, preserve_boundary=1, threshold=DEFAULT_ANGLE, normals=None, colors=None, mutant=None):
    """-> dict(vertices, faces, normals, colors, map, and what the case proofs read: sizes, classes, dim, cell, degenerate, repeated)"""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    n, m = len(v), len(f)
    check(v, f, ratio, strategy, preserve_boundary, threshold)
    if np.float32(ratio) == 0.0:
        return dict(vertices=v.copy(), faces=f.astype(np.uint32), normals=None if normals is None else np.array(normals, np.float32),
                    colors=None if colors is None else np.array(colors, np.uint8), map=np.arange(n, dtype=np.uint32), copy=True)
    mn, mx = v.min(0), v.max(0)
    cell, dim = cell_size(mn, mx, n, ratio, mutant)
    size = mx.astype(np.float64) - mn.astype(np.float64)
    if not (np.floor(size / cell) < 2 ** 20).all():
        raise CheckFailed(UNSUPPORTED, "a cell index does not fit 20 bits")
    boundary, feature = edge_classes(v, f, threshold, mutant)
    cls = np.where(boundary & bool(preserve_boundary), 1, np.where(feature, 2, 0)).astype(np.int64)
    idx = np.floor((v.astype(np.float64) - mn.astype(np.float64)) / cell).astype(np.int64)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 22) | (idx[:, 2] << 2) | (0 if mutant == "class_ignored" else cls)
    members = np.argsort(key, kind="stable")
    ks = key[members]
    head = np.r_[True, ks[1:] != ks[:-1]]
    starts = np.flatnonzero(head)
    counts = np.diff(np.r_[starts, n])
    cluster_of = np.empty(n, np.int64)
    cluster_of[members] = np.cumsum(head) - 1
    R = len(starts)
    # step 7
    valence = np.bincount(f.reshape(-1), minlength=n)
    if strategy == 1:
        w = (valence if mutant == "valence_unclamped" else np.maximum(valence, 1)).astype(np.float64)
        s = _fold(v.astype(np.float64) * w[:, None], members, starts, counts, np.float64)
        W = _fold(w, members, starts, counts, np.float64)
        with np.errstate(all="ignore"):
            rep = (s / W[:, None]).astype(np.float32)
    elif mutant == "centroid_f32":
        rep = _fold(v, members, starts, counts, np.float32) / counts.astype(np.float32)[:, None]
    else:
        rep = (_fold(v, members, starts, counts, np.float64) / counts.astype(np.float64)[:, None]).astype(np.float32)
    single = counts == 1
    if not (mutant == "single_divided" and strategy == 1):
        rep[single] = v[members[starts[single]]]
    # step 8
    c = cluster_of[f]
    live = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 2] != c[:, 0])
    tri = np.sort(c, axis=1)
    k1 = np.unique(tri[:, 0] * R + tri[:, 1], return_inverse=True)[1].reshape(-1)
    k2 = k1 * R + tri[:, 2]
    cand = np.flatnonzero(live)
    if mutant == "last_face_wins":
        first = len(cand) - 1 - np.unique(k2[cand][::-1], return_index=True)[1]
    else:
        first = np.unique(k2[cand], return_index=True)[1]
    kept = cand[first] if mutant == "faces_resorted" else np.sort(cand[first])
    new_faces = c[kept]
    if mutant == "orientation_canonical":
        new_faces = tri[kept]
    # step 9
    used = np.zeros(R, bool)
    used[new_faces.reshape(-1)] = True
    if mutant == "unused_kept":
        used[:] = True
    cpos = np.cumsum(used) - 1
    out = dict(vertices=rep[used], faces=cpos[new_faces].astype(np.uint32), normals=None, colors=None,
               map=np.where(used[cluster_of], cpos[cluster_of], NO_VERTEX).astype(np.uint32), copy=False,
               sizes=counts, used=used, classes=np.bincount(cls, minlength=3), cluster_classes=ks[starts] & 3, dim=dim, cell=cell,
               degenerate=int((~live).sum()), repeated=int(live.sum() - len(kept)), boundary=boundary, feature=feature, cluster_of=cluster_of)
    if normals is not None:
        with np.errstate(all="ignore"):
            s = _fold(np.ascontiguousarray(normals, np.float32).reshape(-1, 3), members, starts, counts, np.float32)
            ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
            good = ln > np.float32(1e-12)
            if mutant != "normals_raw":
                s[good] = s[good] / ln[good][:, None]
        out["normals"] = s[used]
    if colors is not None:
        s = _fold(np.ascontiguousarray(colors, np.uint8).reshape(-1, 3), members, starts, counts, np.uint32)
        cnt = counts.astype(np.uint32)[:, None]
        out["colors"] = (((s + cnt // 2) // cnt) if mutant == "colour_nearest" else (s // cnt)).astype(np.uint8)[used]
    return out


# ---- the reference's uniform road, restated literally -------------------------------------------------------------------------
def literal(vertices, faces, ratio, strategy=0, preserve_boundary=1, threshold=DEFAULT_ANGLE, normals=None, colors=None):
    """clustering.rs:785-829 for ClusteringMode::Uniform with Python dicts and sets; f32 values are np.float32 scalars, f64 values Python
    floats.  -> (clusters as (key, members) in insertion order, new_vertices, faces, normals, colors) with the vertex order of that
    insertion order."""
    f32 = np.float32
    v = [tuple(f32(x) for x in row) for row in np.asarray(vertices, np.float32).reshape(-1, 3)]
    fs = [tuple(int(i) for i in row) for row in np.asarray(faces).reshape(-1, 3)]
    n = len(v)
    mn, mx = [float("inf")] * 3, [float("-inf")] * 3
    for p in v:
        for i in range(3):
            mn[i], mx[i] = min(mn[i], float(p[i])), max(mx[i], float(p[i]))
    valence = [0] * n
    for face in fs:
        for vi in face:
            valence[vi] += 1
    edges = lambda t: [(min(t[0], t[1]), max(t[0], t[1])), (min(t[1], t[2]), max(t[1], t[2])), (min(t[2], t[0]), max(t[2], t[0]))]
    boundary = set()
    if preserve_boundary:
        edge_count = {}
        for face in fs:
            for e in edges(face):
                edge_count[e] = edge_count.get(e, 0) + 1
        for (a, b), cnt in edge_count.items():
            if cnt == 1:
                boundary.update((a, b))
    cos_threshold = cosf(threshold)
    with np.errstate(all="ignore"):
        fnorm = []
        for t in fs:
            e1 = [v[t[1]][i] - v[t[0]][i] for i in range(3)]
            e2 = [v[t[2]][i] - v[t[0]][i] for i in range(3)]
            c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
            ln = np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
            fnorm.append([x / ln for x in c] if ln > f32(1e-12) else [f32(0), f32(0), f32(1)])
        edge_faces = {}
        for fi, face in enumerate(fs):
            for e in edges(face):
                edge_faces.setdefault(e, []).append(fi)
        feature = set()
        for (a, b), lst in edge_faces.items():
            if len(lst) == 2:
                p, q = fnorm[lst[0]], fnorm[lst[1]]
                if p[0] * q[0] + p[1] * q[1] + p[2] * q[2] < cos_threshold:
                    feature.update((a, b))
    target = float(max((f32(1.0) - f32(ratio)) * f32(n), f32(1.0)))
    extents = [mx[i] - mn[i] for i in range(3) if mx[i] - mn[i] > 1e-6]
    cell = 1.0
    if extents:
        product = 1.0
        for e in extents:
            product *= e
        cell = math.pow(product / target, 1.0 / len(extents))
    cells = {}
    for vi, p in enumerate(v):
        k = tuple(int(math.floor((float(p[i]) - mn[i]) / cell)) for i in range(3))
        cls = 1 if (preserve_boundary and vi in boundary) else (2 if vi in feature else 0)
        cells.setdefault(k + (cls,), []).append(vi)
    return _literal_build(list(cells.items()), v, fs, valence, strategy, normals, colors)


def _literal_build(clusters, v, fs, valence, strategy, normals, colors):
    """build_simplified_mesh, clustering.rs:651-781, over `clusters` in the order given"""
    f32 = np.float32
    vertex_to_cluster = {}
    for ci, (_, cluster) in enumerate(clusters):
        for vi in cluster:
            vertex_to_cluster[vi] = ci
    reps = []
    for _, cluster in clusters:
        if len(cluster) == 1:
            reps.append(v[cluster[0]])
        elif strategy == 0:
            s = [0.0, 0.0, 0.0]
            for vi in cluster:
                for i in range(3):
                    s[i] += float(v[vi][i])
            reps.append(tuple(f32(x / float(len(cluster))) for x in s))
        else:
            s, wt = [0.0, 0.0, 0.0], 0.0
            for vi in cluster:
                w = float(max(valence[vi], 1))
                for i in range(3):
                    s[i] += float(v[vi][i]) * w
                wt += w
            reps.append(tuple(f32(x / wt) for x in s))
    new_faces, seen = [], set()
    for face in fs:
        c = [vertex_to_cluster[i] for i in face]
        if c[0] == c[1] or c[1] == c[2] or c[2] == c[0]:
            continue
        k = tuple(sorted(c))
        if k not in seen:
            seen.add(k)
            new_faces.append(c)
    used = {ci for face in new_faces for ci in face}
    old_to_new, out_v, out_n, out_c = {}, [], [], []
    with np.errstate(all="ignore"):
        for ci, (_, cluster) in enumerate(clusters):
            if ci not in used:
                continue
            old_to_new[ci] = len(out_v)
            out_v.append(reps[ci])
            if normals is not None:
                avg = [f32(0), f32(0), f32(0)]
                for vi in cluster:
                    avg = [avg[i] + f32(normals[vi][i]) for i in range(3)]
                ln = np.sqrt(avg[0] * avg[0] + avg[1] * avg[1] + avg[2] * avg[2])
                if ln > f32(1e-12):
                    avg = [x / ln for x in avg]
                out_n.append(avg)
            if colors is not None:
                out_c.append([sum(int(colors[vi][i]) for vi in cluster) // len(cluster) for i in range(3)])
    return dict(clusters=clusters, vertices=np.array(out_v, np.float32).reshape(-1, 3),
                faces=np.array([[old_to_new[i] for i in face] for face in new_faces], np.uint32).reshape(-1, 3),
                normals=None if normals is None else np.array(out_n, np.float32).reshape(-1, 3),
                colors=None if colors is None else np.array(out_c, np.uint8).reshape(-1, 3))


def literal_in_contract_order(vertices, faces, ratio, strategy=0, preserve_boundary=1, threshold=DEFAULT_ANGLE, normals=None, colors=None):
    """the literal road with its clusters sorted by (ix, iy, iz, class): the permutation step 6 fixes.  build_simplified_mesh is run again
    over the sorted list, so the faces come out renumbered as well"""
    first = literal(vertices, faces, ratio, strategy, preserve_boundary, threshold, normals, colors)
    f32 = np.float32
    v = [tuple(f32(x) for x in row) for row in np.asarray(vertices, np.float32).reshape(-1, 3)]
    fs = [tuple(int(i) for i in row) for row in np.asarray(faces).reshape(-1, 3)]
    valence = [0] * len(v)
    for face in fs:
        for vi in face:
            valence[vi] += 1
    return _literal_build(sorted(first["clusters"]), v, fs, valence, strategy, normals, colors)
