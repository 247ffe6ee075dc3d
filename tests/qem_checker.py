"""The contract of include/threecrate_hip_qem.h in numpy (test infrastructure): quadric-error edge collapse in rounds, every operation in
the header's order, one rounding per operation -- f32 values are np.float32 arrays, f64 values np.float64 arrays, and no expression below
gives numpy the chance to fuse or reorder (each line is one operation per element).
  simplify(v, f, cfg, mutant=None)   the contract (and, with `mutant`, the contract with one rule changed) -> a dict
  literal(v, f, cfg)                 quadric_error.rs restated: one global queue (heapq, an insertion counter breaking ties), neighbours in
                                     ascending index, the queue rebuilt every 100 collapses.  For the quality comparison only
  surface_error(v_in, v_out, f_out)  mean distance of the input vertices to the output surface over the input's box diagonal, brute force
"""
import heapq

import numpy as np

OK, INVALID_DATA, UNSUPPORTED = 0, 1, 4
NO_VERTEX = 0xFFFFFFFF
MAX_POINTS = 0xFFFFFFF0
F, D = np.float32, np.float64
SIGN = np.uint64(1 << 63)


class CheckFailed(Exception):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def config(ratio, preserve_boundary=1, max_edge_length=0.0):
    return {"ratio": ratio, "preserve_boundary": preserve_boundary, "max_edge_length": max_edge_length}


def cost_key(cost):
    """f64::total_cmp as a u64 order: flip all bits when the sign is set, else set the sign bit"""
    bits = np.ascontiguousarray(cost, D).view(np.uint64)
    return np.where((bits & SIGN) != 0, ~bits, bits | SIGN)


def total_cmp(a, b):
    """Rust's f64::total_cmp restated (core::f64): the bits as i64, the lower 63 flipped when negative, compared as integers"""
    def k(x):
        i = int(np.array([x], D).view(np.int64)[0])
        return i ^ (((i >> 63) & 0xFFFFFFFFFFFFFFFF) >> 1)
    ka, kb = k(a), k(b)
    return (ka > kb) - (ka < kb)


def target_faces(ratio, m, mutant=None):
    """step 1"""
    if mutant == "target_f64":
        return int((1.0 - float(F(ratio))) * float(m))
    return int(F(F(1.0) - F(ratio)) * F(m))


def planes(v, f):
    """step 3 -> (m, 4) f32"""
    with np.errstate(all="ignore"):
        v0, v1, v2 = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
        e1, e2 = v1 - v0, v2 - v0
        p0, p1 = e1[:, 1] * e2[:, 2], e1[:, 2] * e2[:, 1]
        p2, p3 = e1[:, 2] * e2[:, 0], e1[:, 0] * e2[:, 2]
        p4, p5 = e1[:, 0] * e2[:, 1], e1[:, 1] * e2[:, 0]
        cx, cy, cz = p0 - p1, p2 - p3, p4 - p5
        xx, yy, zz = cx * cx, cy * cy, cz * cz
        ln = np.sqrt((xx + yy) + zz)
        nx, ny, nz = cx / ln, cy / ln, cz / ln
        dx, dy, dz = nx * v0[:, 0], ny * v0[:, 1], nz * v0[:, 2]
        d = -((dx + dy) + dz)
    out = np.stack([nx, ny, nz, d], axis=1).astype(F)
    bad = ~(np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz))
    out[bad] = [0.0, 0.0, 1.0, 0.0]
    return out


PAIRS = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]      # aa ab ac ad bb bc bd cc cd dd


def plane_quadrics(pl):
    p = pl.astype(D)
    return np.stack([p[:, i] * p[:, j] for i, j in PAIRS], axis=1)


def vertex_quadrics(n, f, quad, mutant=None):
    """step 4: per vertex the fold from +0.0 over its incident faces in ascending face index (fold_reversed: descending).
    -> (n, 10) f64, the longest ring"""
    q = np.zeros((n, 10), D)
    if len(f) == 0:
        return q, 0
    vert = f.reshape(-1)                                # corner 3 f + k
    corner = np.arange(len(vert))
    order = np.argsort(vert, kind="stable")             # by vertex, ascending corner inside
    sv, sc = vert[order], corner[order]
    start = np.r_[0, np.nonzero(sv[1:] != sv[:-1])[0] + 1]
    length = np.diff(np.r_[start, len(sv)])
    rank = np.arange(len(sv)) - np.repeat(start, length)
    if mutant == "fold_reversed":
        rank = np.repeat(length, length) - 1 - rank
    for j in range(int(length.max())):
        sel = rank == j                                 # one corner per vertex: no vertex twice in one step
        q[sv[sel]] = q[sv[sel]] + quad[sc[sel] // 3]
    return q, int(length.max())


def solve(q, plo, phi, mutant=None):
    """steps 5d and 5e for E edges: q (E, 10) the summed quadrics -> position (E, 3) f32, cost (E,) f64, used_midpoint (E,) bool"""
    a00, a01, a02, b0, a11, a12, b1, a22, b2, q33 = (q[:, k] for k in range(10))
    with np.errstate(all="ignore"):
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        x = -(((c00 * b0 + c01 * b1) + c02 * b2) / det)
        y = -(((c01 * b0 + c11 * b1) + c12 * b2) / det)
        z = -(((c02 * b0 + c12 * b1) + c22 * b2) / det)
        pos = np.stack([x, y, z], axis=1).astype(F)
        solved = np.isfinite(pos).all(axis=1)
        if mutant != "det_zero_unchecked":
            solved &= (det != 0.0) & np.isfinite(det)
        mid = (plo + phi) * F(0.5)
        if mutant == "fallback_endpoint":
            mid = plo.copy()
        pos[~solved] = mid[~solved]
        X, Y, Z = (pos[:, k].astype(D) for k in range(3))
        r0 = ((a00 * X + a01 * Y) + a02 * Z) + b0
        r1 = ((a01 * X + a11 * Y) + a12 * Z) + b1
        r2 = ((a02 * X + a12 * Y) + a22 * Z) + b2
        r3 = ((b0 * X + b1 * Y) + b2 * Z) + q33
        cost = ((X * r0 + Y * r1) + Z * r2) + r3
    return pos, cost, ~solved


def check(v, f, cfg):
    """checks 2 to 6 of the header (1 is about pointers), in order"""
    n, m = len(v), len(f)
    if n == 0 or m == 0:
        raise CheckFailed(INVALID_DATA, "Mesh is empty")
    if cfg["preserve_boundary"] not in (0, 1):
        raise CheckFailed(INVALID_DATA, "simplify_quadric: preserve_boundary is neither 0 nor 1")
    ratio = F(cfg["ratio"])
    if not (ratio >= 0 and ratio <= 1):
        raise CheckFailed(INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0")
    if not F(cfg["max_edge_length"]) >= 0:
        raise CheckFailed(INVALID_DATA, "simplify_quadric: max_edge_length is negative or NaN")
    if n >= MAX_POINTS:
        raise CheckFailed(UNSUPPORTED, "simplify_quadric: n_vertices is 2^32 - 16 or more")
    if 3 * m >= MAX_POINTS:
        raise CheckFailed(UNSUPPORTED, "simplify_quadric: 3 n_faces is 2^32 - 16 or more")
    if (f >= n).any() or (f < 0).any():
        raise CheckFailed(INVALID_DATA, "simplify_quadric: a face index is >= n_vertices")
    if not np.isfinite(v).all():
        raise CheckFailed(INVALID_DATA, "simplify_quadric: a vertex coordinate is not finite")


def simplify(vertices, faces, cfg, mutant=None):
    """-> dict(vertices, faces, map, rounds, and what the tests read: target, alive0, selected_none, last_multiplicity, min_cost,
    midpoints, longest_ring, per_round)"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    check(v, f, cfg)
    n, m = len(v), len(f)
    info = {"target": None, "alive0": m, "selected_none": False, "last_multiplicity": 0, "min_cost": np.inf, "midpoints": 0, "longest_ring": 0,
            "per_round": [], "copy": False}
    if F(cfg["ratio"]) == 0:
        return dict(info, vertices=v.copy(), faces=f.astype(np.uint32), map=np.arange(n, dtype=np.uint32), rounds=0, copy=True)
    target = target_faces(cfg["ratio"], m, mutant)
    distinct = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])
    pos = v.copy()
    if mutant == "degenerate_quadric":                  # the reference: a degenerate face adds the plane z = 0 to its vertices
        quads = plane_quadrics(planes(pos, f))
        qv, ring = vertex_quadrics(n, f, quads, mutant)
        f = f[distinct]
    else:
        f = f[distinct]
        qv, ring = vertex_quadrics(n, f, plane_quadrics(planes(pos, f)), mutant)
    info.update(target=target, alive0=len(f), longest_ring=ring)
    parent = np.arange(n)
    max_len, preserve = F(cfg["max_edge_length"]), bool(cfg["preserve_boundary"])
    rounds, fixed_boundary = 0, None
    while len(f) > target:
        ends = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2)
        key = (ends.min(axis=1).astype(np.uint64) << np.uint64(32)) | ends.max(axis=1).astype(np.uint64)
        uniq, mult = np.unique(key, return_counts=True)             # ascending key
        lo, hi = (uniq >> np.uint64(32)).astype(np.int64), (uniq & np.uint64(0xFFFFFFFF)).astype(np.int64)
        cand = np.ones(len(uniq), bool)
        if preserve:
            bnd = np.zeros(n, bool)
            single = mult <= 2 if mutant == "boundary_le2" else mult == 1
            bnd[lo[single]] = True
            bnd[hi[single]] = True
            if mutant == "boundary_once":
                fixed_boundary = bnd if fixed_boundary is None else fixed_boundary
                bnd = fixed_boundary
            cand &= ~(bnd[lo] | bnd[hi])
        if max_len > 0:
            d = pos[lo] - pos[hi]
            xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
            cand &= ~(np.sqrt((xx + yy) + zz) > max_len)
        q = qv[lo] + qv[hi]
        where, cost, midpoint = solve(q, pos[lo], pos[hi], mutant)
        cand &= ~np.isnan(cost)
        c = np.nonzero(cand)[0]                                     # ascending unique-edge index: the (lo, hi) order
        if len(c) == 0:
            info["selected_none"] = True
            break
        ck = cost_key(cost[c])
        order = np.argsort(ck, kind="stable")                       # equal keys keep ascending (lo, hi)
        if mutant == "tie_descending":
            order = np.lexsort((-np.arange(len(c)), ck))
        rank = np.empty(len(c), np.int64)
        rank[order] = np.arange(len(c))
        best = np.full(n, len(c), np.int64)
        np.minimum.at(best, lo[c], rank)
        np.minimum.at(best, hi[c], rank)
        sel = (best[lo[c]] == rank) & (best[hi[c]] == rank)
        chosen = c[order][sel[order]]                               # the selected edges in rank order
        before = np.cumsum(mult[chosen]) - mult[chosen]
        take = chosen if mutant == "cut_all" else chosen[before < len(f) - target]
        info["min_cost"] = min(info["min_cost"], float(cost[c].min()))
        info["midpoints"] += int(midpoint[take].sum())
        info["last_multiplicity"] = int(mult[take].max())
        info["per_round"].append((len(f), len(chosen), len(take)))
        if mutant == "survivor_hi":
            pos[hi[take]] = where[take]
            qv[hi[take]] = q[take]
            parent[lo[take]] = hi[take]
        else:
            pos[lo[take]] = where[take]
            qv[lo[take]] = q[take]
            parent[hi[take]] = lo[take]
        f = parent[f]
        f = f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]
        rounds += 1
    root = parent.copy()
    while True:
        up = parent[root]
        if (up == root).all():
            break
        root = up
    used = np.zeros(n, bool)
    used[f.reshape(-1)] = True
    number = np.cumsum(used) - 1
    vmap = np.where(used[root], number[root], NO_VERTEX).astype(np.uint32)
    return dict(info, vertices=pos[used], faces=number[f].astype(np.uint32).reshape(-1, 3), map=vmap, rounds=rounds)


# ---- quadric_error.rs, restated ----
def literal(vertices, faces, cfg):
    """QuadricErrorSimplifier::simplify (quadric_error.rs:413-473) with Python sets and numpy 4 x 4 f64 matrices.  Where the reference's
    order is that of a HashSet or of equal priorities in its queue, this takes ascending index and insertion order: its tie order is
    not the reference's own.  -> (vertices, faces)"""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    fs = [[int(i) for i in row] for row in np.asarray(faces).reshape(-1, 3)]
    n, m = len(v), len(fs)
    if n == 0 or m == 0:
        raise CheckFailed(INVALID_DATA, "Mesh is empty")
    ratio = F(cfg["ratio"])
    if not (ratio >= 0 and ratio <= 1):
        raise CheckFailed(INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0")
    if ratio == 0:
        return v.copy(), np.asarray(fs, np.uint32).reshape(-1, 3)
    target = int(F(F(1.0) - ratio) * F(m))
    max_len = F(cfg["max_edge_length"]) if cfg["max_edge_length"] else None
    preserve = bool(cfg["preserve_boundary"])
    pos = [v[i].copy() for i in range(n)]
    quadric = [np.zeros((4, 4), D) for _ in range(n)]
    vfaces, nbr = [set() for _ in range(n)], [set() for _ in range(n)]
    pl = planes(v, np.asarray(fs, np.int64)).astype(D)
    for fi, face in enumerate(fs):
        k = np.outer(pl[fi], pl[fi])
        for i in face:
            quadric[i] = quadric[i] + k
            vfaces[i].add(fi)
        a, b, c = face
        nbr[a] |= {b, c}
        nbr[b] |= {a, c}
        nbr[c] |= {a, b}

    def boundary_vertices(face_list):
        count = {}
        for a, b, c in face_list:
            for e in ((min(a, b), max(a, b)), (min(b, c), max(b, c)), (min(c, a), max(c, a))):
                count[e] = count.get(e, 0) + 1
        return {x for e, k in count.items() if k == 1 for x in e}

    def collapse_cost(i, j):
        if max_len is not None:
            d = pos[i] - pos[j]
            if np.sqrt((d * d).sum(dtype=F)) > max_len:
                return None
        q = quadric[i] + quadric[j]
        a, b = q[:3, :3], q[:3, 3]
        with np.errstate(all="ignore"):
            det = (a[0, 0] * (a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]) - a[0, 1] * (a[1, 0] * a[2, 2] - a[1, 2] * a[2, 0])
                   + a[0, 2] * (a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]))
            if det != 0:                                # try_inverse: None exactly when the determinant is zero
                adj = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                                [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                                [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]], D)
                p = (-(adj / det) @ b).astype(F)
            else:
                p = (pos[i] + pos[j]) * F(0.5)
            h = np.array([p[0], p[1], p[2], 1.0], D)
            cost = float(h @ q @ h)
        return cost, p

    def generate(face_list):
        bv = boundary_vertices(face_list) if preserve else set()
        out = []
        for i in range(n):
            for j in sorted(nbr[i]):
                if i < j and not (preserve and (i in bv or j in bv)):
                    cc = collapse_cost(i, j)
                    if cc is not None:
                        out.append((i, j) + cc)
        return out

    class Entry:
        __slots__ = ("cost", "tick", "i", "j", "p")

        def __init__(self, cost, tick, i, j, p):
            self.cost, self.tick, self.i, self.j, self.p = cost, tick, i, j, p

        def __lt__(self, other):
            c = total_cmp(self.cost, other.cost)
            return c < 0 or (c == 0 and self.tick < other.tick)

    tick = 0
    heap = []
    for i, j, cost, p in generate(fs):
        heap.append(Entry(cost, tick, i, j, p))
        tick += 1
    heapq.heapify(heap)
    counter = 0
    while len(fs) > target and heap:
        e = heapq.heappop(heap)
        if e.j not in nbr[e.i]:
            continue
        i, j = e.i, e.j
        pos[i] = e.p
        quadric[i] = quadric[i] + quadric[j]
        fs = [[i if x == j else x for x in face] for face in fs]
        fs = [face for face in fs if face[0] != face[1] and face[1] != face[2] and face[2] != face[0]]
        for k in list(nbr[j]):
            if k != i:
                nbr[i].add(k)
                nbr[k].discard(j)
                nbr[k].add(i)
        nbr[i].discard(j)
        nbr[j].clear()
        vfaces[j].clear()
        counter += 1
        if counter % 100 == 0:
            heap = []
            for a, b, cost, p in generate(fs):
                heap.append(Entry(cost, tick, a, b, p))
                tick += 1
            heapq.heapify(heap)
    valid = [i for i in range(n) if nbr[i] or vfaces[i]]
    new = {old: k for k, old in enumerate(valid)}
    out_f = [[new[x] for x in face] for face in fs if all(x in new for x in face)]
    return np.asarray([pos[i] for i in valid], F).reshape(-1, 3), np.asarray(out_f, np.uint32).reshape(-1, 3)


# ---- quality ----
def _segment_distance2(p, a, b):
    """squared distance of points p (P, 1, 3) to segments a-b (1, T, 3), f64"""
    ab = b - a
    t = ((p - a) * ab).sum(axis=2) / np.maximum((ab * ab).sum(axis=2), 1e-300)
    t = np.clip(t, 0.0, 1.0)
    d = p - (a + t[..., None] * ab)
    return (d * d).sum(axis=2)


def surface_error(v_in, v_out, f_out):
    """the mean over the input vertices of the exact point-triangle distance to the output mesh, divided by the diagonal of the input's
    box: the minimum over the triangles of (the distance to the plane where the foot lies inside the triangle, else the distance to
    the nearest side).  Brute force, f64."""
    p = np.asarray(v_in, D)[:, None, :]
    tri = np.asarray(v_out, D)[np.asarray(f_out).astype(np.int64)]
    a, b, c = tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]
    d2 = np.minimum(np.minimum(_segment_distance2(p, a, b), _segment_distance2(p, b, c)), _segment_distance2(p, c, a))
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(axis=2)
    with np.errstate(all="ignore"):
        h = ((p - a) * nrm).sum(axis=2)
        foot = p - (h / nn)[..., None] * nrm
        inside = np.ones(h.shape, bool)
        for s, e in ((a, b), (b, c), (c, a)):
            inside &= (np.cross(e - s, foot - s) * nrm).sum(axis=2) >= 0.0
        inside &= nn > 0.0
        plane2 = h * h / nn
    d2 = np.where(inside, np.minimum(d2, plane2), d2)
    diag = np.sqrt(((np.asarray(v_in, D).max(axis=0) - np.asarray(v_in, D).min(axis=0)) ** 2).sum())
    return float(np.sqrt(d2.min(axis=1)).mean() / diag)
