"""numpy restatement of NDT registration (threecrate-algorithms/src/ndt_registration.rs), as include/threecrate_hip_ndt.h pins it, with a
dtype switch: float32 with every sum sequential and left to right is the reference's arithmetic (np.cumsum accumulates in order,
unlike np.sum), float64 is the yardstick the device is measured against.  Poses are the 7-float isometry (qi qj qk qw tx ty tz).

Besides the result every evaluation leaves a record: the keys of the transformed source points, the hit count, and the smallest distance
of any transformed coordinate from a voxel face in units of the resolution -- the preconditions of the GPU tests are checked on those.

The inputs of the GPU tests are made here too (surface_pair): a noisy sine surface over a 4 x 4 patch, the source a second
sample of it, started from a = 0.03 rad and t = (0.05, -0.04, 0.02); well conditioned (cond(H) of a few tens)."""
import functools

import numpy as np

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)
FACE_MARGIN = 1e-4          # in units of the resolution: no compared evaluation has a coordinate nearer to a voxel face
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

# The rules a mutant changes (tests/test_ndt_edges_cpu.py holds every mutant to a named case of tests/ndt_cases.py that tells it from
# the contract); build(), evaluate() and register() take a `rules` dict that replaces some of them.
RULES = dict(
    key_arith=lambda x, res: x / res,                           # true division, in the key dtype (:61-67)
    floor=np.floor,
    saturate=lambda f: np.clip(np.nan_to_num(f.astype(np.float64), nan=0.0), I32_MIN, I32_MAX),        # Rust's `as i32`, ndt_key()
    source_scores=lambda p: np.isfinite(p).all(axis=1),         # the header's deviation: a non-finite transformed point scores nothing
    survives=lambda count, min_points: count >= min_points,     # :87
    regular=1e-4,                                               # cov + 1e-4 I (:103)
    divisor=lambda n: n)                                        # the covariance is divided by n, not n - 1 (:99)


def _rules(rules):
    assert set(rules or {}) <= set(RULES), set(rules) - set(RULES)
    return dict(RULES, **(rules or {}))


class NdtError(Exception):
    """Error::Algorithm of :194-209"""


# ---- keys and the voxel build (:61-111) ----
def keys_of(p, res, dtype, rules=None):
    """(floor(x / res), ...) as i32: true division in `dtype`, floor, saturating to the i32 range (:61-67); int64 holds them"""
    r = _rules(rules)
    with np.errstate(over="ignore", invalid="ignore"):
        return r["saturate"](r["floor"](r["key_arith"](np.asarray(p, dtype), dtype(res)))).astype(np.int64)


def _inverse3(m, dtype):
    """nalgebra's closed-form 3 x 3 try_inverse; None for a zero determinant"""
    m11, m12, m13, m21, m22, m23, m31, m32, m33 = [dtype(v) for v in m.reshape(9)]
    a = m22 * m33 - m32 * m23
    b = m21 * m33 - m31 * m23
    c = m21 * m32 - m31 * m22
    det = m11 * a - m12 * b + m13 * c
    if det == 0:
        return None
    return np.array([[a / det, (m13 * m32 - m33 * m12) / det, (m12 * m23 - m22 * m13) / det],
                     [-b / det, (m11 * m33 - m31 * m13) / det, (m13 * m21 - m23 * m11) / det],
                     [c / det, (m12 * m31 - m32 * m11) / det, (m11 * m22 - m21 * m12) / det]], dtype)


def build(target, res, min_points, dtype=np.float32, key_dtype=None, rules=None):
    """-> keys (V, 3) int64 ascending by (kx, ky, kz), counts (V,), mean (V, 3), inv_cov (V, 3, 3), all sums in input order.
    A point with a non-finite coordinate takes no part (the header's deviation).  key_dtype (default: dtype) is the arithmetic of the keys:
    key_dtype = float32 with dtype = float64 is the header's keys with f64 sums."""
    r = _rules(rules)
    t = np.asarray(target, np.float32).reshape(-1, 3)
    t = t[np.isfinite(t).all(axis=1)]
    k = keys_of(t, res, key_dtype or dtype, rules)
    t = t.astype(dtype)
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))             # stable: a voxel keeps input order
    ks = k[order]
    heads = np.r_[True, (ks[1:] != ks[:-1]).any(axis=1)] if len(ks) else np.zeros(0, bool)
    starts = np.r_[np.nonzero(heads)[0], len(ks)]
    keys, counts, means, invs = [], [], [], []
    for s, e in zip(starts[:-1], starts[1:]):
        if not r["survives"](e - s, min_points):
            continue
        pts = t[order[s:e]]
        n = dtype(e - s)
        mean = (np.cumsum(pts, axis=0, dtype=dtype)[-1] / n).astype(dtype)
        d = (pts - mean).astype(dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            cov = np.cumsum((d[:, :, None] * d[:, None, :]).astype(dtype), axis=0, dtype=dtype)[-1] / dtype(r["divisor"](e - s))
        cov = (cov + np.eye(3, dtype=dtype) * dtype(r["regular"])).astype(dtype)
        inv = _inverse3(cov, dtype)
        if inv is None:
            continue
        keys.append(ks[s]); counts.append(e - s); means.append(mean); invs.append(inv)
    v = len(keys)
    return (np.array(keys, np.int64).reshape(v, 3), np.array(counts, np.int64), np.array(means, dtype).reshape(v, 3),
            np.array(invs, dtype).reshape(v, 3, 3))


# ---- poses ----
def rotation_matrix(q, dtype):
    """nalgebra's to_rotation_matrix of q = (i j k w)"""
    i, j, k, w = [dtype(v) for v in q]
    two = dtype(2)
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj, ik, jk, wi = i * j * two, w * k * two, w * j * two, i * k * two, j * k * two, w * i * two
    return np.array([[ww + ii - jj - kk, ij - wk, wj + ik], [wk + ij, ww - ii + jj - kk, jk - wi], [ik - wj, wi + jk, ww - ii - jj + kk]], dtype)


def rotate(q, p, dtype):
    """UnitQuaternion * vector(s): t2 = (qv x p) * 2; (t2 * w + qv x t2) + p"""
    q = np.asarray(q, dtype)
    p = np.asarray(p, dtype)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    two = dtype(2)
    tx, ty, tz = (q[1] * z - q[2] * y) * two, (q[2] * x - q[0] * z) * two, (q[0] * y - q[1] * x) * two
    cx, cy, cz = q[1] * tz - q[2] * ty, q[2] * tx - q[0] * tz, q[0] * ty - q[1] * tx
    return np.stack([(tx * q[3] + cx) + x, (ty * q[3] + cy) + y, (tz * q[3] + cz) + z], axis=-1).astype(dtype)


def apply(pose, p, dtype):
    pose = np.asarray(pose, dtype)
    return (rotate(pose[:4], p, dtype) + pose[4:7]).astype(dtype)


def euler_quaternion(roll, pitch, yaw, dtype):
    """nalgebra's UnitQuaternion::from_euler_angles = Rz(yaw) Ry(pitch) Rx(roll), as (i j k w)"""
    h = dtype(0.5)
    sr, cr = np.sin(dtype(roll) * h), np.cos(dtype(roll) * h)
    sp, cp = np.sin(dtype(pitch) * h), np.cos(dtype(pitch) * h)
    sy, cy = np.sin(dtype(yaw) * h), np.cos(dtype(yaw) * h)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], dtype)


def compose(dq, dt, pose, dtype):
    """(Translation(dt), dq) o pose: q <- dq q, t <- dq t + dt"""
    pose = np.asarray(pose, dtype)
    di, dj, dk, dw = [dtype(v) for v in dq]
    qi, qj, qk, qw = pose[:4]
    q = [dw * qi + di * qw + dj * qk - dk * qj, dw * qj - di * qk + dj * qw + dk * qi, dw * qk + di * qj - dj * qi + dk * qw,
         dw * qw - di * qi - dj * qj - dk * qk]
    t = np.asarray(dt, dtype) + rotate(dq, pose[4:7], dtype)
    return np.array(q + list(t), dtype)


def matrix4(pose):
    """the 4 x 4 of a pose, in f64 from the numbers as they are"""
    pose = np.asarray(pose, np.float64)
    m = np.eye(4)
    m[:3, :3] = rotation_matrix(pose[:4], np.float64)
    m[:3, 3] = pose[4:7]
    return m


# ---- the 6 x 6 solve (nalgebra's lu().solve(): partial pivoting, the first of equal pivots) ----
def lu_solve(a, b, dtype):
    a = np.array(a, dtype)
    x = np.array(b, dtype)
    n = len(x)
    for i in range(n):
        p = i + int(np.argmax(np.abs(a[i:, i])))
        if a[p, i] == 0 or not np.isfinite(a[p, i]):
            return None
        if p != i:
            a[[i, p]] = a[[p, i]]
            x[[i, p]] = x[[p, i]]
        inv = dtype(1) / a[i, i]
        for r in range(i + 1, n):
            f = a[r, i] * inv
            a[r, i + 1:] = a[r, i + 1:] - f * a[i, i + 1:]
            x[r] = x[r] - f * x[i]
    for i in range(n - 1, -1, -1):
        s = x[i]
        for j in range(i + 1, n):
            s = s - a[i, j] * x[j]
        x[i] = s / a[i, i]
    return x.astype(dtype)


# ---- one evaluation (:117-176) ----
def _ranks(vkeys, keys):
    """The voxels' and the points' key triples as single int64 ranks that keep the lexicographic order, and which points have a voxel's
    coordinate on every axis.  Each axis is numbered by the voxels' distinct coordinates (at most V of them), so three of them pack into
    V^3 < 2^63 however wide the key box is (2^64 cells and more: the keys themselves would not pack)."""
    pv, pk, known = np.zeros(len(vkeys), np.int64), np.zeros(len(keys), np.int64), np.ones(len(keys), bool)
    for a in range(3):
        ux = np.unique(vkeys[:, a])
        assert float(len(ux)) ** (3 - a) * (abs(pv).max() + 1 if len(pv) else 1) < 2.0 ** 62
        at = np.minimum(np.searchsorted(ux, keys[:, a]), len(ux) - 1)
        known &= ux[at] == keys[:, a]
        pv, pk = pv * len(ux) + np.searchsorted(ux, vkeys[:, a]), pk * len(ux) + at
    return pv, pk, known


def evaluate(source, grid, pose, res, dtype=np.float32, key_dtype=None, rules=None):
    """-> score, g (6), H (6, 6), record {keys, hit (mask), dist (per point: the smallest distance of a coordinate from a voxel face, in units
    of the resolution), face (its minimum)}.  With a key_dtype other than dtype the keys (and which points are finite) come from the
    transformed positions formed in key_dtype from the same pose and points, everything else from those formed in dtype."""
    r = _rules(rules)
    kd = key_dtype or dtype
    vkeys, _, means, invs = grid
    s = np.asarray(source, np.float32).astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        p = apply(pose, s, dtype)
        pk = p if kd == dtype else apply(pose, np.asarray(source, np.float32).astype(kd), kd)
        R = rotation_matrix(np.asarray(pose, dtype)[:4], dtype)
        rs = np.stack([(R[i, 0] * s[:, 0] + R[i, 1] * s[:, 1]) + R[i, 2] * s[:, 2] for i in range(3)], axis=1).astype(dtype)
        ok = r["source_scores"](pk)
        u = r["key_arith"](np.where(ok[:, None], pk, kd(0.5) * kd(res)), kd(res))
        fl = r["floor"](u)
        keys = r["saturate"](fl).astype(np.int64)
        frac = u - fl
        dist = np.where(ok[:, None], np.minimum(frac, 1 - frac), 0.5).min(axis=1)      # per point, in units of the resolution
    face = float(dist.min())
    lo, hi = vkeys.min(axis=0), vkeys.max(axis=0)
    inside = ok & ((keys >= lo) & (keys <= hi)).all(axis=1)
    packed_v, packed_k, known = _ranks(vkeys, keys)             # ascending, as the voxels are
    inside &= known
    hit = np.zeros(len(s), bool)
    vox = np.zeros(len(s), np.int64)
    if inside.any():
        rank = packed_k[inside]
        pos = np.searchsorted(packed_v, rank)
        pos = np.minimum(pos, len(packed_v) - 1)
        found = packed_v[pos] == rank
        idx = np.nonzero(inside)[0]
        hit[idx[found]] = True
        vox[idx[found]] = pos[found]
    rec = {"keys": keys, "hit": hit, "face": face, "dist": dist}
    if not hit.any():
        return dtype(0), np.zeros(6, dtype), np.zeros((6, 6), dtype), rec
    p, rs, v = p[hit], rs[hit], vox[hit]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):     # a hit 10^9 from its voxel's mean: e = 0, huge finite terms
        return _sums(p, rs, means[v], invs[v], dtype) + (rec,)


def _sums(p, rs, mean, A, dtype):
    """score, g, H of the hit points: A (m, 3, 3) and mean (m, 3) are their voxels' """
    d = (p - mean).astype(dtype)
    c = np.stack([(A[:, r, 0] * d[:, 0] + A[:, r, 1] * d[:, 1]) + A[:, r, 2] * d[:, 2] for r in range(3)], axis=1).astype(dtype)
    e = np.exp(dtype(-0.5) * ((d[:, 0] * c[:, 0] + d[:, 1] * c[:, 1]) + d[:, 2] * c[:, 2])).astype(dtype)
    m = len(p)
    zero, one = np.zeros(m, dtype), np.ones(m, dtype)
    # J (3 x 6) by entries: [I | (0, -rs.z, rs.y), (rs.z, 0, -rs.x), (-rs.y, rs.x, 0)] as columns
    J = [[one, zero, zero, zero, rs[:, 2], -rs[:, 1]],
         [zero, one, zero, -rs[:, 2], zero, rs[:, 0]],
         [zero, zero, one, rs[:, 1], -rs[:, 0], zero]]
    gv = np.stack([(J[0][i] * c[:, 0] + J[1][i] * c[:, 1]) + J[2][i] * c[:, 2] for i in range(6)], axis=1).astype(dtype)
    T = [[(J[0][i] * A[:, 0, j] + J[1][i] * A[:, 1, j]) + J[2][i] * A[:, 2, j] for j in range(3)] for i in range(6)]     # J^T A
    Hc = np.stack([np.stack([(T[i][0] * J[0][j] + T[i][1] * J[1][j]) + T[i][2] * J[2][j] for j in range(6)], axis=1) for i in range(6)], axis=1).astype(dtype)
    score = np.cumsum(e, dtype=dtype)[-1]
    g = np.cumsum((e[:, None] * gv).astype(dtype), axis=0, dtype=dtype)[-1]
    H = np.cumsum((e[:, None, None] * Hc).astype(dtype), axis=0, dtype=dtype)[-1]
    return dtype(score), g.astype(dtype), H.astype(dtype)


# ---- the loop (:188-260) ----
def register(source, target, init=None, resolution=1.0, step_size=0.1, max_iterations=35, epsilon=1e-4, min_points_per_voxel=5, dtype=np.float32,
             grid=None, key_dtype=None, rules=None):
    """-> dict(pose, score, iterations, converged, n_voxels, n_hits, evals: the records of the evaluations, deltas: the applied updates)"""
    source = np.asarray(source, np.float32).reshape(-1, 3)
    target = np.asarray(target, np.float32).reshape(-1, 3)
    if len(source) == 0:
        raise NdtError("Source point cloud is empty")
    if len(target) < min_points_per_voxel:
        raise NdtError("Target point cloud has too few points for NDT voxel grid")
    if grid is None:
        grid = build(target, resolution, min_points_per_voxel, dtype, key_dtype, rules)
    if len(grid[0]) == 0:
        raise NdtError("NDT voxel grid is empty — try a larger resolution or lower min_points_per_voxel")
    pose = np.array(IDENTITY if init is None else init, dtype)
    out = {"converged": False, "iterations": 0, "score": dtype(0), "n_voxels": len(grid[0]), "n_hits": 0, "evals": [], "deltas": []}
    for it in range(max_iterations):
        out["iterations"] = it + 1
        score, g, H, rec = evaluate(source, grid, pose, resolution, dtype, key_dtype, rules)
        out["score"], out["n_hits"] = score, int(rec["hit"].sum())
        out["evals"].append(rec)
        delta = lu_solve(H + np.eye(6, dtype=dtype) * dtype(1e-6), -g, dtype)
        if delta is None:
            break
        norm = np.sqrt(np.cumsum(delta * delta, dtype=dtype)[-1])
        if norm > dtype(step_size):
            delta = (delta * (dtype(step_size) / norm)).astype(dtype)
        out["deltas"].append(delta)
        if np.sqrt(np.cumsum(delta * delta, dtype=dtype)[-1]) < dtype(epsilon):
            out["converged"] = True
            break
        pose = compose(euler_quaternion(delta[3], delta[4], delta[5], dtype), delta[:3], pose, dtype)
    out["pose"] = pose
    return out


def distances(a, b):
    """Frobenius distance of the two poses' 4 x 4 matrices, relative distance of the scores (b is the yardstick)"""
    fro = float(np.linalg.norm(matrix4(a["pose"] if isinstance(a, dict) else a[0]) - matrix4(b["pose"])))
    sa = float(a["score"] if isinstance(a, dict) else a[1])
    sb = float(b["score"])
    return fro, abs(sa - sb) / max(abs(sb), 1e-300)


# ---- inputs ----
START = np.array([0.03, 0.05, -0.04, 0.02])     # rotation angle (rad) about the axis (1, 2, 3) / |.|, translation


def start_pose():
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    q = np.r_[axis * np.sin(START[0] / 2), np.cos(START[0] / 2)]
    return np.r_[q, START[1:]].astype(np.float32)


def surface(n, seed, offset=(0.0, 0.0, 0.0)):
    """n points of the noisy sine surface over the 4 x 4 patch around `offset`"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-2.0, 2.0, (n, 2))
    z = 0.4 * np.sin(1.7 * xy[:, 0]) * np.cos(1.3 * xy[:, 1]) + 0.15 * xy[:, 0] + rng.normal(0.0, 0.01, n)
    return (np.c_[xy, z] + np.asarray(offset)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def surface_pair(nt, ns, res, min_points=5, seed=0, init=True, offset=(0.0, 0.0, 0.0), **loop):
    """(source, target, init) of the family: ns source points none of which, in any evaluation of the call described by `loop` (register()'s
    keywords; default one step), comes within 10 x FACE_MARGIN of a voxel face in the f64 run or has different keys in the f32 run.  Points that
    do are replaced by later points of the same sample (an input with a face crossing is replaced, not tolerated)."""
    target = surface(nt, 2 * seed + 1, offset)
    pool = surface(2 * ns + 64, 2 * seed + 2, offset)
    pose = start_pose() if init else IDENTITY.copy()
    if init and any(offset):
        # the start rotation turns about the patch's centre: about the origin it would carry a patch 2^10 away 40 units off, outside the
        # target's key box, and every such call would end with no hit.  t' = t + c - R c in f64, rounded once to the f32 pose both sides read
        c = np.asarray(offset, np.float64)
        pose[4:7] = (pose[4:7].astype(np.float64) + c - rotate(pose[:4], c, np.float64)).astype(np.float32)
    kw = dict(resolution=res, min_points_per_voxel=min_points, max_iterations=1)
    kw.update(loop)
    g32, g64 = build(target, res, min_points, np.float32), build(target, res, min_points, np.float64)
    for _ in range(40):
        src = pool[:ns]
        a = register(src, target, pose, dtype=np.float32, grid=g32, **kw)
        b = register(src, target, pose, dtype=np.float64, grid=g64, **kw)
        bad = np.zeros(ns, bool)
        for r in b["evals"]:
            bad |= r["dist"] < 10 * FACE_MARGIN
        for r32, r64 in zip(a["evals"], b["evals"]):
            bad |= (r32["keys"] != r64["keys"]).any(axis=1)
        if not bad.any():
            return src.copy(), target, pose
        pool = np.r_[pool[:ns][~bad], pool[ns:]]
        assert len(pool) >= ns, "the sample ran out of replacement points"
    raise AssertionError("no clean input found")
