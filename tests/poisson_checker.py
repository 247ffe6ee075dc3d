"""The contract of include/threecrate_hip_poisson.h in numpy, step by step in the header's order (test infrastructure; no GPU).
mode="exact": steps 2-5 and 7 with the header's f32 / f64 rules (every f32 operation is one numpy f32 operation; the splat sums run in
f64 in input order through np.add.at); the conjugate gradient keeps f32 vectors and f64 inner products, whose ORDER is numpy's, not the
device's: the loop's values agree with the device to the last bits of an f64 sum, not bit for bit.  mode="f64": everything after the
splat in f64 (the yardstick for chi and the iso value).  rules: the mutants of tests/test_poisson_cpu.py, each a wrong reading of one
sentence of the header."""
import numpy as np

F, D = np.float32, np.float64
MUTANTS = ("weights_assoc", "no_upper_clamp", "div_sign", "one_sided", "neumann", "iso_grid_mean", "no_screen", "reverse_order")
DEFAULTS = dict(depth=6, scale=1.1, point_weight=0.0, max_iterations=200, tolerance=1e-5, min_density=0.0)


def config(**kw):
    c = dict(DEFAULTS)
    c.update(kw)
    return c


def check(points, normals, cfg):
    """the header's checks in order: None, or the words of the failure"""
    n = len(points)
    if n == 0:
        return "Point cloud is empty"
    if n < 10:
        return "Point cloud too small"
    if not 2 <= cfg["depth"] <= 8:
        return "depth"
    if not (F(cfg["scale"]) >= 1 and np.isfinite(F(cfg["scale"]))):
        return "scale"
    if not all(F(cfg[k]) >= 0 for k in ("point_weight", "tolerance", "min_density")):
        return "negative"
    p, q = np.asarray(points, F), np.asarray(normals, F)
    if not np.isfinite(p).all():
        return "not finite"
    with np.errstate(all="ignore"):
        mag = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        if not ((mag >= F(1e-6)) & (np.abs(mag - F(1.0)) <= F(0.1))).all():
            return "Invalid normal"
    if not (p.max(0) - p.min(0)).max() > 0:
        return "no extent"
    return None


def grid_of(points, depth, scale):
    """step 2 -> origin (3,) f32, h f32, N"""
    p = np.asarray(points, F)
    mn, mx = p.min(0), p.max(0)
    N = 1 << depth
    side = F(scale) * (mx - mn).max()
    h = side / F(N - 1)
    origin = F(0.5) * (mn + mx) - F(0.5) * side
    return origin.astype(F), F(h), N


def cells(points, origin, h, N, rules=()):
    """step 3 -> i (n, 3) int64, f (n, 3) f32"""
    g = (np.asarray(points, F) - origin) / h
    top = N - 1 if "no_upper_clamp" in rules else N - 2
    i = np.where(g >= 0, np.minimum(np.floor(g), top), 0).astype(np.int64)
    return i, (g - i.astype(F)).astype(F)


def corner_weights(i, f, N, rules=()):
    """-> node (n, 8) int64 (x fastest), w (n, 8) f32; corner c = (c & 1, (c >> 1) & 1, c >> 2)"""
    one = F(1.0)
    node, w = np.empty((len(i), 8), np.int64), np.empty((len(i), 8), F)
    for c in range(8):
        up = (c & 1, (c >> 1) & 1, c >> 2)
        wk = [f[:, k] if up[k] else one - f[:, k] for k in range(3)]
        w[:, c] = wk[0] * (wk[1] * wk[2]) if "weights_assoc" in rules else (wk[0] * wk[1]) * wk[2]
        x, y, z = (np.minimum(i[:, k] + up[k], N - 1) for k in range(3))           # (the minimum acts only under no_upper_clamp)
        node[:, c] = (z * N + y) * N + x
    return node, w


def splat(normals, node, w, N, rules=()):
    """-> V (3, N^3) f32, W (N^3,) f32: f64 sums in input order, rounded once"""
    q = np.asarray(normals, F).astype(D)
    order = slice(None, None, -1) if "reverse_order" in rules else slice(None)
    nd, w64 = node[order].reshape(-1), w[order].astype(D).reshape(-1)
    W = np.zeros(N ** 3, D)
    np.add.at(W, nd, w64)
    V = np.zeros((3, N ** 3), D)
    for k in range(3):
        np.add.at(V[k], nd, w64 * np.repeat(q[order][:, k], 8))
    return V.astype(F), W.astype(F)


def _shift(a, axis, step, fill_self=False):
    """a's neighbour at +step along axis (a is [z, y, x]); outside the grid 0, or the node itself"""
    out = a.copy() if fill_self else np.zeros_like(a)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    if step > 0:
        src[axis], dst[axis] = slice(1, None), slice(None, -1)
    else:
        src[axis], dst[axis] = slice(None, -1), slice(1, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def rhs(V, h, N, rules=(), dtype=F):
    """step 4 -> b (N^3,)"""
    v = [V[k].astype(dtype).reshape(N, N, N) for k in range(3)]
    one = "one_sided" in rules
    d = [_shift(v[k], 2 - k, +1, one) - _shift(v[k], 2 - k, -1, one) for k in range(3)]      # axis 2 is x
    c = dtype(0.5 if "div_sign" in rules else -0.5) * dtype(h)
    return (c * ((d[0] + d[1]) + d[2])).reshape(-1)


def apply_A(p, W, pw, N, rules=()):
    """step 5, in p's dtype"""
    t = p.dtype.type
    a = p.reshape(N, N, N)
    nm = "neumann" in rules
    S = ((((_shift(a, 2, -1, nm) + _shift(a, 2, +1, nm)) + _shift(a, 1, -1, nm)) + _shift(a, 1, +1, nm)) + _shift(a, 0, -1, nm)) + _shift(a, 0, +1, nm)
    out = (t(6.0) * a - S).reshape(-1)
    if pw > 0 and "no_screen" not in rules:
        out = out + (t(pw) * W.astype(t)) * p
    return out


def solve(b, W, cfg, N, rules=()):
    """step 6 in b's dtype -> chi, iterations, rel_residual (f64, the recurrence's), history of rel"""
    t = b.dtype.type
    dot = lambda u, v: float(np.dot(u.astype(D), v.astype(D)))
    chi, r, p = np.zeros_like(b), b.copy(), np.zeros_like(b)
    bb = dot(b, b)
    rr, beta, it, rel, hist = bb, t(0.0), 0, (0.0 if bb == 0 else 1.0), []
    if bb == 0:
        return chi, 0, 0.0, hist
    pw, tol = float(F(cfg["point_weight"])), float(F(cfg["tolerance"]))
    while it < cfg["max_iterations"]:
        p = r + beta * p
        q = apply_A(p, W, pw, N, rules)
        pq = dot(p, q)
        if not pq > 0:
            break
        alpha = t(rr / pq)
        chi = chi + alpha * p
        r = r - alpha * q
        rr2 = dot(r, r)
        it += 1
        rel = float(np.sqrt(rr2 / bb))
        hist.append(rel)
        if rel <= tol:
            break
        beta, rr = t(rr2 / rr), rr2
    return chi, it, rel, hist


def iso_of(chi, node, w, rules=()):
    """step 7, in f64 from chi's values"""
    if "iso_grid_mean" in rules:
        return float(chi.astype(D).mean())
    s = np.zeros(len(node), D)
    c64 = chi.astype(D)
    for c in range(8):
        s = s + w[:, c].astype(D) * c64[node[:, c]]
    total = np.zeros(1, D)
    np.add.at(total, np.zeros(len(s), np.int64), s)             # input order
    return float(total[0] / D(len(s)))


def run(points, normals, cfg, mode="exact", rules=()):
    """-> dict: origin, h, N, node, w, V, W (density), occupied_nodes, b, chi, iterations, rel_residual, history, iso_value (all of `mode`)"""
    rules = tuple(rules)
    assert set(rules) <= set(MUTANTS) and mode in ("exact", "f64")
    origin, h, N = grid_of(points, cfg["depth"], cfg["scale"])
    i, f = cells(points, origin, h, N, rules)
    node, w = corner_weights(i, f, N, rules)
    V, W = splat(normals, node, w, N, rules)
    dtype = F if mode == "exact" else D
    b = rhs(V, h, N, rules, dtype)
    chi, it, rel, hist = solve(b, W.astype(dtype), cfg, N, rules)
    iso = iso_of(chi, node, w, rules)
    return dict(origin=origin, h=h, N=N, cell=i, frac=f, node=node, w=w, V=V, W=W, occupied_nodes=int((W > 0).sum()), b=b, chi=chi, iterations=it,
                rel_residual=rel, history=hist, iso_value=F(iso) if mode == "exact" else iso)


def true_residual(chi, b, W, pw, N):
    """|| b - A chi || / || b || in f64 from any chi"""
    c, b64 = np.asarray(chi, D).reshape(-1), np.asarray(b, D).reshape(-1)
    r = b64 - apply_A(c, np.asarray(W, D), float(F(pw)), N)
    return float(np.sqrt(np.dot(r, r) / np.dot(b64, b64)))


def rel_max(a, ref):
    """relative max-norm distance"""
    a, ref = np.asarray(a, D).reshape(-1), np.asarray(ref, D).reshape(-1)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


# ---- mesh properties (a welded mesh: vertices (n, 3), faces (m, 3)) ----
def edge_counts(faces):
    f = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return counts


def is_closed(faces):
    return bool((edge_counts(faces) == 2).all())


def euler(vertices, faces):
    return len(vertices) - len(edge_counts(faces)) + len(faces)


def signed_volume(vertices, faces):
    v, f = np.asarray(vertices, D), np.asarray(faces, np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
