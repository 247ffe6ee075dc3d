"""Checker for SHOT and USC descriptors: the rule of include/threecrate_hip_shot.h in numpy, for tests/test_shot_cpu.py,
tests/test_gpu_shot.py and tests/test_abi_shot.py.

Neighbour lists are tests/fpfh_checker.py's (the same rule: the f32 ball, below k the k + 1 nearest with the query dropped).  dv and dist are
float32 numpy operations, which round every operation and never fuse, so every decision on dist is the device's bit for bit.  arith="f64" is
the contract: the frame, the local coordinates and the normalisations in float64.  arith="f32" restates the reference's float32 sums (the
covariance summed in list order, float32 dots and atan2, float32 normalisation; numpy's eigh stands in for nalgebra's symmetric_eigen), so the
cost of the f64 deviation can be reported.

Per row: the descriptor, the integer counts, the frame, the flags and a MARGIN, the smallest of
  the relative eigen-gap (l1 - l2) / l1 (not for a zero covariance: the rule gives (1, 0, 0));
  |z . dv| / r and |e . dv| / r over the list (what the two votes and SHOT's elevation test);
  every binned neighbour's distance to an azimuth, USC elevation or SHOT cosine bin edge, in bins;
  |2 votes - len| for both votes (an even vote needs none: the rule resolves it, z stays and e takes the canonical sign);
  |length of the projection of e - 1e-10|;
  at an even vote on e only: the gap between the two largest |components| of e (what the canonical sign is read from);
  0 for a fallback list whose membership a distance tie decides.
A row is CLEAN at margin >= 1e-6.  f64 sums in another order differ by ~1e-15 relative and move the eigenvector by that over the gap, so by
at most ~1e-9 on a clean row: three orders inside the margin.  On clean rows the integer counts must therefore agree, descriptor entries are
two roundings of the same real number in [0, 1] (|a - b| <= 2^-23), and frames agree within 1e-6 per component."""
import numpy as np

from tests import fpfh_checker as FC

SHOT_DIM, USC_DIM = 352, 128
ROAD_BALL, ROAD_FALLBACK, ROAD_INERT, X_TIE, ZERO_COV, EMPTY = 0, 1, 2, 4, 8, 16
CLEAN = 1e-6
DESC_TOL, FRAME_TOL = 2.0 ** -23, 1e-6

# what a mutant changes one of (tests/test_shot_cpu.py); the first three are fpfh_checker.RULES'
RULES = dict(within=FC.RULES["within"], falls_back=FC.RULES["falls_back"], fallback_list=FC.RULES["fallback_list"],
             vote_z=True, vote_x=True, weight=lambda r, dist: np.maximum(r - dist, 0.0), votes_beyond=True, bins_beyond=False,
             inner=lambda dist, half: dist <= half, south=lambda lz: lz < 0, azimuth_pi=True,
             volume=lambda rb, eb, ab: rb * 16 + eb * 8 + ab, per_volume=True, l2=True,
             usc_bin=lambda ab, eb, rb: ab * 16 + eb * 4 + rb, usc_by_length=False)


def dim(variant):
    return {"shot": SHOT_DIM, "usc": USC_DIM}[variant]


def _sat(t, n):
    """min((usize)t, n - 1), saturating: NaN and negative values give 0"""
    t = np.asarray(t, np.float64)
    b = np.zeros(t.shape, np.int64)
    with np.errstate(invalid="ignore"):
        m = t > 0
    b[m] = np.minimum(t[m], n - 1).astype(np.int64)
    return b


def _edge(t, lo, hi):
    """distance of t to the nearest integer edge in [lo, hi], in bins; inf without t"""
    t = np.asarray(t, np.float64)
    t = t[np.isfinite(t)]
    if not len(t):
        return np.inf
    e = np.clip(np.round(t), lo, hi)
    return float(np.abs(t - e).min())


def _unit(v, T):
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], dtype=T)


def _row(pos, nrm, i, lst, r, variant, T, rules):
    """one point with a non-empty list -> counts, frame (9,), flag bits, margin, and what normalisation needs"""
    f32 = np.float32
    with np.errstate(all="ignore"):
        dv32 = pos[lst] - pos[i][None, :]
        dist32 = np.sqrt((dv32[:, 0] * dv32[:, 0] + dv32[:, 1] * dv32[:, 1]) + dv32[:, 2] * dv32[:, 2])
        dv, dist, L = dv32.astype(T), dist32.astype(T), len(lst)
        voters = np.ones(L, bool) if rules["votes_beyond"] else ~(dist32 > r)
        n = nrm[i]
        z = np.array([0, 0, 1], T)
        if np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) > f32(1e-10):
            z = _unit(n.astype(T), T)
        dot = lambda a, d: (a[0] * d[:, 0] + a[1] * d[:, 1]) + a[2] * d[:, 2]
        zd = dot(z, dv)
        vz = int((zd[voters] >= 0).sum())
        if rules["vote_z"] and 2 * vz < voters.sum():
            z = -z
        w = rules["weight"](T(r), dist).astype(T)
        terms = np.stack([w * dv[:, 0] * dv[:, 0], w * dv[:, 0] * dv[:, 1], w * dv[:, 0] * dv[:, 2], w * dv[:, 1] * dv[:, 1], w * dv[:, 1] * dv[:, 2],
                          w * dv[:, 2] * dv[:, 2]], 1)
        c = np.cumsum(terms, axis=0, dtype=T)[-1] if T is f32 else terms.sum(axis=0)
        flags, gap = 0, np.inf
        if not (c[0] + c[3]) + c[5] > 0:
            flags |= ZERO_COV
            e = np.array([1, 0, 0], np.float64)
        else:
            lam, vec = np.linalg.eigh(np.array([[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]], np.float64))
            e = vec[:, 2]
            gap = (lam[2] - lam[1]) / lam[2]
        a = np.abs(e)
        lead = int(np.argmax(a))                                # the first of equal magnitudes
        if e[lead] < 0:
            e = -e
        e = e.astype(T)
        ed = dot(e, dv)
        vx = int((ed[voters] >= 0).sum())
        tie = 2 * vx == voters.sum()
        if tie:
            flags |= X_TIE
        flip = rules["vote_x"] and 2 * vx < voters.sum()
        # x with the canonical sign
        proj = e - z * ((z[0] * e[0] + z[1] * e[1]) + z[2] * e[2])
        plen = np.sqrt((proj[0] * proj[0] + proj[1] * proj[1]) + proj[2] * proj[2])
        projected = bool(plen > 1e-10)
        if not projected:
            proj = np.array([1, 0, 0], T) - z * z[0]
            if not np.sqrt((proj[0] * proj[0] + proj[1] * proj[1]) + proj[2] * proj[2]) > 1e-10:
                proj = np.array([0, 1, 0], T) - z * z[1]
        x = _unit(proj, T)
        y = np.array([z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]], T)
        binned = ~(dist32 < f32(1e-10))
        if not rules["bins_beyond"]:
            binned &= ~(dist32 > r)
        d, ds = dv[binned], dist[binned]
        lx, ly, lz = dot(x, d), dot(y, d), dot(z, d)
        pi = T(np.pi)
        az = (np.arctan2(ly, lx) + (pi if rules["azimuth_pi"] else T(0))) / (T(2) * pi) * T(8)
        ab = _sat(az, 8)
        shift = 4 if (flip and projected) else 0
        ab = (ab - shift) % 8                                   # what sat in canonical sector s is read out in sector s - 4
        margin = min(gap, _edge(az, 0, 8))
        if variant == "usc":
            te = (np.clip(lz / ds, -1, 1) - T(-1)) / (T(1) - T(-1)) * T(4)
            rb = _sat((dist32[binned] / r * f32(4)).astype(np.float64), 4)
            counts = np.bincount(rules["usc_bin"](ab, _sat(te, 4), rb), minlength=USC_DIM)
            margin = min(margin, _edge(te, 1, 3))
        else:
            rb = np.where(rules["inner"](dist32[binned], r * f32(0.5)), 0, 1)
            eb = np.where(rules["south"](lz), 0, 1)
            nj = nrm[lst][binned].astype(T)
            tc = (np.clip(dot(z, nj), -1, 1) - T(-1)) / (T(1) - T(-1)) * T(11)
            counts = np.bincount(rules["volume"](rb, eb, ab) * 11 + _sat(tc, 11), minlength=SHOT_DIM)
            margin = min(margin, _edge(tc, 1, 10))
        if flip and projected:
            x, y = -x, -y
        r64 = float(r)
        margin = min(margin, float(np.abs(zd).min()) / r64, float(np.abs(ed).min()) / r64, abs(float(plen) - 1e-10))
        if 2 * vz != L:
            margin = min(margin, abs(2 * vz - L))
        if not tie:
            margin = min(margin, abs(2 * vx - L))
        else:
            s = np.sort(a)
            margin = min(margin, s[2] - s[1])
    return counts, np.concatenate([x, y, z]).astype(f32), flags, float(margin), int(binned.sum()), L


def _normalise(counts, variant, n_binned, L, T, rules):
    v = counts.astype(T)
    with np.errstate(all="ignore"):
        if variant == "usc":
            total = L if rules["usc_by_length"] else n_binned
            if total:
                v = v / T(total)
        elif rules["per_volume"]:
            tot = counts.reshape(32, 11).sum(axis=1)
            v = np.where(np.repeat(tot, 11) > 0, v / np.repeat(np.maximum(tot, 1), 11).astype(T), T(0))
        if rules["l2"]:
            norm = np.sqrt(np.sum(v * v, dtype=T))
            if norm > 1e-10:
                v = v / norm
    return v.astype(np.float32)


def describe(np6, radius, k, variant="shot", arith="f64", rows=None, rules=None):
    """-> dict(rows, desc (m, dim) f32, counts (m, dim) i64, lrf (m, 9) f32, flags (m,) u32, margin (m,), clean (m,) bool, length (m,))"""
    rules = dict(RULES, **(rules or {}))
    T = {"f64": np.float64, "f32": np.float32}[arith]
    np6 = np.ascontiguousarray(np6, np.float32).reshape(-1, 6)
    pos, nrm = np.ascontiguousarray(np6[:, :3]), np.ascontiguousarray(np6[:, 3:])
    r = np.float32(radius)
    nb = FC.Neighbours(pos, r, k, rows, {q: rules[q] for q in ("within", "falls_back", "fallback_list")})
    m, D = len(nb.rows), dim(variant)
    out = dict(rows=nb.rows, desc=np.zeros((m, D), np.float32), counts=np.zeros((m, D), np.int64), lrf=np.zeros((m, 9), np.float32),
               flags=np.zeros(m, np.uint32), margin=np.full(m, np.inf), length=np.zeros(m, np.int64))
    fin = np.all(np.isfinite(pos), axis=1)
    r2 = r * r
    others = np.flatnonzero(fin)
    for s, i in enumerate(nb.rows):
        if not fin[i]:
            out["flags"][s] = ROAD_INERT
            continue
        lst = nb.lists[s]
        # the road: the ball when it holds at least k points (the list IS the ball then)
        ball = int(rules["within"](FC.d2_f32(pos[others[others != i]], pos[i][None, :]), r2).sum())
        road = ROAD_FALLBACK if rules["falls_back"](ball, k) else ROAD_BALL
        out["length"][s] = len(lst)
        if not len(lst):
            out["flags"][s] = road | EMPTY
            continue
        counts, lrf, fl, margin, n_binned, L = _row(pos, nrm, i, lst, r, variant, T, rules)
        out["counts"][s], out["lrf"][s], out["flags"][s] = counts, lrf, road | fl
        out["margin"][s] = 0.0 if nb.tie[s] else margin
        out["desc"][s] = _normalise(counts, variant, n_binned, L, T, rules)
    out["clean"] = out["margin"] >= CLEAN
    return out


def compare(got_desc, got_lrf, got_flags, want):
    """the device's rows against describe()'s on the same rows -> list of complaints (empty: equal within the derived tolerances).
    Flags agree exactly on every row; clean rows are held to DESC_TOL and FRAME_TOL; every row is finite, >= 0 and of unit norm or zero."""
    bad = []
    g, w = np.asarray(got_desc, np.float64), want["desc"].astype(np.float64)
    if not np.array_equal(np.asarray(got_flags).astype(np.uint32), want["flags"]):
        bad.append(("flags", np.flatnonzero(np.asarray(got_flags).astype(np.uint32) != want["flags"])[:10].tolist()))
    c = want["clean"]
    if c.any():
        worst = np.abs(g[c] - w[c]).max(axis=1)
        if worst.max() > DESC_TOL:
            bad.append(("desc", want["rows"][c][worst > DESC_TOL][:10].tolist(), float(worst.max())))
        fw = np.abs(np.asarray(got_lrf, np.float64)[c] - want["lrf"][c].astype(np.float64)).max(axis=1)
        if fw.max() > FRAME_TOL:
            bad.append(("lrf", want["rows"][c][fw > FRAME_TOL][:10].tolist(), float(fw.max())))
    bad += invariants(got_desc)
    return bad


def invariants(desc):
    g = np.asarray(desc, np.float64)
    bad = []
    if not np.all(np.isfinite(g)) or (g < 0).any():
        bad.append(("finite and >= 0",))
    norm = np.sqrt((g * g).sum(axis=1))
    ok = (np.abs(norm - 1.0) <= 1e-6) | (norm == 0.0)
    if not ok.all():
        bad.append(("unit norm or zero", np.flatnonzero(~ok)[:10].tolist()))
    return bad
