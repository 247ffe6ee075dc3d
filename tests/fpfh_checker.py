"""Checker for FPFH descriptors (features.rs:38-259), shared by test_fpfh_cpu.py, test_gpu_fpfh.py and the edge
cases (fpfh_cases.py, test_fpfh_edges_cpu.py, test_gpu_fpfh_edges.py).

Neighbours of i: every finite j != i with d2 <= r * r, d2 = dx*dx + dy*dy + dz*dz in float32 left to right (cKDTree with a widened
radius, then filtered by the f32 relation), ordered by (d2, index) like the kd-tree's sorted result; fewer than k of them: the k + 1
nearest by (f32 d2, index), i removed, truncated to k.  Points whose k-th and (k + 1)-th candidates tie are flagged (`tie`): the
set depends on the tie order, and the row is held to a widened L1 bound (below).

Pair features run in float32 numpy arrays, which round every operation and never fuse.  Every 3-term dot product is
a0*b0 + a1*b1 + a2*b2, left to right, with no leading zero (the kernel's form; nalgebra's, as far as can be told without its source).
The same pairs are computed again in float64; a pair is *ambiguous* when an f32 bin differs from the f64 bin, when the f64 theta
bin coordinate lies within 2e-6 of an interior bin edge (atan2f differs by an ulp or two between libraries: ~4e-7 there; alpha and
phi are the same f32 operations on both sides), or when |n_s x d| < 1e-3 (an ill-conditioned frame).

Summation bound: a descriptor bin is (s_i + (1/W) sum_j w_j s_j) / S with f32 sums over the list in the list's order; the device
sums in its own order.  Values are in [0, 1], so the difference is a few ulps times sqrt(list length) in practice: 1e-5 on
unambiguous points.  Moving one count of an ambiguous pair changes one sub-histogram of SPFH(x) by at most
2 / valid(x) in L1; the renormalised descriptor of i mixes SPFH(i) with a convex combination of its neighbours' SPFH, so each
sub-histogram moves by at most 2 * max over x in {i} + N(i) of amb(x) / valid(x) (ambiguous_l1_bound)."""
import numpy as np

BINS = 11
DIM = 33
PI32 = np.float32(np.pi)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def d2_f32(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return dx * dx + dy * dy + dz * dz


def to_bin(x, lo, hi):
    """features.rs:74-78 with Rust's saturating `as usize`: NaN and negative -> 0, then min(10)"""
    x = np.asarray(x)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (x - lo) / (hi - lo) * x.dtype.type(BINS)
    b = np.zeros(t.shape, np.int64)
    m = t > 0
    b[m] = np.minimum(t[m], BINS - 1).astype(np.int64)
    return b, t


def pair_features(ps, ns, pt, nt, lead_zero=False):
    """compute_pair_features, vectorised, in the dtype of the inputs -> (valid, alpha, phi, theta, |v|).  lead_zero: the dot
    products of theta summed from a leading +0 instead (the form this backend assumes nalgebra does NOT use; the tests show that
    the two forms give different bins, so the assumption is pinned)"""
    with np.errstate(all="ignore"):
        dx, dy, dz = pt[:, 0] - ps[:, 0], pt[:, 1] - ps[:, 1], pt[:, 2] - ps[:, 2]
        dist = np.sqrt(dx * dx + dy * dy + dz * dz)
        valid = ~(dist < 1e-10)
        d0, d1, d2 = dx / dist, dy / dist, dz / dist
        nx, ny, nz = ns[:, 0], ns[:, 1], ns[:, 2]
        vx, vy, vz = ny * d2 - nz * d1, nz * d0 - nx * d2, nx * d1 - ny * d0
        vm = np.sqrt(vx * vx + vy * vy + vz * vz)
        valid &= ~(vm < 1e-10)
        ux, uy, uz = vx / vm, vy / vm, vz / vm
        wx, wy, wz = ny * uz - nz * uy, nz * ux - nx * uz, nx * uy - ny * ux
        tx, ty, tz = nt[:, 0], nt[:, 1], nt[:, 2]
        alpha = ux * tx + uy * ty + uz * tz
        phi = nx * d0 + ny * d1 + nz * d2
        if lead_zero:
            z = ps.dtype.type(0)
            theta = np.arctan2(((z + wx * tx) + wy * ty) + wz * tz, ((z + nx * tx) + ny * ty) + nz * tz)
        else:
            theta = np.arctan2(wx * tx + wy * ty + wz * tz, nx * tx + ny * ty + nz * tz)
    return valid, alpha, phi, theta, vm


def pair_bins(ps, ns, pt, nt, lead_zero=False):
    """-> (valid, bins (m, 3) with offsets 0 / 11 / 22, ambiguous)"""
    valid, a, p, t, _ = pair_features(_f32(ps), _f32(ns), _f32(pt), _f32(nt), lead_zero)
    one = np.float32(1)
    ba, _ = to_bin(a, -one, one)
    bp, _ = to_bin(p, -one, one)
    bt, _ = to_bin(t, -PI32, PI32)
    v64, a64, p64, t64, vm64 = pair_features(*(np.asarray(x, np.float64) for x in (ps, ns, pt, nt)))
    amb = (v64 != valid) | (vm64 < 1e-3)
    for b32, x64, lo, hi, edge in ((ba, a64, -1.0, 1.0, 0.0), (bp, p64, -1.0, 1.0, 0.0), (bt, t64, -np.pi, np.pi, 2e-6)):
        b64, c64 = to_bin(x64, lo, hi)
        with np.errstate(invalid="ignore"):
            near = (np.abs(c64 - np.round(c64)) < edge) & (np.round(c64) >= 1) & (np.round(c64) <= BINS - 1)
        amb |= (b64 != b32) | near
    amb &= valid | v64
    return valid, np.stack([ba, BINS + bp, 2 * BINS + bt], 1), amb


# The rules a mutant changes one of (test_fpfh_edges_cpu.py): which candidates are in the ball, when a point falls back, what the
# fallback keeps of the candidates sorted by (d2, index), the weight of a neighbour at distance dist, what counts as a valid pair,
# what the weighted sum is divided by
RULES = dict(within=lambda d2, r2: d2 <= r2, falls_back=lambda cnt, k: cnt < k,
             fallback_list=lambda cc, i, k: cc[: k + 1][cc[: k + 1] != i][:k], weight=lambda dist: np.float32(1) / dist,
             count_skipped=False, divide_by_length=False, lists_hook=None)


class Neighbours:
    """CSR neighbour lists of the requested rows (all points by default): rows[s], ptr, idx (list order), tie flags"""

    def __init__(self, pos, radius, k, rows=None, rules=None, tree=None):
        rules = dict(RULES, **(rules or {}))
        pos = _f32(pos)
        n = len(pos)
        self.n = n
        fin = np.all(np.isfinite(pos), axis=1)
        rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
        self.rows = rows
        r2 = np.float32(radius) * np.float32(radius)
        fidx = np.nonzero(fin)[0]
        ball = bool(r2 <= r2)
        lists, ties = [], np.zeros(len(rows), bool)
        cand, ci = None, 0
        if len(fidx):
            if tree is None:
                from scipy.spatial import cKDTree
                tree = cKDTree(pos[fidx].astype(np.float64))
            if ball and np.isfinite(r2):
                # widened by the rounding of the f32 differences, which goes with the coordinates of the QUERY and of points within
                # the radius of it (one far outlier must not put the whole cloud into every ball)
                q = pos[rows[fin[rows]]].astype(np.float64)
                r = float(np.sqrt(np.float64(r2)))
                rw = r * (1.0 + 1e-5) + 8.0 * 2.0 ** -24 * (np.abs(q).max(axis=1, initial=0.0) + r)
                cand = tree.query_ball_point(q, rw) if len(q) else []
        for s, i in enumerate(rows):
            if not fin[i]:
                lists.append(np.zeros(0, np.int64))
                continue
            within = np.zeros(0, np.int64)
            if ball:
                if cand is not None:
                    c = fidx[np.asarray(cand[ci], np.int64)]
                    ci += 1
                else:
                    c = fidx
                c = c[c != i]
                d2 = d2_f32(pos[c], pos[i][None, :])
                keep = rules["within"](d2, r2)
                c, d2 = c[keep], d2[keep]
                within = c[np.lexsort((c, d2))]
            if not rules["falls_back"](len(within), k):
                lists.append(within)
                continue
            m = min(len(fidx), k + 8)
            _, cc = tree.query(pos[i].astype(np.float64), m)
            cc = fidx[np.atleast_1d(cc)]
            d2 = d2_f32(pos[cc], pos[i][None, :])
            o = np.lexsort((cc, d2))
            cc, d2 = cc[o], d2[o]
            first = cc[: k + 1]
            lists.append(rules["fallback_list"](cc, i, k))
            # the set is decided by the tie order when the (k + 1)-th and (k + 2)-th candidates tie, or when i itself is not among
            # the first k + 1 (more than k duplicates of it) and the k-th and (k + 1)-th tie
            if len(d2) > k + 1 and (d2[k] == d2[k + 1] or (i not in first and d2[k - 1] == d2[k])):
                ties[s] = True
        self.lists = lists
        self.tie = ties
        self.tree = tree


def fpfh(pos, nrm, radius, k, rows=None, lead_zero=False, rules=None):
    """-> dict(desc (len(rows), 33) f32, amb_pairs, pairs, strict (bool per row), bound (L1 bound per sub-histogram), tie)
    for the given rows (default: all).  Needs the SPFH of the rows' neighbours too, so their lists are computed as well."""
    pos, nrm = _f32(pos), _f32(nrm)
    n = len(pos)
    rows = np.arange(n) if rows is None else np.asarray(rows, np.int64)
    rules = dict(RULES, **(rules or {}))
    first = Neighbours(pos, radius, k, rows, rules)
    if rules["lists_hook"]:                                          # a mutant that hands a row another row's list
        first.lists = rules["lists_hook"](first.lists)
    need = np.unique(np.concatenate([rows] + [l for l in first.lists])) if len(rows) else rows
    nb = first if len(need) == len(rows) and np.array_equal(need, rows) else Neighbours(pos, radius, k, need, rules, first.tree)
    # SPFH of every needed point
    m = len(need)
    lens = np.array([len(l) for l in nb.lists], np.int64)
    src = np.repeat(np.arange(m), lens)
    dst = np.concatenate(nb.lists) if m and lens.sum() else np.zeros(0, np.int64)
    srcp = need[src]
    valid, bins, amb = pair_bins(pos[srcp], nrm[srcp], pos[dst], nrm[dst], lead_zero)
    counts = np.zeros((m, DIM), np.int64)
    for c in range(3):
        np.add.at(counts, (src[valid], bins[valid, c]), 1)
    nvalid = np.bincount(src if rules["count_skipped"] else src[valid], minlength=m)
    namb = np.bincount(src[amb], minlength=m)
    scale = np.where(nvalid > 0, np.float32(1) / np.maximum(nvalid, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    spfh = counts.astype(np.float32) * scale[:, None]
    # FPFH of the requested rows, summed in list order
    r = len(rows)
    pos_of = np.full(n, -1, np.int64)
    pos_of[need] = np.arange(m)
    srow = pos_of[rows]
    rl = np.array([len(l) for l in first.lists], np.int64)
    flat = np.concatenate(first.lists) if r and rl.sum() else np.zeros(0, np.int64)
    ptr = np.concatenate([[0], np.cumsum(rl)])
    desc = spfh[srow].copy()
    acc = np.zeros((r, DIM), np.float32)
    wsum = np.zeros(r, np.float32)
    for t in range(int(rl.max()) if r else 0):
        sel = np.nonzero(rl > t)[0]
        j = flat[ptr[sel] + t]
        d = d2_f32(pos[j], pos[rows[sel]])
        dist = np.sqrt(d)
        ok = ~(dist < 1e-10)
        sel, j, dist = sel[ok], j[ok], dist[ok]
        w = rules["weight"](dist)
        wsum[sel] = wsum[sel] + (np.float32(1) if rules["divide_by_length"] else w)
        acc[sel] = acc[sel] + w[:, None] * spfh[pos_of[j]]
    has = (rl > 0) & (wsum > 0)
    inv = np.zeros(r, np.float32)
    inv[has] = np.float32(1) / wsum[has]
    desc[has] = desc[has] + inv[has, None] * acc[has]
    for part in range(3):
        sl = slice(part * BINS, (part + 1) * BINS)
        s = np.zeros(r, np.float32)
        for b in range(part * BINS, (part + 1) * BINS):
            s = s + desc[:, b]
        div = has & (s > 0)
        desc[div, sl] = desc[div, sl] / s[div, None]
    # ambiguity of each requested row: its own pairs and its neighbours'
    frac = np.where(nvalid > 0, namb / np.maximum(nvalid, 1), (namb > 0).astype(np.float64))
    seg = np.repeat(np.arange(r), rl)
    mem = pos_of[flat]
    tie = nb.tie[srow] | (np.bincount(seg, weights=nb.tie[mem].astype(np.float64), minlength=r) > 0)
    ambsum = namb[srow] + np.bincount(seg, weights=namb[mem].astype(np.float64), minlength=r)
    strict = ~tie & (ambsum == 0)
    fmax = frac[srow].copy()
    np.maximum.at(fmax, seg, frac[mem])
    bound = 2.0 * fmax + 1e-5
    # a tied row may hold another neighbour at the tied distance.  That neighbour is the farthest of the list, so its weight is at
    # most 1 / len(list) of the total; the own SPFH moves by at most 2 / valid in L1 per sub-histogram, 4 / valid if the swapped
    # pair is a skipped one.  A tied neighbour j moves SPFH(j) by at most 4 / valid(j).
    inv_valid = 1.0 / np.maximum(nvalid, 1)
    tmax = np.where(nb.tie[srow], inv_valid[srow], 0.0)
    np.maximum.at(tmax, seg, np.where(nb.tie[mem], inv_valid[mem], 0.0))
    bound = bound + np.where(tie, 4.0 * tmax + np.where(nb.tie[srow], 2.0 / np.maximum(rl, 1), 0.0), 0.0)
    return dict(desc=desc, strict=strict, bound=bound, tie=tie, pairs=nvalid[srow], amb=namb[srow],
                nlist=rl)


def compare(got, ref, tol=1e-5, min_strict=None):
    """The parity rule of test_gpu_fpfh.py: strict rows bin by bin within tol; every other row (ambiguous pairs, ties) within its
    L1 bound per sub-histogram.  Returns the fraction of strict rows."""
    got = np.asarray(got, np.float32)
    desc, strict, bound = ref["desc"], ref["strict"], ref["bound"]
    assert got.shape == desc.shape, (got.shape, desc.shape)
    diff = np.abs(got.astype(np.float64) - desc.astype(np.float64))
    if strict.any():
        worst = diff[strict].max()
        bad = np.nonzero(strict & (diff.max(1) > tol))[0]
        assert worst <= tol, (float(worst), bad[:10].tolist())
    loose = ~strict
    for part in range(3):
        l1 = diff[:, part * BINS:(part + 1) * BINS].sum(1)
        bad = np.nonzero(loose & (l1 > bound))[0]
        assert len(bad) == 0, (part, bad[:10].tolist(), l1[bad[:10]].tolist(), bound[bad[:10]].tolist())
    frac = float(strict.mean()) if len(strict) else 1.0
    if min_strict is not None:
        assert frac >= min_strict, frac
    return frac


def two_walls():
    """two 6 x 6 walls facing each other: x = 0 with normal +x, and the same lattice moved by (0.05, 0.05, 0) with normal -x"""
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * np.float32(0.1)
    a = np.concatenate([np.zeros((36, 1), np.float32), g], 1)
    pos = np.concatenate([a, a + np.array([[0.05, 0.05, 0]], np.float32)])
    nrm = np.concatenate([np.tile([[1, 0, 0]], (36, 1)), np.tile([[-1, 0, 0]], (36, 1))]).astype(np.float32)
    return pos, nrm
