"""The contract of descriptor matching and RANSAC over correspondences (include/threecrate_hip_global.h; the two device steps of
threecrate-algorithms/src/global_registration.rs) restated with numpy: every f32 operation of the header in the header's order, the
three-pair model in f64 through numpy.linalg.svd, the winner as the literal sequential loop with its break.  The inputs of
tests/test_gpu_global.py are built here, so that tests/test_global_cpu.py can prove on the checker alone what each of them is for.
Mutants: a named wrong rule, for the table that shows which inputs tell it apart."""
import numpy as np

F = np.float32
DIM = 33
# the constants of csrc/global.hip that the size lists name (tests/test_global_cpu.py compares them with the source text)
MATCH_SRC_PER_BLOCK, MATCH_TGT_TILE, PAIRS_PER_BLOCK, CAND_TILE, CHUNK = 128, 128, 1024, 128, 4096
MAX_ITERS = 1 << 20
LCG_MULT, LCG_INC, GOLDEN, MASK = 6364136223846793005, 1442695040888963407, 0x9E3779B97F4A7C15, (1 << 64) - 1
NONE = 0xFFFFFFFF

MATCH_MUTANTS = ("le_for_lt", "highest_on_ties")
SCORE_MUTANTS = ("lt_for_le",)
WINNER_MUTANTS = ("last_of_equal", "exit_ignored", "exit_without_strict_best")


# ---- matching ----
def distances(src, tgt):
    """(ns, nt) f32: acc = 0; for j: t = s[j] - g[j]; acc = acc + t*t"""
    src, tgt = np.asarray(src, F), np.asarray(tgt, F)
    acc = np.zeros((src.shape[0], tgt.shape[0]), F)
    with np.errstate(all="ignore"):
        for j in range(src.shape[1]):
            t = src[:, j, None] - tgt[None, :, j]
            acc = acc + t * t
    return acc


def match(src, tgt, mutant=None):
    """-> (index uint32, distance f32): target 0 is the incumbent; a later target replaces it iff d_new < d_best"""
    d = distances(src, tgt)
    order = range(1, d.shape[1])
    first = 0
    if mutant == "highest_on_ties":                 # the scan from the other end
        order, first = range(d.shape[1] - 2, -1, -1), d.shape[1] - 1
    best, idx = d[:, first].copy(), np.full(d.shape[0], first, np.uint32)
    with np.errstate(invalid="ignore"):
        for t in order:
            take = d[:, t] <= best if mutant == "le_for_lt" else d[:, t] < best
            best[take], idx[take] = d[take, t], t
    return idx, best


# ---- samples ----
def state0(m, max_iters, seed):
    return ((((m << 32) & MASK) ^ max_iters ^ GOLDEN) ^ seed) & MASK


def map_draws(r0, r1, r2, m):
    """global_registration.rs:261-272: three distinct indices below m (m >= 3)"""
    i0 = r0 % m
    i1 = r1 % (m - 1)
    i1 += i1 >= i0
    i2 = r2 % (m - 2)
    i2 += i2 >= min(i0, i1)
    i2 += i2 >= max(i0, i1)
    return i0, i1, i2


def lcg_triples(m, max_iters, seed=0):
    """the sequential recurrence: three draws (state >> 32) per iteration -> (max_iters, 3) uint32"""
    s, out = state0(m, max_iters, seed), np.zeros((max_iters, 3), np.uint32)
    for it in range(max_iters):
        r = []
        for _ in range(3):
            s = (s * LCG_MULT + LCG_INC) & MASK
            r.append(s >> 32)
        out[it] = map_draws(*r, m)
    return out


def lcg_jump(steps):
    """(multiplier, increment) of `steps` steps at once, by repeated squaring: what the device does per iteration"""
    cm, ci, mult, inc = LCG_MULT, LCG_INC, 1, 0
    while steps:
        if steps & 1:
            mult, inc = (mult * cm) & MASK, (inc * cm + ci) & MASK
        ci, cm = ((cm + 1) * ci) & MASK, (cm * cm) & MASK
        steps >>= 1
    return mult, inc


# ---- model, score, winner ----
def gather(src, tgt, corr_src, corr_tgt):
    """(m, 3) source and target points of the pairs; a pair with an index out of range is NaN on both sides"""
    src, tgt = np.asarray(src, F).reshape(-1, 3), np.asarray(tgt, F).reshape(-1, 3)
    cs, ct = np.asarray(corr_src, np.int64), np.asarray(corr_tgt, np.int64)
    ok = (cs < len(src)) & (ct < len(tgt))
    ps, pt = np.full((len(cs), 3), np.nan, F), np.full((len(cs), 3), np.nan, F)
    ps[ok], pt[ok] = src[cs[ok]], tgt[ct[ok]]
    return ps, pt


def singular_ratio(s3, t3):
    s, t = np.asarray(s3, np.float64), np.asarray(t3, np.float64)
    sv = np.linalg.svd((s - s.mean(0)).T @ (t - t.mean(0)), compute_uv=False)
    return sv[1] / sv[0] if sv[0] > 0 else 0.0


def model(s3, t3):
    """three pairs -> (R (3, 3), t (3,), centroids) in f64, or None: a non-finite point, or sigma_2 <= 1e-9 sigma_1"""
    s, t = np.asarray(s3, F).astype(np.float64), np.asarray(t3, F).astype(np.float64)
    if not (np.isfinite(s).all() and np.isfinite(t).all()):
        return None
    cs, ct = s.sum(0) / 3.0, t.sum(0) / 3.0
    h = (s - cs).T @ (t - ct)
    u, sv, vt = np.linalg.svd(h)
    if not sv[1] > 1e-9 * sv[0]:
        return None
    v = vt.T
    r = v @ np.diag([1.0, 1.0, np.sign(np.linalg.det(v @ u.T))]) @ u.T
    return r, ct - r @ cs, cs, ct


def models(ps, pt, triples):
    """every candidate's stored transform: (n, 12) f32 (NaN without a model) and the valid flags"""
    m, out = len(ps), np.full((len(triples), 12), np.nan, F)
    valid = np.zeros(len(triples), bool)
    for it, (a, b, c) in enumerate(np.asarray(triples, np.int64)):
        if max(a, b, c) >= m or len({a, b, c}) < 3:
            continue
        r = model(ps[[a, b, c]], pt[[a, b, c]])
        if r is not None:
            out[it, :9], out[it, 9:], valid[it] = r[0].reshape(9).astype(F), r[1].astype(F), True
    return out, valid


def d2_all(T, ps, pt):
    """(n, m) f32 squared distances under the stored transforms: x' = ((R00*x + R01*y) + R02*z) + tx; d2 = (dx*dx + dy*dy) + dz*dz"""
    T, ps, pt = np.asarray(T, F).reshape(-1, 12), np.asarray(ps, F), np.asarray(pt, F)
    x, y, z = ps[None, :, 0], ps[None, :, 1], ps[None, :, 2]
    with np.errstate(all="ignore"):
        d = [(((T[:, 3 * a, None] * x + T[:, 3 * a + 1, None] * y) + T[:, 3 * a + 2, None] * z) + T[:, 9 + a, None]) - pt[None, :, a] for a in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def score(T, ps, pt, threshold, mutant=None):
    """(n,) uint32 inlier counts: d2 <= threshold*threshold, the product in f32; NaN is never an inlier"""
    thr2 = F(threshold) * F(threshold)
    d2 = d2_all(T, ps, pt)
    with np.errstate(invalid="ignore"):
        return ((d2 < thr2) if mutant == "lt_for_le" else (d2 <= thr2)).sum(1).astype(np.uint32)


def exit_count(inlier_ratio, m):
    """:255 -- max(3, ceil(inlier_ratio * m as f32) as usize), the conversion saturating, NaN -> 0"""
    with np.errstate(all="ignore"):
        e = np.ceil(F(inlier_ratio) * F(m))
    if np.isnan(e) or e <= 0:
        return 3
    return max(3, (1 << 64) - 1 if e >= F(2.0) ** 64 else int(e))


def winner(counts, valid, E, mutant=None):
    """the literal loop :259-299 -> (found, best_iteration, best_count, early_exit, iterations_run)"""
    best, best_it, n = 0, 0, len(counts)
    for it in range(n):
        if not valid[it]:
            continue
        c = int(counts[it])
        if mutant == "exit_without_strict_best" and c >= E and c > 0:
            return True, it, c, True, it + 1
        if c > best or (mutant == "last_of_equal" and c == best and c > 0):
            best, best_it = c, it
            if c >= E and mutant != "exit_ignored":
                return True, it, c, True, it + 1
    return best > 0, best_it, best, False, n


def winner_closed(counts, valid, E):
    """the closed form the device runs: the first candidate that reaches E, else the lowest-indexed maximum"""
    c = np.where(np.asarray(valid, bool), np.asarray(counts, np.int64), 0)
    hit = np.nonzero((c >= E) & (c > 0))[0]
    if len(hit):
        return True, int(hit[0]), int(c[hit[0]]), True, int(hit[0]) + 1
    if c.max(initial=0) == 0:
        return False, 0, 0, False, len(c)
    return True, int(np.argmax(c)), int(c.max()), False, len(c)


IDENTITY12 = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)


def ransac(src, tgt, corr_src, corr_tgt, threshold, inlier_ratio, triples, transforms=None, mutant=None):
    """the whole call on the checker's models (or on given stored transforms, NaN rows = no model) -> dict like the device's outputs"""
    ps, pt = gather(src, tgt, corr_src, corr_tgt)
    if transforms is None:
        T, valid = models(ps, pt, triples)
    else:
        T = np.asarray(transforms, F).reshape(-1, 12)
        valid = ~np.isnan(T).any(1)
    counts = score(T, ps, pt, threshold, mutant if mutant in SCORE_MUTANTS else None)
    found, it, c, ex, run = winner(counts, valid, exit_count(inlier_ratio, len(ps)), mutant if mutant in WINNER_MUTANTS else None)
    return dict(transform=T[it].copy() if found else IDENTITY12.copy(), inlier_count=c, iterations_run=run, best_iteration=it if found else 0,
                early_exit=ex, inlier_ratio=F(c) / F(len(ps)), cand_transform=T, cand_count=counts, valid=valid)


# ---- the inputs of tests/test_gpu_global.py ----
MATCH_NS = [1, 63, 64, 65, MATCH_SRC_PER_BLOCK - 1, MATCH_SRC_PER_BLOCK + 1, 2 * MATCH_SRC_PER_BLOCK + 1]
MATCH_NT = [1, 2, MATCH_TGT_TILE - 1, MATCH_TGT_TILE, MATCH_TGT_TILE + 1, 2 * MATCH_TGT_TILE + 1]
MATCH_SIZES = [(ns, 2 * MATCH_TGT_TILE + 1) for ns in MATCH_NS] + [(65, nt) for nt in MATCH_NT] + [(2 * MATCH_SRC_PER_BLOCK + 1, 1)]


def match_case(kind, ns, nt, seed=0):
    """descriptors (src, tgt) of one matching case.
    int     small integers, so that equal distances are genuine ties; for nt > MATCH_TGT_TILE the targets just below and at the tile
            boundary (MATCH_TGT_TILE - 1, MATCH_TGT_TILE) are copies of source 0's best target, moved to an even closer descriptor:
            the tie spans the boundary and the lower index must win
    float   random floats
    nan0    float, target 0 is NaN (the incumbent that is never replaced)
    nanmid  float, a NaN target in the middle of the second tile (never replaces)
    equal   every target the same descriptor"""
    rng = np.random.default_rng(1000 * ns + nt + seed)
    if kind == "int":
        src, tgt = rng.integers(0, 3, (ns, DIM)).astype(F), rng.integers(0, 3, (nt, DIM)).astype(F)
        if nt > MATCH_TGT_TILE:
            near = src[0].copy()
            near[0] += 1                            # distance 1 from source 0: nothing random is that close in 33 dimensions
            tgt[MATCH_TGT_TILE - 1] = tgt[MATCH_TGT_TILE] = near
            if nt > MATCH_TGT_TILE + 5:
                tgt[MATCH_TGT_TILE + 5] = near
        return src, tgt
    src, tgt = rng.random((ns, DIM), F), rng.random((nt, DIM), F)
    if kind == "nan0":
        tgt[0, 7] = np.nan
    elif kind == "nanmid" and nt > MATCH_TGT_TILE + MATCH_TGT_TILE // 2:
        tgt[MATCH_TGT_TILE + MATCH_TGT_TILE // 2, 3] = np.nan
    elif kind == "equal":
        tgt[:] = tgt[0]
    return src, tgt


def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def score_case(m, n_cand, seed=0):
    """a random pair list in the unit cube moved by a small rotation, with noise, some pairs with an index out of range, and random
    sample rows of which a few are repeated / out of range -> (src, tgt, corr_src, corr_tgt, samples)"""
    rng = np.random.default_rng(7 * m + n_cand + seed)
    ns = nt = m + 5
    src = rng.random((ns, 3), F)
    tgt = (src.astype(np.float64) @ rot((1, 2, 3), 0.3).T + (0.1, -0.2, 0.05) + rng.normal(0, 0.15, (ns, 3))).astype(F)
    cs, ct = rng.permutation(ns)[:m].astype(np.uint32), None
    ct = cs.copy()
    if m >= 8:
        cs[m // 3], ct[m // 2], cs[m - 1] = NONE, nt, ns            # never counted, never dereferenced
    smp = rng.integers(0, m, (n_cand, 3)).astype(np.uint32)
    if n_cand >= 8:
        smp[2, 1], smp[5, 2] = smp[2, 0], m                         # without a model
    return src, tgt, cs, ct, smp


SCORE_M = [3, 4, 63, 64, 65, PAIRS_PER_BLOCK - 1, PAIRS_PER_BLOCK, PAIRS_PER_BLOCK + 1, 2 * PAIRS_PER_BLOCK + 1]
SCORE_CAND = [1, 127, 128, 129, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SCORE_SIZES = [(m, 129) for m in SCORE_M] + [(65, n) for n in SCORE_CAND] + [(2 * PAIRS_PER_BLOCK + 1, 2 * CHUNK + 1)]
SCORE_THRESHOLD = 0.3


def model_case(n=300, seed=5):
    """triples in the unit cube with sigma_2 / sigma_1 >= 0.05 (rejection sampling), their images under random rigid motions plus a
    little noise (so that the fit is a least-squares one), then four degenerate rows: equal indices, an index >= m, three collinear
    points, a non-finite point -> (src, tgt, corr, samples, n_good)"""
    rng = np.random.default_rng(seed)
    src, tgt, smp = [], [], []
    while len(smp) < n:
        s = rng.random((3, 3), F)
        r = rot(rng.normal(size=3), rng.uniform(0, np.pi))
        t = (s.astype(np.float64) @ r.T + rng.uniform(-1, 1, 3) + rng.normal(0, 0.01, (3, 3))).astype(F)
        if singular_ratio(s, t) >= 0.05:
            base = len(src)
            src += list(s); tgt += list(t); smp.append((base, base + 1, base + 2))
    base = len(src)
    src += [(0, 0, 0), (1, 2, 3), (2, 4, 6), (0.5, 0.25, 0.125)]            # exactly collinear, centroid exact
    tgt += [(1, 0, 0), (0, 1, 0), (0, 0, 1), (np.inf, 0, 0)]
    src, tgt = np.asarray(src, F), np.asarray(tgt, F)
    m = len(src)
    smp += [(0, 0, 1), (0, 1, m), (base, base + 1, base + 2), (0, 1, base + 3)]
    corr = np.arange(m, dtype=np.uint32)
    return src, tgt, corr, np.asarray(smp, np.uint32), n


WINNER_M, WINNER_INLIERS, WINNER_THRESHOLD, WINNER_RATIO = 200, 80, 0.01, 0.25


def winner_pairs(seed=11):
    """200 pairs: the first 80 are exact under one rigid motion with small-integer coordinates (a quarter turn about z and an integer
    shift: every product and sum is exact), the rest are junk -> (src, tgt, corr)"""
    rng = np.random.default_rng(seed)
    src = (rng.integers(0, 64, (WINNER_M, 3)) / 4.0).astype(F)
    tgt = (rng.integers(0, 64, (WINNER_M, 3)) / 4.0).astype(F)
    rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    tgt[:WINNER_INLIERS] = (src[:WINNER_INLIERS].astype(np.float64) @ rz.T + (1, 2, 3)).astype(F)
    return src, tgt, np.arange(WINNER_M, dtype=np.uint32)


def winner_case(name, seed=11):
    """sample rows for winner_pairs(): junk rows (triples of junk pairs) with planted rows (triples of exact pairs) at named places.
    -> (samples, expected) with expected = (best_iteration or None when nothing wins, early_exit, iterations_run)"""
    rng = np.random.default_rng(seed + 1)
    n = 2 * CHUNK + 1

    def junk(k):
        return np.stack([rng.permutation(np.arange(WINNER_INLIERS, WINNER_M))[:3] for _ in range(k)]).astype(np.uint32)

    def planted():
        return rng.permutation(WINNER_INLIERS)[:3].astype(np.uint32)
    smp = junk(n)
    at = {"exit_first_chunk": [77], "exit_chunk_last_row": [CHUNK - 1], "exit_second_chunk_first_row": [CHUNK], "two_exits": [CHUNK + 9, 300],
          "no_exit": [CHUNK + 904], "nothing_wins": []}[name.split(":")[0]]
    for i in at:
        # three exact pairs that are not collinear (the CPU twin checks that the row has a model)
        while True:
            smp[i] = planted()
            if singular_ratio(*[a[smp[i].astype(np.int64)] for a in winner_pairs(seed)[:2]]) > 0.05:
                break
    if name == "two_exits":
        smp[CHUNK + 9] = smp[300]                   # the same triple: the same model, the same count
    if name == "nothing_wins":
        smp[:] = (0, 0, 1)
    return smp


WINNER_CASES = ["exit_first_chunk", "exit_chunk_last_row", "exit_second_chunk_first_row", "two_exits", "no_exit", "nothing_wins"]


def tie_case():
    """equal best counts in two different chunks, the exit not reached: the same planted row at CHUNK + 9 and at 300, inlier_ratio 0.9
    (E = 180 > 80 exact pairs) -> samples; the lower iteration must win"""
    return winner_case("two_exits")


# ---- the pose-recovery case of the whole pipeline ----
POSE_N, POSE_RADIUS, POSE_K, POSE_THRESHOLD, POSE_ITERS, POSE_SEED = 2000, 0.12, 10, 0.02, CHUNK + 1, 0


def pose_case():
    """2 000 points of a smooth asymmetric surface z = f(x, y) over the unit square with its analytic normals (the target), and the same
    points moved by the inverse of a planted rigid motion (the source, with the normals turned along): a turn of 2.6 rad about
    (1, 2, 3) and a shift of half the cloud's size, outside the basin of ICP from the identity (the CPU twin shows it on the oracle).
    -> (source, target, source_normals, target_normals, planted 4 x 4 f64: source -> target)"""
    from threecrate_amd import synth
    u = synth.uniform_cloud(POSE_N, 33).astype(np.float64)
    x, y = u[:, 0], u[:, 1]
    z = 0.3 * np.sin(4 * x) * np.cos(3 * y) + 0.2 * x * x + 0.1 * x * y
    fx = 1.2 * np.cos(4 * x) * np.cos(3 * y) + 0.4 * x + 0.1 * y
    fy = -0.9 * np.sin(4 * x) * np.sin(3 * y) + 0.1 * x
    n = np.stack([-fx, -fy, np.ones_like(x)], 1)
    n /= np.linalg.norm(n, axis=1)[:, None]
    tgt = np.stack([x, y, z], 1)
    r0, t0 = rot((1, 2, 3), 2.6), np.array([0.5, -0.3, 0.2])
    src = (tgt - t0) @ r0                                       # rows: R0^T (p - t0)
    planted = np.eye(4)
    planted[:3, :3], planted[:3, 3] = r0, t0
    return src.astype(F), tgt.astype(F), (n @ r0).astype(F), n.astype(F), planted


def partners_are_nearest(transform12, src, tgt):
    """the fraction of source points whose nearest target point under the stored transform is their own image (point i of both clouds).
    At 1.0 the first point-to-point ICP step is the Kabsch fit over the true pairs: the start is inside ICP's basin"""
    T = np.asarray(transform12, np.float64)
    moved = np.asarray(src, np.float64) @ T[:9].reshape(3, 3).T + T[9:]
    d = ((moved[:, None, :] - np.asarray(tgt, np.float64)[None, :, :]) ** 2).sum(2)
    return float((d.argmin(1) == np.arange(len(src))).mean())


def pose_chain(seed=POSE_SEED):
    """the checker chain fpfh_checker -> match -> winner on pose_case() -> (the ransac dict, the share of correct matches)"""
    from tests import fpfh_checker as FC
    src, tgt, sn, tn, _ = pose_case()
    sd = FC.fpfh(src, sn, POSE_RADIUS, POSE_K)["desc"]
    td = FC.fpfh(tgt, tn, POSE_RADIUS, POSE_K)["desc"]
    idx, _ = match(sd, td)
    corr = np.arange(len(src), dtype=np.uint32)
    r = ransac(src, tgt, corr, idx, POSE_THRESHOLD, 0.25, lcg_triples(len(src), POSE_ITERS, seed))
    return r, float((idx == corr).mean())
