"""RANSAC plane segmentation restated in numpy (threecrate-algorithms/src/segmentation.rs:28-91, :117-180; the sampler of
threecrate-gpu/src/segmentation.rs:979-1011), as include/threecrate_hip_segmentation.h pins it.  Every float operation is on
np.float32 values, one at a time and left to right, so nothing is contracted; the sampler runs on Python integers masked to 64 bits."""
import numpy as np

F = np.float32
M64 = (1 << 64) - 1
LCG_MUL, LCG_INC, GOLDEN = 6364136223846793005, 1442695040888963407, 0x9E3779B97F4A7C15
MIN_LEN = F(1e-8)


def samples(n, max_iters, seed=0):
    """(max_iters, 3) uint32: the triples of tc_segment_plane(n, max_iters, seed)"""
    state = (((n << 32) & M64) ^ max_iters ^ GOLDEN ^ seed) & M64
    out = np.empty((max_iters, 3), np.uint32)
    for it in range(max_iters):
        draw = []
        for _ in range(3):
            state = (state * LCG_MUL + LCG_INC) & M64
            draw.append((state >> 32) % n)
        a, b, c = draw
        if a == b or a == c or b == c:
            a, b, c = it % n, (it * 37 + 1) % n, (it * 101 + 2) % n
            while b == a:
                b = (b + 1) % n
            while c == a or c == b:
                c = (c + 1) % n
        out[it] = (a, b, c)
    return out


def collisions(n, max_iters, seed=0):
    """(max_iters,) bool: the iterations whose three draws collided, i.e. whose triple is the closed-form fallback"""
    state = (((n << 32) & M64) ^ max_iters ^ GOLDEN ^ seed) & M64
    out = np.zeros(max_iters, bool)
    for it in range(max_iters):
        draw = []
        for _ in range(3):
            state = (state * LCG_MUL + LCG_INC) & M64
            draw.append((state >> 32) % n)
        out[it] = len(set(draw)) < 3
    return out


def model(p, triple):
    """(4,) float32 a, b, c, d of the plane through p[triple], or None (an index >= n, or len < 1e-8)"""
    p = np.asarray(p, F)
    i0, i1, i2 = (int(t) for t in triple)
    if max(i0, i1, i2) >= len(p):
        return None
    with np.errstate(all="ignore"):
        p0 = p[i0]
        v1, v2 = p[i1] - p0, p[i2] - p0
        cx = v1[1] * v2[2] - v1[2] * v2[1]
        cy = v1[2] * v2[0] - v1[0] * v2[2]
        cz = v1[0] * v2[1] - v1[1] * v2[0]
        ln = np.sqrt(cx * cx + cy * cy + cz * cz)
        if ln < MIN_LEN:
            return None
        a, b, c = cx / ln, cy / ln, cz / ln
        d = -(a * p0[0] + b * p0[1] + c * p0[2])
    return np.array([a, b, c, d], F)


def signed_offsets(p, coeff):
    """a*x + b*y + c*z + d per point, f32, left to right"""
    p = np.asarray(p, F)
    a, b, c, d = (F(v) for v in coeff)
    with np.errstate(all="ignore"):
        return a * p[:, 0] + b * p[:, 1] + c * p[:, 2] + d


def normal_length(coeff):
    a, b, c = (F(v) for v in coeff[:3])
    with np.errstate(all="ignore"):
        return np.sqrt(a * a + b * b + c * c)


def distances(p, coeff):
    """(n,) float32 distance_to_point (segmentation.rs:59-73)"""
    m = normal_length(coeff)
    if m < MIN_LEN:
        return np.full(len(p), np.inf, F)
    with np.errstate(all="ignore"):
        return np.abs(signed_offsets(p, coeff)) / m


def inliers(p, coeff, threshold):
    with np.errstate(all="ignore"):
        return np.nonzero(distances(p, coeff) <= F(threshold))[0].astype(np.uint32)


def segment(p, threshold, triples):
    """-> (coefficients or None, inliers, best index or None, counts (len(triples),) int64); a candidate without a model counts 0.
    The winner is the greatest count, the lowest index among equals; count 0 never wins."""
    counts = np.zeros(len(triples), np.int64)
    models = []
    for k, t in enumerate(triples):
        m = model(p, t)
        models.append(m)
        if m is not None:
            counts[k] = len(inliers(p, m, threshold))
    if counts.max(initial=0) == 0:
        return None, np.zeros(0, np.uint32), None, counts
    best = int(np.argmax(counts))            # the first of the maxima
    return models[best], inliers(p, models[best], threshold), best, counts


# ---- the clouds of the tests --------------------------------------------------------------------
def plane_clutter_cloud(n, seed=3):
    """~60 % of the points within +-0.01 of the plane 0.3 x - 0.2 y + z = 0.5, the rest uniform in the box"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    on = rng.random(n) < 0.6
    p[on, 2] = 0.5 - 0.3 * p[on, 0] + 0.2 * p[on, 1] + rng.normal(0.0, 0.004, int(on.sum()))
    return p.astype(F)


def two_plane_cloud(n, seed=4):
    """z = 0 (about 55 %) and x = 0.25 (about 45 %), both with noise"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    first = rng.random(n) < 0.55
    p[first, 2] = rng.normal(0.0, 0.003, int(first.sum()))
    p[~first, 0] = 0.25 + rng.normal(0.0, 0.003, int((~first).sum()))
    return p.astype(F)


WINNER_THRESHOLD = F(1e-3)


def winner_cloud(n, triples, target, seed=9):
    """n points of which exactly four are coplanar (z = 0): the triple of iteration `target` and one further point, picked so that
    no earlier triple lies among the four.  Every other triple's plane holds its own three points only, so iteration `target` is the
    first with four inliers at WINNER_THRESHOLD: it wins only if the device drew exactly that triple there.  None when every
    choice of the fourth point is covered by an earlier triple."""
    mine = set(int(v) for v in triples[target])
    earlier = [set(int(v) for v in t) for t in triples[:target]]
    for extra in range(n):
        four = mine | {extra}
        if extra in mine or any(e <= four for e in earlier):
            continue
        rng = np.random.default_rng(seed)
        p = np.column_stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n)])
        p[sorted(four), 2] = 0.0
        return p.astype(F)
    return None


BAND_THRESHOLD = F(0.25)


def tilted_band_cloud(count=4096, seed=5):
    """Three points that span a tilted plane whose stored normal has m != 1, then `count` points foot + t * normal on both sides
    of the plane, the feet spread over the plane and t within a few ulps of BAND_THRESHOLD * m: after rounding to f32 their distances
    straddle the threshold ulp by ulp (tests/test_plane_cpu.py counts them).  -> (cloud, triple)"""
    base = np.array([[0.1, 0.2, 0.3], [0.7, 0.15, 0.6], [0.15, 0.75, 0.5]], F)
    coeff = model(base, (0, 1, 2)).astype(np.float64)
    nrm = coeff[:3]
    t0 = float(BAND_THRESHOLD) * float(normal_length(coeff)) / float(nrm @ nrm)
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(0.0, 0.6, count), rng.uniform(0.0, 0.6, count)
    b64 = base.astype(np.float64)
    feet = b64[0] + u[:, None] * (b64[1] - b64[0]) + v[:, None] * (b64[2] - b64[0])
    feet -= ((feet @ nrm + coeff[3]) / (nrm @ nrm))[:, None] * nrm             # onto the plane of the STORED coefficients
    t = (t0 + rng.integers(-5, 6, count) * float(np.spacing(BAND_THRESHOLD))) * rng.choice([-1.0, 1.0], count)
    return np.concatenate([base, (feet + t[:, None] * nrm).astype(F)]), (0, 1, 2)
