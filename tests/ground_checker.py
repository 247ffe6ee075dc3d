"""Ground segmentation restated in numpy: the contract of include/threecrate_hip_ground.h with its arithmetic (arith="f64", what the
device is held to), and the reference's own arithmetic (arith="f32": f32 sums in index order, as ground_segmentation.rs adds them up),
which documents what the header's deviation costs.

segment(points, cfg) -> a dict:
  labels    (n,) bool
  patches   a structured array, one record per patch in (zone, ring, sector) order: count, n_inliers, status, normal, d, mean_z, flatness
  patch_of  (n,) the patch of every point, n_patches for a point out of range or not finite
  iterations, early_stop   per patch: plane fits made, and whether the loop ended on equal counts
  margin    the smallest relative distance of any decision taken to its flipping point (arith="f64" only), and margin_at, which one

The margin.  With f64 sums on both sides a device result differs from this one by the order of summation alone, some 1e-15 relative; a
decision whose operands are further apart than 1e-6 relative cannot come out differently.  The decisions:
  r        a finite point's r against max_range, every zone radius and the nearest inner ring edge of its zone, |r - e| / e.  An edge
           at 0 is no decision (r is never negative)
  theta    against the nearest sector edge k * sector_width, k = 0 .. sectors, |theta - edge| / 2 pi; zones of one sector have no edge.
           A point with y == +-0 and x >= 0 is exempt from the edge at 0: atan2 is exactly +-0 there (C Annex F), on every
           implementation, and +-0 is not below 0
  z        a patch point's z against the seed cutoff
  dist     a patch point's distance against dist_threshold, every iteration
  valid    the validation values that were looked at against their thresholds
  tie      the early stop compares two counts: they differ by a whole point or not at all, max(|new - cur|, 1) / max(new, cur)
  gap      (l1 - l0) / l2 of every PCA whose normal is used, and |normal.z| of that normal (its sign is a decision too)
"""
import numpy as np

STATUS = ("EMPTY", "TOO_FEW_POINTS", "TOO_FEW_SEEDS", "TOO_FEW_INLIERS", "NO_ITERATION", "NOT_UPRIGHT", "ELEVATION", "NOT_FLAT", "GROUND")
EMPTY, TOO_FEW_POINTS, TOO_FEW_SEEDS, TOO_FEW_INLIERS, NO_ITERATION, NOT_UPRIGHT, ELEVATION, NOT_FLAT, GROUND = range(9)
PATCH_DTYPE = np.dtype([("count", np.uint32), ("n_inliers", np.uint32), ("status", np.uint32), ("normal", np.float32, (3,)),
                        ("d", np.float32), ("mean_z", np.float32), ("flatness", np.float32)])
F = np.float32
TWO_PI = F(2.0) * F(np.pi)


def default_config(sensor_height=1.723, **over):
    """PatchworkConfig::default() as a dict of the C struct's fields (lists for the per-zone ones)"""
    cfg = dict(sensor_height=sensor_height, zone_radii=[0.0, 2.7, 12.3625, 22.025, 80.0], num_rings=[2, 4, 4, 4], num_sectors=[16, 32, 54, 32],
               max_range=80.0, min_points_per_patch=10, num_seed_points=20, seed_selection_threshold=0.5, dist_threshold=0.125,
               num_iterations=3, uprightness_threshold=0.707, flatness_threshold=0.05, elevation_threshold=1.0)
    assert set(over) <= set(cfg), set(over) - set(cfg)
    cfg.update(over)
    return cfg


def patch_count(cfg):
    return int(sum(r * s for r, s in zip(cfg["num_rings"], cfg["num_sectors"])))


def ordered_bits(z):
    b = np.ascontiguousarray(z, F).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


class _Margin:
    def __init__(self):
        self.value, self.at = np.inf, None

    def take(self, values, what):
        values = np.asarray(values, np.float64).reshape(-1)
        values = values[~np.isnan(values)]
        if values.size and values.min() < self.value:
            self.value, self.at = float(values.min()), what


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)


def bucket(points, cfg, margin=None):
    """the header's (1): the patch of every point (n_patches: in none), f32 with one rounding per operation"""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, n_patches = len(p), patch_count(cfg)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    patch = np.full(n, n_patches, np.int64)
    with np.errstate(all="ignore"):
        finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        r = np.sqrt(x * x + y * y)
        live = finite & ~(r > F(cfg["max_range"]))
        theta = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F)
        theta = np.where(theta < 0, theta + TWO_PI, theta).astype(F)
        radii = [F(v) for v in cfg["zone_radii"]]
        if margin is not None:
            rf = r[finite].astype(np.float64)
            for e in [cfg["max_range"]] + list(cfg["zone_radii"]):
                if np.isfinite(e) and float(F(e)) > 0:
                    margin.take(np.abs(rf - float(F(e))) / float(F(e)), f"r against {e}")
        base, taken = 0, np.zeros(n, bool)
        for zone, (rings, sectors) in enumerate(zip(cfg["num_rings"], cfg["num_sectors"])):
            r_in, r_out = radii[zone], radii[zone + 1]
            m = live & ~taken & (r >= r_in) & (r < r_out)
            taken |= m
            ring_width = F(r_out - r_in) / F(rings)
            u = (r[m] - r_in) / ring_width
            ring = np.where(~(u >= 0), 0, np.where(u < F(rings), np.minimum(np.nan_to_num(u, nan=0.0, posinf=0.0).astype(np.int64), rings - 1), rings - 1))
            sector_width = TWO_PI / F(sectors)
            v = theta[m] / sector_width
            sector = np.where(~(v >= 0), 0, np.where(v < F(sectors), np.minimum(np.nan_to_num(v, nan=0.0, posinf=0.0).astype(np.int64), sectors - 1), sectors - 1))
            patch[m] = base + ring * sectors + sector
            base += rings * sectors
            if margin is not None and m.any():
                if rings > 1:
                    k = np.clip(np.rint(u.astype(np.float64)), 1, rings - 1)
                    edge = float(r_in) + k * float(ring_width)
                    margin.take(np.abs(r[m].astype(np.float64) - edge) / edge, f"r against a ring edge of zone {zone}")
                if sectors > 1:
                    k = np.clip(np.rint(v.astype(np.float64)), 0, sectors)
                    dist = np.abs(theta[m].astype(np.float64) - k * float(sector_width)) / float(TWO_PI)
                    exact_zero = (y[m] == 0) & (x[m] >= 0) & (k == 0)
                    margin.take(dist[~exact_zero], f"theta against a sector edge of zone {zone}")
    return patch


def _pca64(q):
    """q: the set's points about the pivot (m, 3) f64 -> mean, eigenvalues ascending, eigenvectors (columns), by raw moments as the header says"""
    cnt = float(len(q))
    s1 = q.sum(axis=0)
    mean = s1 / cnt
    s2 = {(a, b): float((q[:, a] * q[:, b]).sum()) for a in range(3) for b in range(a, 3)}
    cov = np.zeros((3, 3))
    for (a, b), s in s2.items():
        cov[a, b] = cov[b, a] = s / cnt - mean[a] * mean[b]
    w, v = np.linalg.eigh(cov)
    return mean, w, v


def _fit_f64(pts, cfg, margin, name):
    """one patch, the header's (2) to (4) in its arithmetic; pts (count, 3) f32 in sorted order (z ascending, ties by index) with count >= min"""
    count = len(pts)
    rec = dict(status=None, n_inliers=0, normal=(0, 0, 0), d=0.0, mean_z=0.0, flatness=0.0, iterations=0, early_stop=False, inliers=None)
    pivot = pts[0].astype(np.float64)
    q = pts.astype(np.float64) - pivot
    k = min(int(cfg["num_seed_points"]), count)
    cutoff = q[:k, 2].sum() / float(k) + float(F(cfg["seed_selection_threshold"]))
    margin.take(_rel(q[:, 2], cutoff), f"z against the cutoff, {name}")
    cur = q[:, 2] <= cutoff
    if cur.sum() < 3:
        rec["status"] = TOO_FEW_SEEDS
        return rec
    if cfg["num_iterations"] == 0:
        rec["status"] = NO_ITERATION
        return rec
    thr = float(F(cfg["dist_threshold"]))
    normal = d = None
    for _ in range(int(cfg["num_iterations"])):
        mean, w, v = _pca64(q[cur])
        normal = v[:, 0] if v[2, 0] >= 0 else -v[:, 0]
        margin.take([(w[1] - w[0]) / max(abs(w[2]), 1e-300), abs(normal[2])], f"eigen gap / normal sign, {name}")
        d = -((normal[0] * mean[0] + normal[1] * mean[1]) + normal[2] * mean[2])
        dist = np.abs(((normal[0] * q[:, 0] + normal[1] * q[:, 1]) + normal[2] * q[:, 2]) + d)
        margin.take(_rel(dist, thr), f"distance against dist_threshold, {name}")
        new = dist <= thr
        rec["iterations"] += 1
        if new.sum() < 3:
            rec["status"] = TOO_FEW_INLIERS
            return rec
        margin.take(max(abs(int(new.sum()) - int(cur.sum())), 1) / max(int(new.sum()), int(cur.sum())), f"early-stop tie, {name}")
        stop = new.sum() == cur.sum()
        cur = new
        if stop:
            rec["early_stop"] = True
            break
    mean, w, _ = _pca64(q[cur])
    total = (w[0] + w[1]) + w[2]
    flatness = w[0] / total if total > 0 else 0.0
    mean_z = pivot[2] + q[cur, 2].sum() / float(cur.sum())
    rec.update(n_inliers=int(cur.sum()), normal=tuple(F(c) for c in normal), d=F(d - ((normal[0] * pivot[0] + normal[1] * pivot[1]) + normal[2] * pivot[2])),
               mean_z=F(mean_z), flatness=F(flatness), inliers=cur)
    up, elev = abs(F(normal[2])), abs(F(mean_z) + F(cfg["sensor_height"]))
    margin.take(_rel(up, F(cfg["uprightness_threshold"])), f"uprightness, {name}")
    if up < F(cfg["uprightness_threshold"]):
        rec["status"] = NOT_UPRIGHT
        return rec
    margin.take(_rel(elev, F(cfg["elevation_threshold"])), f"elevation, {name}")
    if elev > F(cfg["elevation_threshold"]):
        rec["status"] = ELEVATION
        return rec
    if total > 0:
        margin.take(_rel(F(flatness), F(cfg["flatness_threshold"])), f"flatness, {name}")
        if F(flatness) > F(cfg["flatness_threshold"]):
            rec["status"] = NOT_FLAT
            return rec
    rec["status"] = GROUND
    return rec


def _seq(a):
    """the f32 sum of a one after another, as a Rust loop adds it up"""
    a = np.asarray(a, F)
    return np.cumsum(a, dtype=F)[-1] if len(a) else F(0)


def _pca32(p):
    """pca() of the reference on (m, 3) f32 points in index order: f32 sums one after another.  The eigen-solver is LAPACK's f32 one, not
    nalgebra's: the one step that is not restated operation for operation"""
    n = F(len(p))
    mean = np.array([_seq(p[:, c]) for c in range(3)], F) / n
    dd = (p - mean).astype(F)
    cov = np.zeros((3, 3), F)
    for a in range(3):
        for b in range(3):
            cov[a, b] = _seq(dd[:, a] * dd[:, b]) / n
    w, v = np.linalg.eigh(cov)
    return mean, w.astype(F), v.astype(F)


def _fit_f32(pts_by_index, cfg):
    """fit_patch and validate_patch of the reference: the patch's points in INDEX order, (count, 3) f32"""
    p = pts_by_index
    count = len(p)
    rec = dict(status=None, n_inliers=0, normal=(0, 0, 0), d=0.0, mean_z=0.0, flatness=0.0, iterations=0, early_stop=False, inliers=None)
    by_z = np.argsort(p[:, 2], kind="stable")
    k = min(int(cfg["num_seed_points"]), count)
    cutoff = _seq(p[by_z[:k], 2]) / F(k) + F(cfg["seed_selection_threshold"])
    below = p[by_z, 2] <= cutoff
    n_seed = len(below) if below.all() else int(np.argmin(below))          # take_while
    cur = by_z[:n_seed]
    if len(cur) < 3:
        rec["status"] = TOO_FEW_SEEDS
        return rec
    if cfg["num_iterations"] == 0:
        rec["status"] = NO_ITERATION
        return rec
    normal = None
    for _ in range(int(cfg["num_iterations"])):
        mean, _, v = _pca32(p[cur])
        normal = v[:, 0] if not v[2, 0] < 0 else -v[:, 0]
        d = -((normal[0] * mean[0] + normal[1] * mean[1]) + normal[2] * mean[2])
        dist = np.abs(((normal[0] * p[:, 0] + normal[1] * p[:, 1]) + normal[2] * p[:, 2]) + d)
        new = np.flatnonzero(dist <= F(cfg["dist_threshold"]))
        rec["iterations"] += 1
        if len(new) < 3:
            rec["status"] = TOO_FEW_INLIERS
            return rec
        stop = len(new) == len(cur)
        cur = new
        if stop:
            rec["early_stop"] = True
            break
    mask = np.zeros(count, bool)
    mask[cur] = True
    mean_z = _seq(p[cur, 2]) / F(len(cur))
    _, w, _ = _pca32(p[cur])
    total = (w[0] + w[1]) + w[2]
    flatness = w[0] / total if total > 0 else F(0)
    rec.update(n_inliers=len(cur), normal=tuple(normal), d=d, mean_z=mean_z, flatness=flatness, inliers=mask)
    if abs(normal[2]) < F(cfg["uprightness_threshold"]):
        rec["status"] = NOT_UPRIGHT
    elif abs(mean_z + F(cfg["sensor_height"])) > F(cfg["elevation_threshold"]):
        rec["status"] = ELEVATION
    elif total > 0 and flatness > F(cfg["flatness_threshold"]):
        rec["status"] = NOT_FLAT
    else:
        rec["status"] = GROUND
    return rec


def segment(points, cfg, arith="f64"):
    assert arith in ("f64", "f32")
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n, n_patches = len(p), patch_count(cfg)
    margin = _Margin()
    patch_of = bucket(p, cfg, margin if arith == "f64" else None)
    labels = np.zeros(n, bool)
    patches = np.zeros(n_patches, PATCH_DTYPE)
    iterations, early = np.zeros(n_patches, np.int64), np.zeros(n_patches, bool)
    # patch by patch: ascending in the order-preserving bits of z, ties by index (what a stable sort of the keys leaves)
    order = np.lexsort((np.arange(n), ordered_bits(p[:, 2]), patch_of))
    sorted_patch = patch_of[order]
    starts = np.searchsorted(sorted_patch, np.arange(n_patches + 1))
    counts = np.diff(starts)
    patches["count"] = counts
    patches["status"][(counts > 0) & (counts < cfg["min_points_per_patch"])] = TOO_FEW_POINTS
    for pid in np.flatnonzero((counts > 0) & (counts >= cfg["min_points_per_patch"])):
        idx = order[starts[pid]:starts[pid + 1]]
        if arith == "f64":
            rec = _fit_f64(p[idx], cfg, margin, f"patch {pid}")
        else:
            idx = np.sort(idx)
            rec = _fit_f32(p[idx], cfg)
        patches["status"][pid] = rec["status"]
        iterations[pid], early[pid] = rec["iterations"], rec["early_stop"]
        if rec["status"] >= NOT_UPRIGHT:
            patches["n_inliers"][pid], patches["normal"][pid], patches["d"][pid] = rec["n_inliers"], rec["normal"], rec["d"]
            patches["mean_z"][pid], patches["flatness"][pid] = rec["mean_z"], rec["flatness"]
        if rec["status"] == GROUND:
            labels[idx[rec["inliers"]]] = True
    return dict(labels=labels, patches=patches, patch_of=patch_of, iterations=iterations, early_stop=early, margin=margin.value, margin_at=margin.at)
