"""Named inputs of the streaming voxel map's tests (test infrastructure): tests/test_voxelmap_cpu.py proves on the checker that each
does what it claims (tells a mutant apart, is order-sensitive, crosses a doubling), tests/test_gpu_voxelmap.py runs the same arrays on
the device.  Everything is deterministic; the searches are short loops over f32 candidates."""
import functools

import numpy as np

from tests.voxelmap_checker import KEY_LIMIT, LONG_RUN, MIN_CAPACITY

F = np.float32


def _col(x):
    """x coordinates -> (n, 3) points on the x axis"""
    x = np.asarray(x, F).reshape(-1)
    return np.ascontiguousarray(np.stack([x, np.zeros_like(x), np.zeros_like(x)], axis=1))


@functools.lru_cache(maxsize=None)
def product_vs_division(voxel_size):
    """points x near the voxel faces where floor(x * (1 / voxel_size)) != floor(x / voxel_size) in f32 (found by search), each with a
    partner well inside the voxel the PRODUCT puts it in, so that the two rules also differ in the number of voxels"""
    vs = F(voxel_size)
    inv = F(1.0) / vs
    found = []
    for k in range(1, 4000):
        x = F(k) * vs
        for cand in (np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))):
            if np.floor(cand * inv) != np.floor(cand / vs):
                found.append(cand)
        if len(found) >= 24:
            break
    return _col(found)


def faces():
    """points exactly on voxel faces and their f32 neighbours on either side, voxel_size 0.5"""
    x = []
    for k in range(-6, 7):
        f = F(k) * F(0.5)
        x += [np.nextafter(f, F(-np.inf)), f, np.nextafter(f, F(np.inf))]
    pts = _col(x)
    return np.concatenate([pts, pts[:, [1, 0, 2]], pts[:, [2, 1, 0]]])


def negatives():
    """negative coordinates: floor and truncation differ; keys of both signs: signed and unsigned order differ"""
    x = F([-0.5, 0.5, -1.0, 1.0, -1.5, 1.5, -0.0, 0.0, -1e-30, 1e-30, -2.25, 2.25, -3.0, 2.999])
    pts = _col(x)
    return np.concatenate([pts, pts[:, [1, 0, 2]], pts[:, [2, 1, 0]], np.stack([x, -x, x], axis=1).astype(F)])


def nan_points():
    """a NaN on each axis (key 0 there, the sum poisoned), next to finite points of the same and of other voxels"""
    n = F(np.nan)
    return np.array([[0.25, 0.25, 0.25], [n, 0.5, 0.5], [1.5, n, 0.5], [0.5, 1.5, n], [n, n, 2.5], [0.75, 0.5, 0.5], [-1.5, 0.5, 0.5],
                     [n, 0.25, 0.25], [-1.5, n, 0.5]], F)


def order_sensitive():
    """300 points of the voxel [0, 1)^3 at voxel_size 1: 2^-40-scale and 0.9-scale values interleaved.  The f64 sum of the large ones
    sits near 135 (ulp 2^-45), the small ones carry bits down to 2^-63: every add rounds, and the rounding depends on the order."""
    rng = np.random.default_rng(1235)      # (a seed at which all three axes differ between the two fold orders)
    small = (rng.uniform(1.0, 2.0, (150, 3)) * 2.0 ** -40).astype(F)
    large = rng.uniform(0.85, 0.95, (150, 3)).astype(F)
    pts = np.empty((300, 3), F)
    pts[0::2], pts[1::2] = small, large
    return pts


@functools.lru_cache(maxsize=None)
def reciprocal_case(count):
    """`count` points of the voxel [0, 1)^3 at voxel_size 1 whose x sum s lies within a few f64 ulps of count * m, m the midpoint of two
    adjacent f32 values: (float)(s / count) and (float)(s * (1 / count)) fall on different sides of the tie.  count - 3 copies of a value a
    in [0.25, 0.33) and the remainder split greedily into three f32 values (24 + 24 + the last few bits); searched over a and the
    offset until the two roundings of the FOLDED sum differ."""
    import math
    u = 2.0 ** -25                                  # the f32 ulp in [0.25, 0.5)
    for K in range((1 << 23) + 1, (1 << 23) + 20000):
        a = K * u
        m = a + u / 2
        for j in range(-6, 7):
            target = count * m + j * math.ulp(count * m)
            rest, x = target - (count - 3) * a, [a] * (count - 3)
            for _ in range(3):
                v = float(np.nextafter(F(rest), F(0.0))) if float(F(rest)) > rest else float(F(rest))      # the f32 at or below
                x.append(v)
                rest -= v
            if rest != 0.0 or not all(0.0 <= v < 1.0 for v in x):
                continue
            s = 0.0
            for v in x:
                s = s + v
            if F(s / count) != F(s * (1.0 / count)):
                return _col(x)
    raise AssertionError("no case found")


def range_points():
    """voxel_size 1: the first and the last valid key on every axis"""
    lo, hi = F(-KEY_LIMIT), F(KEY_LIMIT - 1)
    return np.array([[lo, 0, 0], [hi, 0, 0], [0, lo, 0], [0, hi, 0], [0, 0, lo], [0, 0, hi], [lo, lo, lo], [hi, hi, hi], [hi + F(0.5), 1, 1]], F)


def out_of_range_points():
    """voxel_size 1: single coordinates one key beyond either limit, the infinities, and a product that saturates an i32"""
    return [F(KEY_LIMIT), F(-KEY_LIMIT - 1), F(np.inf), F(-np.inf), F(3e9), F(-3e38)]


def line_cloud(runs, m, seed=0):
    """`runs` distinct voxels on the x axis (voxel_size 1, keys -runs // 2 ..) x m points each, in a shuffled stream order"""
    rng = np.random.default_rng(seed + 7 * runs + m)
    k = np.repeat(np.arange(runs) - runs // 2, m)
    pts = np.stack([k + rng.uniform(0.05, 0.95, len(k)), rng.uniform(0.05, 0.95, len(k)), rng.uniform(0.05, 0.95, len(k))], axis=1).astype(F)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def long_runs(lengths, short=0, seed=0):
    """one voxel per entry of `lengths` (keys 0, 1, .. on the y axis) with that many points, plus `short` voxels of 3 points each,
    shuffled"""
    rng = np.random.default_rng(seed + sum(lengths))
    k = np.concatenate([np.repeat(np.arange(len(lengths)), lengths), np.repeat(np.arange(short) + 1000, 3)])
    pts = np.stack([rng.uniform(0.05, 0.95, len(k)), k + rng.uniform(0.05, 0.95, len(k)), rng.uniform(0.05, 0.95, len(k)) * 2.0 ** -20], axis=1).astype(F)
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


LONG_LENGTHS = (LONG_RUN - 1, LONG_RUN, LONG_RUN + 1)
WAVE_LENGTHS = (192, 193, 256, 257)         # all long: a wave's last trip of 64 points has exactly 64 of them, or one


@functools.lru_cache(maxsize=None)
def stream():
    """6 000 points over about 900 voxels (voxel_size 1), negative coordinates included, values of mixed magnitude"""
    rng = np.random.default_rng(99)
    pts = np.stack([rng.uniform(-15, 15, 6000), rng.uniform(-15, 15, 6000), rng.uniform(0.0, 1.0, 6000) * 10.0 ** rng.integers(-6, 1, 6000)], axis=1)
    return np.ascontiguousarray(pts.astype(F))


def cut(pts, size):
    return [pts[i:i + size] for i in range(0, len(pts), size)]


def random_cut(pts, seed=5):
    rng = np.random.default_rng(seed)
    out, i = [], 0
    while i < len(pts):
        n = int(rng.integers(1, 700))
        out.append(pts[i:i + n])
        i += n
    return out


def growth_steps():
    """chunks for a map created at MIN_CAPACITY slots, as (points, distinct voxels of the chunk all new, slots expected afterwards):
    V + R one below, at, and one above slots / 2 at the first doubling and again at the second; then three doublings in one insert"""
    half = MIN_CAPACITY // 2
    steps, base = [], 0
    for r, slots in ((half - 1, MIN_CAPACITY), (1, MIN_CAPACITY), (1, 2 * MIN_CAPACITY),                   # V + R = 127, 128, 129
                     (2 * half - (half + 1) - 1, 2 * MIN_CAPACITY), (1, 2 * MIN_CAPACITY), (1, 4 * MIN_CAPACITY),   # 255, 256, 257
                     (2 * MIN_CAPACITY * 4, 32 * MIN_CAPACITY)):                                             # 2 (257 + 2048) = 4610 > 1024 -> 8192
        k = np.arange(base, base + r)
        pts = np.stack([k % 64 + 0.5, k // 64 + 0.5, np.full(r, -0.5)], axis=1).astype(F)
        pts = np.concatenate([pts, pts[: max(1, r // 3)] + F(0.25)])            # some voxels get a second point
        steps.append((np.ascontiguousarray(pts), r, slots))
        base += r
    return steps
