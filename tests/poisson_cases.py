"""The case table of the Poisson surface, read by tests/test_poisson_cpu.py (the checker alone) and tests/test_gpu_poisson.py (the device).
A case: points, normals (f32), cfg (tests/poisson_checker.config), family.  MEASURED holds what the CPU twin measured on the checker and
asserts again on every run: per case the distance between the checker's exact and f64 modes (chi in the relative max-norm, the iso value
relative to max |chi|), per sphere depth the radial bound of the f64 checker's mesh, and plane_patch's min_density.  The device's budgets
are derived from these numbers, never from the device."""
import functools

import numpy as np

from tests import poisson_checker as PC

F = np.float32
RADIUS = 0.5


def sphere(n, shift=0.0, seed=None):
    """n points on the sphere of radius 0.5 (a Fibonacci spiral; seeded jitter of the order when seed is given), outward normals"""
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    phi = k * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), z], 1)
    if seed is not None:
        d = d[np.random.default_rng(seed).permutation(n)]
    nrm = d.astype(F)
    return (RADIUS * d + shift).astype(F), nrm


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def faces_cloud(depth):
    """Points of the box [0, N - 1]^3 with scale 1: h = 1 and origin = 0 exactly, so integer coordinates are nodes and half-integers cell
    faces / centres.  The eight corners and the face centres (g = N - 1: the clamp with f = 1), every node of the boundary, and points
    with one integer coordinate (on a cell face).  Normals point away from the centre."""
    N = 1 << depth
    t = float(N - 1)
    ax = np.arange(N, dtype=np.float64)
    nodes = np.array([(x, y, z) for z in ax for y in ax for x in ax if 0 in (x, y, z) or t in (x, y, z)])
    half = ax[:-1] + 0.5
    onface = np.array([(x, y, z) for x in ax for y in half for z in half] + [(y, x, z) for x in ax for y in half for z in half] +
                      [(y, z, x) for x in ax for y in half for z in half])
    corners = np.array([(x, y, z) for x in (0, t) for y in (0, t) for z in (0, t)])
    pts = np.concatenate([corners, nodes, onface])
    pts = pts[np.abs(pts - t / 2).max(1) > 1e-9]                 # (the centre has no direction)
    return pts.astype(F), _unit(pts - t / 2)


def dense_node_cloud():
    """6 000 points inside one cell of the depth-3 grid of a sphere of 500 (a node gets thousands of records), random unit normals"""
    rng = np.random.default_rng(11)
    p, q = sphere(500)
    origin, h, _ = PC.grid_of(p, 3, 1.1)
    lo = origin.astype(np.float64) + 3.0 * float(h)
    inner = lo + rng.uniform(0.05, 0.95, (6000, 3)) * float(h)
    pts = np.concatenate([inner, p.astype(np.float64)])
    nrm = np.concatenate([_unit(rng.normal(size=(6000, 3))), q])
    perm = rng.permutation(len(pts))
    return pts[perm].astype(F), nrm[perm]


def duplicates_cloud():
    p, q = sphere(300)
    return np.repeat(p, 8, 0), np.repeat(q, 8, 0)


def plane_patch_cloud():
    """an open surface: a gently curved patch over [-0.5, 0.5]^2, 40 x 40 points, normals up"""
    u = np.linspace(-0.5, 0.5, 40)
    x, y = np.meshgrid(u, u, indexing="ij")
    z = 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)
    gx, gy = 0.3 * np.cos(3.0 * x) * np.cos(2.0 * y), -0.2 * np.sin(3.0 * x) * np.sin(2.0 * y)
    pts = np.stack([x, y, z], -1).reshape(-1, 3)
    return pts.astype(F), _unit(np.stack([-gx, -gy, np.ones_like(gx)], -1).reshape(-1, 3))


# what the CPU twin measured (tests/test_poisson_cpu.py asserts each again): name -> (chi distance, iso distance, exact iterations)
MEASURED = {
    "sphere_d3_pw0": (2.3409648046224933e-07, 4.586706430900649e-09, 17), "sphere_d3_pw2": (3.251812111615688e-07, 2.559152595252929e-09, 22),
    "sphere_d4_pw0": (5.722735678211672e-07, 2.6609583012265193e-08, 34), "sphere_d4_pw2": (3.383560825256616e-07, 1.0480717817616113e-09, 31),
    "sphere_d5_pw0": (5.801148014363672e-07, 1.136343237059456e-08, 61), "sphere_d5_pw2": (5.174893058700268e-07, 5.2028609646656276e-09, 48),
    "faces_d2": (1.4637134364458994e-07, 3.785448680585903e-08, 4), "faces_d3": (1.9000812261040348e-07, 5.237221972262358e-08, 14),
    "small_10": (1.2886475577891863e-07, 3.150352253298371e-08, 12), "small_11": (9.728865952443717e-08, 2.4829445737639635e-10, 12),
    "blocks_255": (3.7195179707540165e-07, 9.906543686904645e-09, 20), "blocks_256": (3.8559847216478865e-07, 2.0274422623582955e-08, 20),
    "blocks_257": (2.429172036672957e-07, 3.1240010198584143e-09, 20), "blocks_513": (3.530170874548878e-07, 2.170937550184037e-08, 19),
    "blocks_4097": (2.9988748015630065e-07, 1.3002809337339478e-08, 19), "dense_node": (2.1230848096134287e-07, 4.516462894978489e-08, 24),
    "duplicates": (2.425614756510502e-07, 2.760480956810643e-08, 20), "plane_patch": (4.2504990413443835e-07, 2.9136663544138538e-08, 31),
    "shifted": (3.0740735040324093e-07, 5.836469743980823e-09, 17),
}
# sphere depth -> the largest | |v| - 0.5 | over the f64 checker's welded mesh at point_weight 0 and 2
RADIAL = {3: 0.035540133166122145, 4: 0.006206676567017788, 5: 0.006676951738507131}
# plane_patch: the median of the checker's positive densities, as an f32 literal
PLANE_MIN_DENSITY = 2.3650002479553223


@functools.lru_cache(maxsize=None)
def _table():
    t = {}
    add = lambda name, family, pn, **cfg: t.__setitem__(name, dict(name=name, family=family, points=pn[0], normals=pn[1], cfg=PC.config(**cfg)))
    for depth in (3, 4, 5):
        for pw in (0.0, 2.0):
            # (depth 5 stops at 2e-5: at 1e-5 both of its cases end within 10 % of the tolerance)
            add(f"sphere_d{depth}_pw{int(pw)}", "sphere", sphere(2000), depth=depth, point_weight=pw, tolerance=2e-5 if depth == 5 else 1e-5)
    add("sphere_d6", "sphere6", sphere(2000), depth=6, max_iterations=40)
    for depth in (2, 3):
        add(f"faces_d{depth}", "faces", faces_cloud(depth), depth=depth, scale=1.0)
    for n in (10, 11):
        p, q = sphere(64)
        add(f"small_{n}", "small", (p[:n], q[:n]), depth=2)
    for n in (255, 256, 257, 513, 4097):
        add(f"blocks_{n}", "blocks", sphere(n), depth=3)
    add("dense_node", "dense_node", dense_node_cloud(), depth=3)
    add("duplicates", "duplicates", duplicates_cloud(), depth=3)
    add("plane_patch", "plane_patch", plane_patch_cloud(), depth=4, min_density=PLANE_MIN_DENSITY)
    add("shifted", "shifted", sphere(2000, shift=1024.0), depth=3)
    return t


def names(family=None):
    return [k for k, c in _table().items() if family is None or c["family"] == family]


def case(name):
    return _table()[name]


@functools.lru_cache(maxsize=None)
def expected(name, mode="exact"):
    """the checker's result for a case, computed once and shared; treat as read-only"""
    c = case(name)
    return PC.run(c["points"], c["normals"], c["cfg"], mode)


# the depth-8 smoke of the loop alone: three iterations, compared with the checker's exact mode at the same three
def depth8():
    p, q = sphere(2000)
    return dict(name="depth8", points=p, normals=q, cfg=PC.config(depth=8, max_iterations=3))


def bad_inputs():
    """name -> (points, normals, cfg, accepted)"""
    p, q = sphere(64)
    out = {}
    nan = p.copy(); nan[5, 1] = np.nan
    out["nan_coordinate"] = (nan, q, PC.config(depth=3), False)
    for length, ok in ((0.0, False), (0.85, False), (1.15, False), (0.95, True), (1.05, True)):
        s = q.copy(); s[7] = s[7] * F(length)
        out[f"normal_{length}"] = (p, s, PC.config(depth=3), ok)
    out["identical_points"] = (np.repeat(p[:1], 16, 0), q[:16], PC.config(depth=3), False)
    out["nine_points"] = (p[:9], q[:9], PC.config(depth=2), False)
    out["depth_1"] = (p, q, PC.config(depth=1), False)
    out["depth_9"] = (p, q, PC.config(depth=9), False)
    out["scale_0.5"] = (p, q, PC.config(depth=3, scale=0.5), False)
    return out
