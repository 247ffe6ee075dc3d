"""The case table of the mesh simplification tests: read by tests/test_simplify_cpu.py (the checker against the literal restatement of
the reference, the proofs that a case holds what it is there for, the mutants) and by tests/test_gpu_simplify.py (the device against
the checker, bit for bit).  Every mesh is small but wide_keys, which has to pass 2^21 vertices to reach the two-pass face sort.
A case is {"vertices", "faces", "normals" | None, "colors" | None, "runs": [parameters, ...], "literal": bool}; a run's parameters are
the keyword arguments of simplify_checker.simplify."""
import os
import re

import numpy as np

from tests import simplify_checker as K
from threecrate_amd import synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_CLUSTER = int(re.search(r"constexpr uint32_t kSimplifyLongCluster = (\d+);",
                             open(os.path.join(ROOT, "threecrate_amd", "csrc", "simplify.hip")).read()).group(1))
PI = float(F(np.pi))
CENTROID, WEIGHTED = 0, 1

CASES = {}


def run(ratio, strategy=CENTROID, preserve_boundary=1, threshold=K.DEFAULT_ANGLE):
    return dict(ratio=ratio, strategy=strategy, preserve_boundary=preserve_boundary, threshold=threshold)


BOTH = lambda ratio, **kw: [run(ratio, CENTROID, **kw), run(ratio, WEIGHTED, **kw)]


def case(name, vertices, faces, runs, normals=None, colors=None, literal=True):
    assert name not in CASES
    CASES[name] = {"vertices": np.ascontiguousarray(vertices, F).reshape(-1, 3), "faces": np.ascontiguousarray(faces, np.uint32).reshape(-1, 3),
                   "normals": None if normals is None else np.ascontiguousarray(normals, F).reshape(-1, 3),
                   "colors": None if colors is None else np.ascontiguousarray(colors, np.uint8).reshape(-1, 3), "runs": runs, "literal": literal}


def attributes(n, seed):
    """normals and colours with no pattern: (n, 3) f32 spanning a few binades, (n, 3) u8"""
    u = synth.splitmix_u01(seed, np.arange(6 * n, dtype=np.uint64)).reshape(n, 6)
    nrm = ((u[:, :3] - F(0.5)) * np.ldexp(F(1.0), (np.arange(n) * 7 % 9) - 4).astype(F)[:, None]).astype(F)
    return nrm, np.floor(u[:, 3:] * F(256.0)).astype(np.uint8)


# ---- reference: the unit-test meshes of clustering.rs:837-933, at its ratios ----
def plane_grid(size, height=None):
    """make_plane_grid / make_curved_surface: faces (tl, bl, tr), (tr, bl, br)"""
    y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(size), np.arange(size), indexing="ij"))
    z = np.zeros(size * size, F) if height is None else height(x.astype(F), y.astype(F))
    cy, cx = np.divmod(np.arange((size - 1) ** 2), size - 1)
    tl = cy * size + cx
    faces = np.stack([np.stack([tl, tl + size, tl + 1], axis=1), np.stack([tl + 1, tl + size, tl + size + 1], axis=1)], axis=1).reshape(-1, 3)
    return np.stack([x.astype(F), y.astype(F), z.astype(F)], axis=1), faces


def curved(size):
    h = lambda x, y: (np.sin(x / F(size - 1) * F(np.pi)).astype(F) * np.sin(y / F(size - 1) * F(np.pi)).astype(F)) * F(2.0)
    return plane_grid(size, h)


TRIANGLE = ([[0, 0, 0], [1, 0, 0], [0.5, 1, 0]], [[0, 1, 2]])
TETRAHEDRON = ([[0, 0, 0], [1, 0, 0], [0.5, 1, 0], [0.5, 0.5, 1]], [[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]])
SHARP_V = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0], [0, 1, 1], [1, 1, 1], [2, 1, 1]]
SHARP_F = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [3, 4, 6], [4, 7, 6], [4, 5, 7], [5, 8, 7]]
REF_RUNS = BOTH(0.3) + BOTH(0.5) + [run(0.5, CENTROID, 0, PI)]
case("reference_triangle", *TRIANGLE, REF_RUNS)
case("reference_tetrahedron", *TETRAHEDRON, REF_RUNS)
case("reference_plane_6", *plane_grid(6), REF_RUNS)
case("reference_plane_11", *plane_grid(11), REF_RUNS)
case("reference_curved_8", *curved(8), REF_RUNS)
case("reference_sharp_edge", SHARP_V, SHARP_F, REF_RUNS)
case("reference_plane_5_attributes", *plane_grid(5), [run(0.3)], normals=np.tile(F([0, 0, 1]), (25, 1)), colors=np.tile(np.uint8([128, 64, 200]), (25, 1)))


# ---- blocks: vertex counts either side of a 256-thread block; 257 is prime: the 128 x 2 strip and one unreferenced vertex ----
def strip(n_vertices):
    for ny in (3, 5):
        if n_vertices % ny == 0:
            return synth.grid_mesh(n_vertices // ny, ny, 0.5, seed=n_vertices)
    if n_vertices % 2 == 0:
        return synth.grid_mesh(n_vertices // 2, 2, 0.5, seed=n_vertices)
    v, f = synth.grid_mesh((n_vertices - 1) // 2, 2, 0.5, seed=n_vertices)
    return np.concatenate([v, [[-1.0, -2.0, 0.25]]]).astype(F), f


BLOCKS = (255, 256, 257, 513)
for n in BLOCKS:
    v, f = strip(n)
    nrm, col = attributes(n, n)
    case(f"blocks_{n}", v, f, BOTH(0.5) + [run(0.9, WEIGHTED, 0)], normals=nrm, colors=col)
# an unreferenced vertex INSIDE the grid: valence 0 in a cluster with others
v, f = synth.grid_mesh(12, 10, 0.0)
case("blocks_unreferenced_inside", np.concatenate([v, [[5.3, 4.2, 0.0]]]).astype(F), f, BOTH(0.9) + BOTH(0.9, preserve_boundary=0))
# face counts either side of 256: 65 x 3 gives 256 faces; one fewer and one more by dropping and repeating the last
v, f = synth.grid_mesh(65, 3, 0.5, seed=9)
case("blocks_faces_255", v, f[:-1], BOTH(0.5))
case("blocks_faces_256", v, f, BOTH(0.5))
case("blocks_faces_257", v, np.concatenate([f, f[-1:]]), BOTH(0.5))


# ---- cluster_sizes: a fan whose `size` apex vertices share one cell; B and C have cells of their own.  At ratio 1 the planar unit box
# has cell = 1: the apexes (inside [0, 0.4]^2) are cell (0, 0), B = (1, 0, 0) is cell (1, 0), C = (0, 1, 0) is cell (0, 1).  Every face
# (A_i, B, C) maps to the same triple.  The apex coordinates span 40 binades with both signs, so the order of an f64 fold shows ----
def apex_fan(size, seed=5):
    u = synth.splitmix_u01(seed, np.arange(3 * size, dtype=np.uint64)).reshape(size, 3)
    k = np.arange(size)
    scale = np.ldexp(F(0.2), -(k * 11 % 40)).astype(F)
    a = ((F(1.0) + u) * scale[:, None]).astype(F)
    a[:, 2] = 0.0
    a[0, :2] = 0.0                                       # the box's corner
    v = np.concatenate([a, F([[1, 0, 0], [0, 1, 0]])])
    f = np.stack([k, np.full(size, size), np.full(size, size + 1)], axis=1)
    return v, f


CLUSTER_SIZES = sorted({1, 2, 3, 4, 5, 63, 64, 65, LONG_CLUSTER - 1, LONG_CLUSTER, LONG_CLUSTER + 1, 192, 193, 256, 257, 4097})
for s in CLUSTER_SIZES:
    v, f = apex_fan(s)
    nrm, col = attributes(s + 2, 100 + s)
    case(f"cluster_sizes_{s}", v, f, BOTH(1.0, preserve_boundary=0, threshold=PI), normals=nrm, colors=col, literal=s <= 300)
# five long clusters among forty short ones.  1 224 vertices in the planar box [0, 8.5] x [0, 4.5] at ratio 31 / 32: (1 - ratio) n = 38.25 =
# 8.5 x 4.5 exactly in f32, so the cell is exactly 1 and the clusters are the 9 x 5 unit cells.  Cells 4, 13, 22, 31, 40 (row-major) hold
# FIVE_LONG members, the others 5 or 4; the vertex order is shuffled, so the members of every cluster are scattered over the index range
FIVE_LONG = (LONG_CLUSTER + 1, 192, 193, 256, 257)


def five_long_clusters():
    counts = np.full(45, 5)
    counts[[4, 13, 22, 31, 40]] = FIVE_LONG
    counts[[0, 1, 2]] = 4
    n = int(counts.sum())
    cell = np.repeat(np.arange(45), counts)
    u = synth.splitmix_u01(77, np.arange(2 * n, dtype=np.uint64)).reshape(n, 2)
    xy = np.stack([cell % 9, cell // 9], axis=1).astype(F) + (F(0.05) + F(0.4) * u).astype(F)
    xy[0] = 0.0                                          # the box's corners: cell 0 and cell 44
    xy[-1] = F([8.5, 4.5])
    order = np.random.default_rng(7).permutation(n)
    v = np.concatenate([xy, np.zeros((n, 1), F)], axis=1)[order]
    k = np.arange(n)
    return v, np.stack([k, (k + 1) % n, (k + 2) % n], axis=1), counts


v, f, _ = five_long_clusters()
assert len(v) == 1224
nrm, col = attributes(len(v), 1224)
case("cluster_sizes_five_long", v, f, BOTH(0.96875, preserve_boundary=0, threshold=PI), normals=nrm, colors=col, literal=False)
# ratio 1 on a flat square grid: the cell is the box's edge, so everything but the two far rims is one cell, split by class
case("cluster_sizes_ratio_1_grid", *synth.grid_mesh(33, 33, 0.0), BOTH(1.0) + BOTH(1.0, preserve_boundary=0))
# two of a triangle's corners in one cell (a line of extent 1 at ratio 1 has cell 1): its only face is degenerate and the output is empty
case("cluster_sizes_zero_faces", [[0, 0, 0], [0.125, 0, 0], [1, 0, 0]], [[0, 1, 2]], [run(1.0, CENTROID, 0, PI)])

# ---- classes: the welded box (dihedral dots exactly 0 across its edges, exactly 1 inside a side), with one side removed, thresholds whose
# cosf lies either side of those dots, preserve_boundary on and off ----
HALF_PI = float(F(np.pi) / F(2.0))
BELOW_HALF_PI = float(np.nextafter(F(HALF_PI), F(0.0)))
CLASS_THRESHOLDS = {"default": K.DEFAULT_ANGLE, "half_pi": HALF_PI, "below_half_pi": BELOW_HALF_PI, "zero": 0.0, "tiny": 1e-3, "pi": PI}
for name, (v, f, nrm) in {"box": synth.box_mesh(4), "open_box": synth.box_mesh(4, open_side=True)}.items():
    _, col = attributes(len(v), 7)
    case(f"classes_{name}", v, f, [run(r, s, pb, t) for r in (0.5, 0.9) for s in (CENTROID, WEIGHTED) for pb in (0, 1) for t in CLASS_THRESHOLDS.values()],
         normals=nrm, colors=col)

# ---- faces: every face twice; the second copy reversed (dot exactly -1 across every edge: four incidences, and pi's cosf is exactly -1);
# faces that repeat an index ----
v, f = synth.grid_mesh(9, 7, 0.5, seed=4)
case("faces_twice", v, np.concatenate([f, f]), BOTH(0.5) + BOTH(0.3))
case("faces_twice_interleaved_reversed", v, np.stack([f, f[:, ::-1]], axis=1).reshape(-1, 3), BOTH(0.5) + BOTH(0.3))
case("faces_reversed_first", v, np.concatenate([f[:, ::-1], f]), BOTH(0.5))
case("faces_open_pair", [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.5]], [[0, 1, 2], [2, 1, 0]], [run(0.3, CENTROID, 1, PI), run(0.3, CENTROID, 1, 3.0)])
case("faces_repeated_index", v, np.concatenate([f[:20], [[0, 0, 1], [5, 5, 5], [3, 4, 3], [10, 11, 10]], f[20:]]), BOTH(0.5) + BOTH(0.3))

# ---- degenerate_box: dim 0, 1, 2, and one extent either side of 1e-6 ----
case("degenerate_box_point", np.tile(F([[0.5, -2, 3]]), (7, 1)), [[0, 1, 2], [2, 3, 4], [4, 5, 6]], BOTH(0.5))
line = np.stack([np.arange(12, dtype=F) * F(0.37), np.full(12, 2, F), np.full(12, -1, F)], axis=1)
case("degenerate_box_line", line, [[i, i + 1, i + 2] for i in range(10)], BOTH(0.5) + BOTH(0.9))
case("degenerate_box_plane", *plane_grid(9), BOTH(0.6))
for tag, dz in (("below", 9.5e-7), ("above", 1.5e-6)):
    v, f = plane_grid(9)
    v[::2, 2] = dz
    case(f"degenerate_box_extent_{tag}", v, f, BOTH(0.6))

# an extent of exactly 1e-6 (the f64): z is either f32(1e-6) or what is missing from it, which is an f32 as well
Z_HI = F(1e-6)
Z_LO = F(float(Z_HI) - 1e-6)
assert float(Z_HI) - float(Z_LO) == 1e-6
v, f = plane_grid(9)
v[:, 2] = np.where(np.arange(81) % 2 == 0, Z_HI, Z_LO)
case("degenerate_box_extent_equal", v, f, BOTH(0.6))
# f32 target: ten vertices at ratio 0.3 have target f32(0.7f * 10) = 7.0 where the f64 product is 6.99999988; on a line of extent 7 the cell is
# exactly 1.0 and the integer positions sit on the cell borders
line10 = np.stack([F([0, 0.5, 1, 1.5, 2, 3, 4, 5, 6, 7]), np.zeros(10, F), np.zeros(10, F)], axis=1)
case("degenerate_box_line_target", line10, [[i, i + 1, i + 2] for i in range(8)], BOTH(0.3, preserve_boundary=0, threshold=PI))

# ---- shifted: a grid snapped to 2^-7, moved by 2^10 and 2^16: the f64 cell arithmetic is exact either way, the clusters are the unmoved run's ----
v, f = synth.grid_mesh(23, 17, 0.8, seed=6)
SNAPPED = (np.round(v * F(128.0)) / F(128.0)).astype(F)
SHIFTS = (0.0, 1024.0, 65536.0)
for sh in SHIFTS:
    case(f"shifted_{int(sh)}", SNAPPED + F([sh, -sh, sh]), f, BOTH(0.7))

# ---- attributes: normals that cancel inside a cluster, colours 255 everywhere; either, both, neither ----
v, f = synth.grid_mesh(16, 12, 0.5, seed=8)
cancel = np.tile(F([[0, 0, 1], [0, 0, -1]]), (len(v) // 2, 1))
white = np.full((len(v), 3), 255, np.uint8)
case("attributes_both", v, f, BOTH(0.95, preserve_boundary=0, threshold=PI), normals=cancel, colors=white)
case("attributes_normals", v, f, BOTH(0.95, preserve_boundary=0, threshold=PI), normals=cancel)
case("attributes_colors", v, f, BOTH(0.95, preserve_boundary=0, threshold=PI), colors=attributes(len(v), 3)[1])
case("attributes_neither", v, f, BOTH(0.95, preserve_boundary=0, threshold=PI))

# ---- wide_keys: more than 2^21 vertices, so three cluster numbers do not fit one 64-bit key: the two-pass face sort.  Only the faces of
# the last hundred columns are kept (the checker's edge sort is what costs); their clusters are numbered beyond 2^21 ----
WIDE_N = 1800


def wide_keys():
    v, f = synth.grid_mesh(WIDE_N, WIDE_N, 0.0)
    keep = (f % WIDE_N >= WIDE_N - 100).all(axis=1)
    f = f[keep]
    return v, np.concatenate([f, f[:1000, ::-1]]), run(0.3)          # a thousand faces again, reversed: repeated triples on this road too


# ---- limits: the order of checks.  (name, vertices, faces, parameters, status, message) ----
GRID_V, GRID_F = synth.grid_mesh(6, 5, 0.5, seed=1)
SLIVER_V = np.concatenate([GRID_V * F([1, 1, 0]) * F([1.0, 2e-6, 1.0]), F([[3e6, 0, 0]])]).astype(F)       # 3e6 x 8e-6: cell 4e-3 at ratio 0.5


def with_coordinate(value):
    v = GRID_V.copy()
    v[7, 1] = value
    return v


def with_index(value):
    f = GRID_F.copy()
    f[3, 2] = value
    return f


LIMITS = [
    ("ratio_negative", GRID_V, GRID_F, run(-0.1), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("ratio_above_one", GRID_V, GRID_F, run(1.1), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("ratio_nan", GRID_V, GRID_F, run(float("nan")), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("threshold_inf", GRID_V, GRID_F, run(0.5, threshold=float("inf")), K.INVALID_DATA, "feature_angle_threshold is not finite"),
    ("ratio_before_threshold", GRID_V, GRID_F, run(1.5, threshold=float("nan")), K.INVALID_DATA, "Reduction ratio"),
    ("index_equal_n", GRID_V, with_index(len(GRID_V)), run(0.5), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("index_equal_n_ratio_0", GRID_V, with_index(len(GRID_V)), run(0.0), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("index_max", GRID_V, with_index(0xFFFFFFFF), run(0.5), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("coordinate_nan", with_coordinate(np.nan), GRID_F, run(0.5), K.INVALID_DATA, "a vertex coordinate is not finite"),
    ("coordinate_inf", with_coordinate(np.inf), GRID_F, run(0.5), K.INVALID_DATA, "a vertex coordinate is not finite"),
    ("coordinate_inf_ratio_0", with_coordinate(-np.inf), GRID_F, run(0.0), K.INVALID_DATA, "a vertex coordinate is not finite"),
    ("index_before_coordinate", with_coordinate(np.nan), with_index(99), run(0.5), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("ratio_before_index", GRID_V, with_index(99), run(2.0), K.INVALID_DATA, "Reduction ratio"),
    ("sliver", SLIVER_V, GRID_F, run(0.5), K.UNSUPPORTED, "a cell index does not fit 20 bits"),
    ("coordinate_before_sliver", np.concatenate([SLIVER_V, F([[np.nan, 0, 0]])]), GRID_F, run(0.5), K.INVALID_DATA, "a vertex coordinate is not finite"),
]
