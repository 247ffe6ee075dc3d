"""The case table of the quadric-error simplification tests (tests/test_qem_cpu.py on the checker alone, tests/test_gpu_qem.py on the
device against it): the smallest shapes at which each rule of include/threecrate_hip_qem.h can go wrong.  A case is
dict(vertices, faces, runs): every run is a config of tests/qem_checker.py."""
import numpy as np

from threecrate_amd import synth
from tests import qem_checker as K

F = np.float32
LONG_RING = 128                 # qem.hip's kQemLongRing as built: the cone's apexes lie above it
CONE_FACES = 200

# Quality against the reference's algorithm (test_qem_cpu.py): surface_error(checker) <= QUALITY_K * surface_error(literal) at the same
# target.  Measured on the CPU (checker / literal):
#   icosphere level 3      ratio 0.5: 0.74    ratio 0.9: 0.49
#   bumpy 32 x 32 field    ratio 0.5: 0.56    ratio 0.9: 0.32
# QUALITY_K is the worst of the four plus a quarter; the margin is for the tie order of `literal`, which is not the reference's own.
QUALITY_MEASURED = {("icosphere_3", 0.5): 0.74, ("icosphere_3", 0.9): 0.49, ("bumpy_32", 0.5): 0.56, ("bumpy_32", 0.9): 0.32}
QUALITY_K = 0.99


def case(vertices, faces, *runs):
    return {"vertices": np.ascontiguousarray(vertices, F).reshape(-1, 3), "faces": np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), "runs": list(runs)}


def tetrahedron(at=(0.0, 0.0, 0.0)):
    v = np.asarray([[0, 0, 0], [1, 0, 0], [0.3, 1, 0], [0.4, 0.3, 1.1]], F) + np.asarray(at, F)
    return v, np.asarray([[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], np.uint32)


def octahedron():
    v = np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1.25, 0], [0, -1.25, 0], [0, 0, 1.5], [0, 0, -1.5]], F)
    f = np.asarray([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)
    return v, f


def fan(k=12):
    """k flat triangles around vertex 0, open: every rim edge is blocked by a spoke of lower rank, so a round takes one collapse"""
    a = np.arange(k + 1) * (1.5 * np.pi / k)
    v = np.concatenate([[[0.0, 0.0, 0.0]], np.stack([np.cos(a), np.sin(a), 0 * a], axis=1)])
    return v.astype(F), np.asarray([[0, i + 1, i + 2] for i in range(k)], np.uint32)


def cone(k=CONE_FACES):
    """a closed double cone: apex 0 and apex 1 with k faces each over a ring of k vertices"""
    a = np.arange(k) * (2 * np.pi / k)
    ring = np.stack([np.cos(a), np.sin(a), 0.05 * np.sin(3 * a)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 1.0], [0.0, 0.0, -0.7]], ring])
    up = [[0, 2 + i, 2 + (i + 1) % k] for i in range(k)]
    down = [[1, 2 + (i + 1) % k, 2 + i] for i in range(k)]
    return v.astype(F), np.asarray(up + down, np.uint32)


def book():
    """three triangles on the edge (0, 1): multiplicity 3"""
    v = np.asarray([[0, 0, 0], [0, 2, 0], [1, 1, 0], [-0.5, 1, 0.9], [-0.5, 1, -0.9]], F)
    return v, np.asarray([[0, 1, 2], [0, 1, 3], [0, 1, 4]], np.uint32)


def two_components():
    """two tetrahedra and three vertices in no face: first, between and last"""
    va, fa = tetrahedron()
    vb, fb = tetrahedron((5.0, 0.0, 0.0))
    loose = np.asarray([[9, 9, 9]], F)
    v = np.concatenate([loose, va, loose + 1, vb, loose + 2])
    return v, np.concatenate([fa + 1, fb + 6]).astype(np.uint32)


def untidy():
    """an octahedron with faces that repeat an index and a face given twice"""
    v, f = octahedron()
    extra = np.asarray([[0, 0, 1], [2, 3, 2], [4, 4, 4]], np.uint32)
    return v, np.concatenate([extra[:1], f[:3], extra[1:2], f[:1], f[3:], extra[2:]])


def stretched(nx=7, ny=6):
    """a bumpy grid whose right half is three times as wide per cell: max_edge_length 1.5 rules that half out"""
    v, f = synth.bumpy_grid_mesh(nx, ny, amplitude=0.2, waves=1.0, spacing=1.0)
    x = v[:, 0].astype(np.float64)
    v[:, 0] = np.where(x > 3, 3 + (x - 3) * 3, x).astype(F)
    return v, f


def build():
    cases = {}
    cases["tetrahedron"] = case(*tetrahedron(), K.config(0.5), K.config(1.0))
    cases["octahedron"] = case(*octahedron(), K.config(0.5), K.config(0.25, 0))
    cases["octahedron_odd"] = case(*octahedron(), K.config(0.375))                     # target 5: alive - target = 3 is odd
    grid = synth.grid_mesh(5, 5)
    cases["flat_grid_boundary"] = case(*grid, K.config(0.5, 1), K.config(1.0, 1))
    cases["flat_grid_open"] = case(*grid, K.config(0.5, 0), K.config(1.0, 0))
    ico = synth.icosphere(3)
    cases["icosphere_3"] = case(*ico, K.config(0.1), K.config(0.5), K.config(0.9), K.config(1.0))
    cases["fan_12"] = case(*fan(), K.config(0.5, 0), K.config(1.0, 0), K.config(0.5, 1))
    cases[f"cone_{CONE_FACES}"] = case(*cone(), K.config(0.5), K.config(0.9, 0))
    cases["book"] = case(*book(), K.config(0.5, 0), K.config(0.5, 1))
    cases["two_components"] = case(*two_components(), K.config(0.5), K.config(1.0, 0))
    cases["untidy"] = case(*untidy(), K.config(0.5), K.config(0.01))
    cases["stretched_max_edge"] = case(*stretched(), K.config(0.9, 0, 1.5), K.config(0.9, 0, 0.0))
    # a gently curved patch 1e4 away from the origin: the f32 plane term d is large and its rounding shows in costs of both signs
    v, f = synth.bumpy_grid_mesh(12, 12, amplitude=0.01, waves=1.0, spacing=0.05)
    cases["offset_1e4"] = case(v + F(1e4), f, K.config(0.5, 0), K.config(0.9, 1))
    cases["field_128"] = case(*synth.bumpy_grid_mesh(128, 128, amplitude=0.1, waves=4.0), K.config(0.9))
    return cases


CASES = build()

# quality shapes (curved everywhere: det well away from 0)
QUALITY = {"icosphere_3": synth.icosphere(3), "bumpy_32": synth.bumpy_grid_mesh(32, 32, amplitude=0.1, waves=2.0)}

# (name, vertices, faces, config, status, message): the checks found after the pointer checks, in the header's order
_tv, _tf = tetrahedron()
_nan = _tv.copy()
_nan[2, 1] = np.nan
_inf = _tv.copy()
_inf[0, 0] = np.inf
_bad = _tf.copy()
_bad[3, 2] = 4
LIMITS = [
    ("preserve_boundary", _tv, _tf, K.config(2.0, 2), K.INVALID_DATA, "preserve_boundary"),
    ("ratio above", _tv, _tf, K.config(1.5, 1, -1.0), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("ratio below", _tv, _tf, K.config(-0.1), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("ratio nan", _tv, _tf, K.config(float("nan")), K.INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0"),
    ("max_edge_length negative", _tv, _bad, K.config(0.5, 1, -1.0), K.INVALID_DATA, "max_edge_length"),
    ("max_edge_length nan", _nan, _tf, K.config(0.5, 1, float("nan")), K.INVALID_DATA, "max_edge_length"),
    ("bad index", _tv, _bad, K.config(0.5), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("bad index, ratio 0", _tv, _bad, K.config(0.0), K.INVALID_DATA, "a face index is >= n_vertices"),
    ("nan", _nan, _tf, K.config(0.5), K.INVALID_DATA, "a vertex coordinate is not finite"),
    ("inf, ratio 0", _inf, _tf, K.config(0.0), K.INVALID_DATA, "a vertex coordinate is not finite"),
]
