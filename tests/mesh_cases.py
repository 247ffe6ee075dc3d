"""The case table of the mesh smoothing tests: read by tests/test_mesh_cpu.py (the checker against itself, its mutants) and by
tests/test_gpu_mesh.py (the device against the checker, bit for bit).  Every mesh is small; the largest is the 65 537-vertex key_bits case.
A case is {"vertices": (n, 3) f32, "faces": (m, 3) u32, "runs": [(method, parameters), ...]}."""
import os
import re

import numpy as np

from tests import mesh_checker as K
from threecrate_amd import synth

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_RING = int(re.search(r"constexpr uint32_t kMeshLongRing = (\d+);", open(os.path.join(ROOT, "threecrate_amd", "csrc", "mesh.hip")).read()).group(1))
METHODS = {"laplacian": K.LAPLACIAN, "taubin": K.TAUBIN, "hc": K.HC}
ALL_DEFAULT = [(m, {}) for m in METHODS]


def all_with(**params):
    return [(m, dict(params)) for m in METHODS]


CASES = {}


def case(name, vertices, faces, runs):
    assert name not in CASES
    CASES[name] = {"vertices": np.ascontiguousarray(vertices, F).reshape(-1, 3), "faces": np.ascontiguousarray(faces, np.uint32).reshape(-1, 3), "runs": runs}


# ---- the reference's two test meshes (mesh_smoothing.rs:298-321, :398-422) ----
SPIKE_V = [[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [1, 1, 1], [2, 1, 0], [0, 2, 0], [1, 2, 0], [2, 2, 0]]
SPIKE_F = [[0, 1, 3], [1, 4, 3], [1, 2, 4], [2, 5, 4], [3, 4, 6], [4, 7, 6], [4, 5, 7], [5, 8, 7]]
BOX_V = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]]
BOX_F = [[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [3, 7, 6], [3, 6, 2], [0, 4, 7], [0, 7, 3], [1, 2, 6], [1, 6, 5]]
case("spike", SPIKE_V, SPIKE_F, ALL_DEFAULT)
case("box", BOX_V, BOX_F, ALL_DEFAULT)


# ---- block_edges: vertex counts either side of a 256-thread block, strips nx x 2 and nx x 3 ----
# 257 is prime, so it is no strip: the 128 x 2 strip with one unreferenced vertex behind it
def strip(n_vertices):
    for ny in (2, 3):
        if n_vertices % ny == 0:
            return synth.grid_mesh(n_vertices // ny, ny, 0.5, seed=n_vertices)
    v, f = synth.grid_mesh((n_vertices - 1) // 2, 2, 0.5, seed=n_vertices)
    return np.concatenate([v, [[-1.0, -2.0, 0.25]]]).astype(F), f


BLOCK_EDGES = (4, 255, 256, 257, 513)
for n in BLOCK_EDGES:
    case(f"block_edges_{n}", *strip(n), ALL_DEFAULT)
EMPTY_STRIP = synth.grid_mesh(1, 2, 0.5)                # two vertices, no face possible: "Mesh is empty"

# ---- iterations: both parities of the ping-pong and the copy road ----
ITERATIONS = (0, 1, 2, 3, 10)
for it in ITERATIONS:
    case(f"iterations_{it}", *synth.grid_mesh(7, 5, 0.5, seed=3), all_with(iterations=it))


# ---- rings: one hub fan; the rim's coordinates span twelve binades with both signs, so the order of the fold shows in the bits ----
def fan(ring, hub_at, seed=5):
    """ring + 1 vertices, the hub at index hub_at; faces (hub, rim k, rim k + 1), closed when ring >= 3; ring 1 is the face (hub, a, a)"""
    n = ring + 1
    u = synth.splitmix_u01(seed, np.arange(3 * n, dtype=np.uint64)).reshape(n, 3)
    k = np.arange(n)
    scale = np.ldexp(F(1.0), (k * 5 % 12) - 4).astype(F) * np.where(k % 3 == 0, F(-1.0), F(1.0))
    v = ((F(1.0) + u) * scale[:, None]).astype(F)
    rim = np.array([i for i in range(n) if i != hub_at], np.uint32)
    if ring == 1:
        f = [[hub_at, rim[0], rim[0]]]
    elif ring == 2:
        f = [[hub_at, rim[0], rim[1]]]
    else:
        f = np.stack([np.full(ring, hub_at, np.uint32), rim, np.roll(rim, -1)], axis=1)
    return v, np.asarray(f, np.uint32)


RING_SIZES = sorted({1, 2, 63, 64, 65, 127, 128, 129, LONG_RING - 1, LONG_RING, LONG_RING + 1, 192, 193, 256, 257, 4097})
HUB_AT = {"first": lambda n: 0, "middle": lambda n: n // 2, "last": lambda n: n - 1}
for ring in RING_SIZES:
    for where, at in HUB_AT.items():
        case(f"rings_{ring}_{where}", *fan(ring, at(ring + 1)), all_with(iterations=2))


def two_hubs(ring=LONG_RING + 36):
    """two fans side by side whose hubs (vertices 0 and 1) are joined by a face: each hub is in the other's (long) ring"""
    va, fa = fan(ring, 0, seed=7)
    vb, fb = fan(ring, 0, seed=8)
    v = np.concatenate([va[:1], vb[:1], va[1:], vb[1:]])
    ma = np.concatenate([[0], 2 + np.arange(ring)]).astype(np.uint32)
    mb = np.concatenate([[1], 2 + ring + np.arange(ring)]).astype(np.uint32)
    return v, np.concatenate([ma[fa], mb[fb], [[0, 1, 2]]]).astype(np.uint32)


case("rings_two_hubs", *two_hubs(), all_with(iterations=3))

FIVE_HUBS = (LONG_RING + 1, 192, 193, 256, 257)


def five_hubs(short=40, short_ring=5):
    """45 separate fans in vertex order, every hub first in its fan: eight of ring 5, then one of FIVE_HUBS, five times over -- five listed
    vertices for the wave-per-vertex kernel between vertices that a lane folds"""
    vs, fs, hubs, base = [], [], [], 0
    rings = [ring for long in FIVE_HUBS for ring in [short_ring] * (short // len(FIVE_HUBS)) + [long]]
    for k, ring in enumerate(rings):
        v, f = fan(ring, 0, seed=20 + k)
        vs.append(v); fs.append(f + np.uint32(base)); hubs.append(base)
        base += ring + 1
    return np.concatenate(vs), np.concatenate(fs).astype(np.uint32), np.array(hubs), np.array(rings)


case("rings_five_hubs", *five_hubs()[:2], all_with(iterations=2))

# ---- key_bits: a change of b, long runs of unreferenced vertices, the largest index in both key halves ----
KEY_BITS = (255, 256, 257, 65535, 65536, 65537)
for n in KEY_BITS:
    r = np.random.default_rng(n)
    special = np.array([0, n // 2, n - 1])
    f = np.concatenate([r.choice(special, (12, 3)), np.stack([r.choice(special, 24), r.integers(0, n, 24), r.integers(0, n, 24)], axis=1),
                        [[n - 1, n - 1, 0], [n - 1, n - 2, n // 2], [0, 1, n - 1]]])
    v = (r.standard_normal((n, 3)) * np.ldexp(1.0, r.integers(-3, 4, (n, 1)))).astype(F)
    case(f"key_bits_{n}", v, f, all_with(iterations=2))

# ---- multiplicity: an edge shared by five faces, every face stored three times, both windings of one face ----
_mv = synth.uniform_cloud(7, seed=11) * F(3.0) - F(1.0)
_mf = [[0, 1, 2], [0, 1, 3], [1, 0, 4], [0, 1, 5], [1, 0, 6], [2, 1, 0]]
case("multiplicity", _mv, _mf * 3, all_with(iterations=3))

# ---- degenerate: repeated indices (self-neighbours), a mesh of one face, isolated vertices at 0, in the middle and at n - 1 ----
_dv = synth.uniform_cloud(9, seed=13) * F(2.0) + F(0.5)
case("degenerate_self", _dv, [[1, 1, 2], [3, 3, 3], [5, 6, 7], [6, 6, 5]], all_with(iterations=3))         # isolated: 0, 4, 8
case("degenerate_one_face", _dv[:3], [[0, 1, 2]], ALL_DEFAULT)
case("degenerate_all_same", _dv[:2], [[1, 1, 1]], all_with(iterations=2))

# ---- nonfinite: a NaN, a +inf and a -inf vertex; they spread by IEEE rules ----
_nv, _nf = synth.grid_mesh(16, 16, 0.5, seed=17)
_nv[37, 2], _nv[120, 0], _nv[200, 1] = np.nan, np.inf, -np.inf
case("nonfinite", _nv, _nf, all_with(iterations=3))

# ---- shifted: coordinates snapped to 2^-7 and moved far from the origin ----
SHIFTS = (0.0, 2.0 ** 10, 2.0 ** 16)
_sv, _sf = synth.grid_mesh(32, 32, 0.5, seed=19)
_sv = np.round(_sv * F(128.0)) / F(128.0)
for shift in SHIFTS:
    case(f"shifted_{int(shift)}", (_sv + F(shift)).astype(F), _sf, all_with(iterations=3))

# ---- params: the accepted ends of every range ----
_pv, _pf = synth.grid_mesh(9, 6, 0.7, seed=23)
BELOW_ONE = float(np.nextafter(F(1.0), F(0.0)))
case("params_lambda", _pv, _pf, [("laplacian", {"lambda_": 1.0, "iterations": 3}), ("taubin", {"lambda_": BELOW_ONE, "iterations": 3}),
                                 ("taubin", {"mu": -1e-30, "iterations": 3}), ("laplacian", {"lambda_": 0.3, "iterations": 3})])
# (1 - 0.3f is exact in f32; 1 - 0.1f is not: the last run is the one in which an f64 `1 - alpha` shows)
case("params_hc", _pv, _pf, [("hc", {"alpha": a, "beta": b, "iterations": 3}) for a in (0.0, 1.0, 0.3) for b in (0.0, 1.0, 0.3)] +
     [("hc", {"alpha": 0.1, "beta": 0.3, "iterations": 3})])

# every rejected value either side of each bound, NaN and the infinities; (method code or name, parameters, message)
ABOVE_ONE, BELOW_ZERO, ABOVE_ZERO = float(np.nextafter(F(1.0), F(2.0))), -float(np.nextafter(F(0.0), F(1.0))), float(np.nextafter(F(0.0), F(1.0)))
NOT_FINITE = (float("nan"), float("inf"), float("-inf"))
REJECTED = ([("laplacian", {"lambda_": x}, r"lambda must be in \(0, 1\]") for x in (0.0, -0.0, BELOW_ZERO, ABOVE_ONE, 1.5) + NOT_FINITE] +
            [("taubin", {"lambda_": x}, r"lambda must be in \(0, 1\)") for x in (0.0, BELOW_ZERO, 1.0, ABOVE_ONE) + NOT_FINITE] +
            [("taubin", {"mu": x}, "mu must be negative") for x in (0.0, -0.0, ABOVE_ZERO, 0.1) + NOT_FINITE] +
            [("hc", {"alpha": x}, r"alpha must be in \[0, 1\]") for x in (BELOW_ZERO, -0.1, ABOVE_ONE) + NOT_FINITE] +
            [("hc", {"beta": x}, r"beta must be in \[0, 1\]") for x in (BELOW_ZERO, ABOVE_ONE, 1.5) + NOT_FINITE] +
            [(3, {}, "method is none of")])
ACCEPTED_EDGES = [("laplacian", {"lambda_": ABOVE_ZERO}), ("taubin", {"lambda_": ABOVE_ZERO}), ("taubin", {"mu": BELOW_ZERO}),
                  ("hc", {"alpha": -0.0, "beta": -0.0})]

# ---- which named case tells each checker mutant apart (tests/test_mesh_cpu.py asserts it; the GPU file runs every case) ----
TELLS = {
    "descending_fold": ["rings_65_first"],
    "pairwise_sum": ["rings_129_middle"],
    "fused_step": ["params_lambda"],
    "reciprocal_division": ["block_edges_513"],
    "no_self_neighbour": ["degenerate_self"],
    "duplicates_in_degree": ["spike"],
    "f64_one_minus_alpha": ["params_hc"],
    "mu_first": ["box"],
    "avg_over_qbar": ["spike"],
    "isolated_to_origin": ["degenerate_self"],
}


def run_checker(c, rules=()):
    """every run of a case through the checker -> [(method, parameters, vertices)]"""
    return [(m, p, K.smooth(c["vertices"], c["faces"], METHODS[m], **p, rules=rules)) for m, p in c["runs"]]
