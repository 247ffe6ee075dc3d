"""Mesh smoothing without a GPU: the reference's unit tests as literals through the checker (tests/mesh_checker.py), the checker's
adjacency against a plain-Python set build, what separates the fixed summation order from the reference's unspecified one, the calls that
need no device, the compat surface, the Rust facade's names, and the mutant table -- every rule of the contract a mutant breaks is told
apart by a named case of tests/mesh_cases.py that tests/test_gpu_mesh.py also runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import abi_text as T
from tests import mesh_cases as MC
from tests import mesh_checker as K
from threecrate_amd import _lib, compat as threecrate, synth

F = np.float32


def smooth(name, method, **p):
    c = MC.CASES[name]
    return K.smooth(c["vertices"], c["faces"], MC.METHODS[method], **p)


# ---- the reference's unit tests (mesh_smoothing.rs:330-633) ----
@pytest.mark.parametrize("method", list(MC.METHODS))
def test_reference_spike_is_reduced_and_the_vertex_count_kept(method):
    out = smooth("spike", method)
    assert out.shape == (9, 3) and out.dtype == F
    assert out[4, 2] < 1.0


def test_reference_taubin_shrinks_less_than_laplacian():
    def spread(v):
        c = v.mean(axis=0)
        return np.linalg.norm(v - c, axis=1).mean()
    lap, tau = smooth("box", "laplacian", iterations=50, lambda_=0.5), smooth("box", "taubin", iterations=50, lambda_=0.5, mu=-0.53)
    assert spread(tau) > spread(lap)


@pytest.mark.parametrize("method", list(MC.METHODS))
def test_reference_zero_iterations_return_the_input(method):
    assert smooth("spike", method, iterations=0).tobytes() == MC.CASES["spike"]["vertices"].tobytes()


def test_reference_more_iterations_smooth_more():
    assert smooth("spike", "laplacian", iterations=5)[4, 2] < smooth("spike", "laplacian", iterations=1)[4, 2]


def test_reference_spike_literals():
    """one Laplacian step at lambda 0.5 by hand: the centre's ring is the six vertices its faces name, a corner's two, an edge's four"""
    off, nbr = K.adjacency(9, MC.SPIKE_F)
    assert nbr[off[4]:off[5]].tolist() == [1, 2, 3, 5, 6, 7] and nbr[off[0]:off[1]].tolist() == [1, 3]
    out = smooth("spike", "laplacian", iterations=1)
    assert out[4].tolist() == [1.0, 1.0, 0.5] and out[0].tolist() == [0.25, 0.25, 0.0]
    assert nbr[off[1]:off[2]].tolist() == [0, 2, 3, 4] and out[1].tolist() == [0.875, 0.25, 0.125]


# ---- the checker's adjacency ----
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_adjacency_is_the_plain_set_build(name):
    c = MC.CASES[name]
    n = len(c["vertices"])
    adj = [set() for _ in range(n)]
    for a, b, cc in c["faces"].tolist():
        adj[a] |= {b, cc}
        adj[b] |= {a, cc}
        adj[cc] |= {a, b}
    off, nbr = K.adjacency(n, c["faces"])
    assert off.dtype == nbr.dtype == np.uint32 and off[0] == 0 and off[-1] == len(nbr) == sum(len(s) for s in adj)
    flat = [j for s in adj for j in sorted(s)]
    assert nbr.tolist() == flat and np.diff(off.astype(np.int64)).tolist() == [len(s) for s in adj]


def test_what_the_case_groups_are_for():
    deg = lambda name: np.diff(K.adjacency(len(MC.CASES[name]["vertices"]), MC.CASES[name]["faces"])[0].astype(np.int64))
    assert [len(MC.CASES[f"block_edges_{n}"]["vertices"]) for n in MC.BLOCK_EDGES] == [4, 255, 256, 257, 513]
    assert len(MC.EMPTY_STRIP[0]) == 2 and len(MC.EMPTY_STRIP[1]) == 0
    assert MC.LONG_RING == 128 and {MC.LONG_RING - 1, MC.LONG_RING, MC.LONG_RING + 1, 1, 2, 127, 128, 129, 192, 193, 256, 257, 4097} <= set(MC.RING_SIZES)
    for ring in MC.RING_SIZES:
        for where, at in MC.HUB_AT.items():
            d = deg(f"rings_{ring}_{where}")
            assert d[at(ring + 1)] == ring and d.argmax() == at(ring + 1) or ring <= 3
    d = deg("rings_two_hubs")
    off, nbr = K.adjacency(len(d), MC.CASES["rings_two_hubs"]["faces"])
    assert d[0] > MC.LONG_RING and d[1] > MC.LONG_RING and 1 in nbr[off[0]:off[1]] and 0 in nbr[off[1]:off[2]]
    _, _, hubs, rings = MC.five_hubs()
    d = deg("rings_five_hubs")
    assert np.array_equal(d[hubs], rings) and sorted(rings[rings > MC.LONG_RING].tolist()) == [129, 192, 193, 256, 257] and (rings <= MC.LONG_RING).sum() == 40
    assert np.array_equal(np.flatnonzero(d > MC.LONG_RING), hubs[rings > MC.LONG_RING]) and (np.diff(np.flatnonzero(rings > MC.LONG_RING)) == 9).all()
    for n in MC.KEY_BITS:
        f = MC.CASES[f"key_bits_{n}"]["faces"]
        d = deg(f"key_bits_{n}")
        assert len(f) < 48 and f.max() == n - 1 and f.min() == 0 and (d == 0).sum() > n - 150 and d[0] and d[n // 2] and d[n - 1]
        assert (n - 1) in f[:, 0] and (n - 1) in f[:, 1:]                   # the largest index in both halves of a key
    d = deg("degenerate_self")
    off, nbr = K.adjacency(9, MC.CASES["degenerate_self"]["faces"])
    assert d[[0, 4, 8]].tolist() == [0, 0, 0] and nbr[off[1]:off[2]].tolist() == [1, 2] and nbr[off[3]:off[4]].tolist() == [3]
    d = deg("multiplicity")
    assert d[0] == 6 and d[1] == 6 and len(MC.CASES["multiplicity"]["faces"]) == 18
    v = MC.CASES["nonfinite"]["vertices"]
    assert np.isnan(v).sum() == 1 and np.isposinf(v).sum() == 1 and np.isneginf(v).sum() == 1
    for shift in MC.SHIFTS:
        v = MC.CASES[f"shifted_{int(shift)}"]["vertices"]
        assert (v * 128 == np.round(v * 128)).all() and v.min() >= shift - 1
    assert max(len(c["vertices"]) for c in MC.CASES.values()) == 65537


def test_a_long_ring_does_not_cost_a_pass_per_neighbour():
    """the 4 097-ring hub: the checker groups by degree, so the whole case is a handful of numpy calls"""
    import time
    t0 = time.perf_counter()
    MC.run_checker(MC.CASES["rings_4097_middle"])
    assert time.perf_counter() - t0 < 2.0


def test_accumulate_is_the_sequential_fold_and_reduce_is_not():
    x = MC.CASES["rings_129_middle"]["vertices"][:, 0]
    seq = F(0.0)
    for v in x:
        seq = F(seq + v)
    assert np.add.accumulate(np.concatenate([[F(0.0)], x]), dtype=F)[-1] == seq
    assert np.add.reduce(x, dtype=F) != seq


# ---- the summation order: what separates this contract from the reference's unspecified order ----
@pytest.mark.parametrize("name", ["rings_65_first", "rings_4097_middle", "block_edges_513", "rings_two_hubs"])
def test_any_order_stays_within_the_derived_bound_of_the_ascending_one(name):
    """the header's figure, as it stands: two sequential f32 folds of the same d terms each carry at most d - 1 roundings (the first add,
    to +0, is exact) of at most 2^-24 times a partial sum of at most sum|x_j|, so they differ by at most 2 (d - 1) 2^-24 sum|x_j|"""
    c = MC.CASES[name]
    v = c["vertices"]
    off, nbr = K.adjacency(len(v), c["faces"])
    want = K.ring_sums(v, off, nbr)
    r = np.random.default_rng(1)
    shuffled = nbr.copy()
    for i in range(len(v)):
        r.shuffle(shuffled[off[i]:off[i + 1]])
    got = K.ring_sums(v, off, shuffled)
    d = np.diff(off.astype(np.int64))
    absum = np.stack([np.bincount(np.repeat(np.arange(len(v)), d), np.abs(v[nbr, k]).astype(np.float64), len(v)) for k in range(3)], axis=1)
    bound = 2.0 * np.maximum(d - 1, 0)[:, None] * 2.0 ** -24 * absum
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= bound).all()
    if name.startswith("rings"):
        assert got.tobytes() != want.tobytes()      # and the order does show in the bits


# ---- the calls that need no device ----
def test_a_null_context_is_invalid_data_whatever_else_is_wrong_and_writes_nothing():
    L = _lib.load_companion("threecrate_hip_mesh.h")
    for method in (0, 1, 2, 7):
        cfg = _lib.MeshSmoothConfigC(9, 9, 9, 9, 9, 9)
        L.tc_mesh_smooth_config_default(method, C.byref(cfg))
        assert (cfg.method, cfg.iterations, getattr(cfg, "lambda"), cfg.mu, cfg.alpha, cfg.beta) == (method, 10, 0.5, F(-0.53), 0.0, 0.5)
    L.tc_mesh_smooth_config_default(0, None)
    v, f, out = np.zeros((3, 3), F), np.array([[0, 1, 2]], np.uint32), np.full((3, 3), 7, F)
    bad = _lib.MeshSmoothConfigC(3, 1, float("nan"), 1.0, 2.0, 2.0)
    for fn in (L.tc_mesh_smooth, L.tc_mesh_smooth_device):
        for args in ((v.ctypes.data, 3, f.ctypes.data, 1, C.byref(cfg)), (None, 3, None, 1, None), (v.ctypes.data, 0, f.ctypes.data, 0, C.byref(cfg)),
                     (v.ctypes.data, 3, f.ctypes.data, 1, C.byref(bad)), (v.ctypes.data, 2 ** 32, f.ctypes.data, 2 ** 32, C.byref(cfg))):
            assert fn(None, *args, out.ctypes.data) == _lib.TC_INVALID_DATA
    off, nbr, total = np.full(4, 7, np.uint32), np.full(6, 7, np.uint32), C.c_size_t(7)
    for fn in (L.tc_mesh_vertex_adjacency, L.tc_mesh_vertex_adjacency_device):
        for args in ((3, f.ctypes.data, 1), (0, None, 0), (2 ** 32, f.ctypes.data, 2 ** 32)):
            assert fn(None, *args, off.ctypes.data, nbr.ctypes.data, 6, C.byref(total)) == _lib.TC_INVALID_DATA
    assert (out == 7).all() and (off == 7).all() and (nbr == 7).all() and total.value == 7


def test_the_header_states_the_checks_in_the_order_the_entry_points_make_them():
    """the order itself needs a context (tests/test_gpu_mesh.py runs it); here: the text of mesh_check() follows the header's list"""
    src = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "mesh.hip")).read()
    body = src[src.index("static tc_status mesh_check("):src.index("static tc_status mesh_check_adjacency(")]
    marks = ["if (!ctx)", "!vertices)", "!faces)", "!cfg)", "!out_vertices)", "mesh_check_empty(", "method > TC_MESH_HC", "lambda must be in (0, 1]",
             "lambda must be in (0, 1)", "mu must be negative", "alpha must be in [0, 1]", "beta must be in [0, 1]", "mesh_check_limits("]
    at = [body.index(m) for m in marks]
    assert at == sorted(at)
    body = src[src.index("static tc_status mesh_check_adjacency("):src.index('extern "C" {')]
    at = [body.index(m) for m in ("if (!ctx)", "!faces)", "!n_entries)", "mesh_check_empty(", "mesh_check_limits(")]
    assert at == sorted(at)
    # the index check is the build's, and the build comes before the iterations == 0 shortcut
    body = src[src.index("static tc_status mesh_smooth_on_device("):src.index("static tc_status mesh_adjacency(")]
    assert body.index("mesh_build(") < body.index("cfg.iterations == 0")
    assert '"Mesh is empty"' in src and "a face index is >= n_vertices" in src
    header = open(os.path.join(T.ROOT, "include", "threecrate_hip_mesh.h")).read()
    assert "Deviations from mesh_smoothing.rs" in header and "ASCENDING" in header and "2^32 - 16" in header
    assert "#pragma clang fp contract(off)" in src
    mk = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "Makefile")).read()
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1) and "$(HIPCC) $(CXXFLAGS) -c mesh.hip" in mk


def test_the_unit_has_one_sort_call_site_and_no_atomics_in_a_sweep():
    src = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "mesh.hip")).read()
    assert "rocprim" not in src and src.count("group_by_key(ctx") == 1 and "sort_pairs(ctx" not in src and "key_runs(ctx" not in src
    for kernel in ("mesh_sweep_kernel", "mesh_sweep_long_kernel"):
        body = src[src.index(f"{kernel}(MeshSweep a"):]
        body = body[:body.index("\n}\n")]
        assert "atomic" not in body, kernel
    assert re.search(r"constexpr uint32_t kMeshLongRing = \d+;", src)
    internal = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "tc_internal.h")).read()
    assert "offsetof(PinnedBlock, mesh_out) == 2048 + 8192 + 736" in internal
    assert internal.index("ColorOut color_out;") < internal.index("MeshOut  mesh_out;")


# ---- synth.grid_mesh ----
def test_grid_mesh_is_a_row_major_height_field():
    v, f = synth.grid_mesh(4, 3, 0.5, seed=2)
    assert v.shape == (12, 3) and v.dtype == F and f.shape == (12, 3) and f.dtype == np.uint32
    assert v[:, 0].tolist() == [0, 1, 2, 3] * 3 and v[:, 1].tolist() == [0] * 4 + [1] * 4 + [2] * 4 and (np.abs(v[:, 2]) <= 0.25).all()
    assert f[:2].tolist() == [[0, 1, 4], [1, 5, 4]] and f[-1].tolist() == [7, 11, 10]
    assert (synth.grid_mesh(4, 3, 0.0)[0][:, 2] == 0).all() and np.array_equal(synth.grid_mesh(4, 3, 0.5, seed=2)[0], v)
    assert len(synth.grid_mesh(1000, 1000)[1]) == 2 * 999 * 999
    for nx, ny in ((1, 2), (2, 1), (1, 1)):
        assert synth.grid_mesh(nx, ny)[0].shape == (nx * ny, 3) and synth.grid_mesh(nx, ny)[1].shape == (0, 3)


# ---- compat ----
def test_triangle_mesh_has_the_wheels_surface_and_messages():
    v, f = synth.grid_mesh(3, 3, 0.5)
    mesh = threecrate.TriangleMesh.from_numpy(v.astype(np.float64), f.astype(np.int64))
    assert (mesh.vertex_count, mesh.face_count, mesh.is_empty) == (9, 8, False) and repr(mesh) == "TriangleMesh(9 vertices, 8 faces)"
    assert mesh.vertices().dtype == F and np.array_equal(mesh.vertices(), v) and mesh.faces().dtype == np.uint32 and np.array_equal(mesh.faces(), f)
    empty = threecrate.TriangleMesh()
    assert (empty.vertex_count, empty.face_count, empty.is_empty) == (0, 0, True) and repr(empty) == "TriangleMesh(0 vertices, 0 faces)"
    assert empty.vertices().shape == (0, 3) and empty.faces().shape == (0, 3)
    for dtype in (np.uint32, np.int32, np.uint64, np.int64):
        assert np.array_equal(threecrate.TriangleMesh.from_numpy(v, f.astype(dtype)).faces(), f)
    for bad in (f.astype(np.int16), f.astype(np.float32), f.tolist(), f.reshape(-1)):
        with pytest.raises(ValueError, match=r"Faces array must be \(M, 3\) integer numpy array \(int32, int64, uint32, or uint64\)"):
            threecrate.TriangleMesh.from_numpy(v, bad)
    with pytest.raises(ValueError, match=r"Faces array must have shape \(M, 3\), got \[12, 2\]"):
        threecrate.TriangleMesh.from_numpy(v, f.reshape(12, 2))
    with pytest.raises(ValueError, match="float32 or float64"):
        threecrate.TriangleMesh.from_numpy(v.astype(np.int32), f)
    with pytest.raises(ValueError, match=r"must have shape \(N, 3\)"):
        threecrate.TriangleMesh.from_numpy(v[:, :2], f)
    # `as usize` of a negative or too large index is out of range in the wheel, and stays out of range here
    assert threecrate.TriangleMesh.from_numpy(v, np.array([[0, -1, 2]], np.int32)).faces().tolist() == [[0, 0xFFFFFFFF, 2]]
    assert threecrate.TriangleMesh.from_numpy(v, np.array([[0, 2 ** 32, 2]], np.uint64)).faces().tolist() == [[0, 0xFFFFFFFF, 2]]
    v[0, 0] = 5
    assert mesh.vertices()[0, 0] == 0


def test_the_smoothers_have_the_wheels_signatures_and_the_empty_error():
    sig = lambda fn: [(k, p.default) for k, p in inspect.signature(fn).parameters.items()][1:]
    assert sig(threecrate.smooth_mesh_laplacian) == [("iterations", 10), ("lambda_", 0.5)]
    assert sig(threecrate.smooth_mesh_taubin) == [("iterations", 10), ("lambda_", 0.5), ("mu", -0.53)]
    assert sig(threecrate.smooth_mesh_hc) == [("iterations", 10), ("alpha", 0.0), ("beta", 0.5)]
    assert {"TriangleMesh", "smooth_mesh_laplacian", "smooth_mesh_taubin", "smooth_mesh_hc"} <= set(threecrate.__all__)
    no_faces = threecrate.TriangleMesh.from_numpy(np.zeros((3, 3), F), np.zeros((0, 3), np.uint32))
    for fn in (threecrate.smooth_mesh_laplacian, threecrate.smooth_mesh_taubin, threecrate.smooth_mesh_hc):
        for mesh in (threecrate.TriangleMesh(), no_faces):
            with pytest.raises(RuntimeError, match="Mesh is empty"):
                fn(mesh)
    from threecrate_amd import api
    assert sig(api.GpuContext.smooth_mesh) == [("vertices", inspect.Parameter.empty), ("faces", inspect.Parameter.empty), ("method", "laplacian"),
                                               ("iterations", 10), ("lambda_", 0.5), ("mu", -0.53), ("alpha", 0.0), ("beta", 0.5)]
    assert [k for k, _ in sig(api.GpuContext.mesh_adjacency)] == ["n_vertices", "faces"]
    assert K.DEFAULTS == {k: d for k, d in sig(api.GpuContext.smooth_mesh)[3:]}


# ---- the Rust facade ----
def test_the_rust_facade_has_the_references_names():
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    mod = lib_rs[lib_rs.index("pub mod mesh_smoothing {"):]
    for decl in ("pub struct LaplacianSmoothingConfig", "pub struct TaubinSmoothingConfig", "pub struct HcSmoothingConfig",
                 "impl Default for LaplacianSmoothingConfig", "impl Default for TaubinSmoothingConfig", "impl Default for HcSmoothingConfig",
                 "pub fn smooth_laplacian(", "pub fn smooth_taubin(", "pub fn smooth_hc("):
        assert decl in mod, decl
    assert "Self { iterations: 10, lambda: 0.5 }" in mod and "Self { iterations: 10, lambda: 0.5, mu: -0.53 }" in mod
    assert "Self { iterations: 10, alpha: 0.0, beta: 0.5 }" in mod
    assert re.search(r"^pub mod ffi_mesh;", lib_rs, re.M)


# ---- the mutants ----
INVISIBLE = {}      # rule -> why no case can show it.  Empty: every mutant below is told apart


def _bits(results):
    return b"".join(v.tobytes() for _, _, v in results)


@pytest.mark.parametrize("rule", sorted(K.RULES))
def test_every_mutant_is_told_apart_by_a_named_case(rule):
    assert (rule in MC.TELLS) != (rule in INVISIBLE)
    for name in MC.TELLS.get(rule, ()):
        c = MC.CASES[name]
        assert _bits(MC.run_checker(c)) != _bits(MC.run_checker(c, rules={rule})), (rule, name)


def test_the_mutant_table_is_the_issues(capsys):
    assert sorted(K.RULES) == sorted(MC.TELLS) and len(K.RULES) == 10 and not INVISIBLE
    assert all(name in MC.CASES for names in MC.TELLS.values() for name in names)
    with capsys.disabled():
        print("\nmutant | cases of the table that tell it apart (of %d)" % len(MC.CASES))
        for rule in sorted(K.RULES):
            seen = [name for name, c in MC.CASES.items() if len(c["vertices"]) <= 5000 and _bits(MC.run_checker(c)) != _bits(MC.run_checker(c, rules={rule}))]
            print(f"{rule} | {len(seen)}: {', '.join(seen[:4])}{' ...' if len(seen) > 4 else ''}")
