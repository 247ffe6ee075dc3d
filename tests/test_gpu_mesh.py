"""tc_mesh_smooth and tc_mesh_vertex_adjacency on the device against tests/mesh_checker.py: every case of tests/mesh_cases.py on both
roads (numpy in: the host entry point; torch device tensors in: the _device one).  Smoothed vertices are bit-EQUAL to the checker's (a NaN
compares as a NaN, zeros by their sign), offsets and neighbours exactly equal: no tolerance, nothing left out of a comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib
from tests import mesh_cases as MC
from tests import mesh_checker as K

pytestmark = pytest.mark.gpu
F = np.float32
SWEEP_ROWS = ("mesh_sweep_step", "mesh_sweep_hc_b", "mesh_sweep_hc_q")


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the checker's answer to every run of every case and its adjacency, computed once and shared"""
    return {name: (MC.run_checker(c), K.adjacency(len(c["vertices"]), c["faces"])) for name, c in MC.CASES.items()}


def _to(a, road):
    if road == "numpy":
        return a
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")


def _host(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same_bits(a, b):
    """bit for bit, every NaN equal to every NaN"""
    nan = np.isnan(a)
    return a.shape == b.shape and a.dtype == b.dtype == F and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def run(ctx, case, road, method, params):
    return _host(ctx.smooth_mesh(_to(case["vertices"], road), _to(case["faces"], road), method, **params))


@pytest.mark.parametrize("road", ["numpy", "torch"])
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_every_case_equals_the_checker(ctx, expected, name, road):
    case = MC.CASES[name]
    for method, params, want in expected[name][0]:
        got = run(ctx, case, road, method, params)
        diff = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1) & ~np.isnan(want).any(axis=1))[0]
        assert same_bits(got, want), (method, params, diff[:10], got[diff[:3]], want[diff[:3]])


@pytest.mark.parametrize("road", ["numpy", "torch"])
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_adjacency_equals_the_checker(ctx, expected, name, road):
    case = MC.CASES[name]
    off, nbr = ctx.mesh_adjacency(len(case["vertices"]), _to(case["faces"], road))
    assert isinstance(off, torch.Tensor) == (road == "torch")
    want_off, want_nbr = expected[name][1]
    off, nbr = _host(off), _host(nbr)
    assert off.dtype == nbr.dtype == np.uint32 and np.array_equal(off, want_off) and np.array_equal(nbr, want_nbr)


def test_two_calls_give_equal_bits_and_two_meshes_share_a_context(ctx, expected):
    names = ("rings_4097_middle", "key_bits_65537", "nonfinite", "rings_two_hubs")
    for road in ("numpy", "torch"):
        first = {name: [run(ctx, MC.CASES[name], road, m, p) for m, p, _ in expected[name][0]] for name in names}
        for name in reversed(names):                # interleaved: a mesh, another mesh, the first again
            for (m, p, want), before in zip(expected[name][0], first[name]):
                again = run(ctx, MC.CASES[name], road, m, p)
                assert same_bits(again, before) and same_bits(again, want)
                assert again.tobytes() == before.tobytes()          # the device's own NaNs, bit for bit


@pytest.mark.parametrize("name", ["block_edges_513", "rings_129_last", "iterations_0", "iterations_3"])
def test_the_output_may_be_the_input(ctx, expected, name):
    L = _lib.load_companion("threecrate_hip_mesh.h")
    case = MC.CASES[name]
    n, m = len(case["vertices"]), len(case["faces"])
    for method, params, want in expected[name][0]:
        cfg = _lib.MeshSmoothConfigC(MC.METHODS[method], *[{**K.DEFAULTS, **params}[k] for k in ("iterations", "lambda_", "mu", "alpha", "beta")])
        v = case["vertices"].copy()
        assert L.tc_mesh_smooth(ctx._h, v.ctypes.data, n, case["faces"].ctypes.data, m, C.byref(cfg), v.ctypes.data) == _lib.TC_OK
        assert same_bits(v, want)
        dv, df = _to(case["vertices"].copy(), "torch"), _to(case["faces"], "torch")
        torch.cuda.synchronize()
        assert L.tc_mesh_smooth_device(ctx._h, dv.data_ptr(), n, df.data_ptr(), m, C.byref(cfg), dv.data_ptr()) == _lib.TC_OK
        assert same_bits(_host(dv), want)


@pytest.mark.parametrize("name", ["spike", "key_bits_257", "rings_65_middle"])
def test_the_capacity_rule(ctx, expected, name):
    L = _lib.load_companion("threecrate_hip_mesh.h")
    case = MC.CASES[name]
    n, m = len(case["vertices"]), len(case["faces"])
    want_off, want_nbr = expected[name][1]
    total = len(want_nbr)
    message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
    for road, fn in (("numpy", L.tc_mesh_vertex_adjacency), ("torch", L.tc_mesh_vertex_adjacency_device)):
        faces = _to(case["faces"], road)
        fptr = faces.ctypes.data if road == "numpy" else faces.data_ptr()

        def call(with_off, with_nbr, capacity):
            off, nbr = _to(np.full(n + 1, 7, np.uint32), road), _to(np.full(total + 2, 7, np.uint32), road)
            ptr = lambda a: a.ctypes.data if road == "numpy" else a.data_ptr()
            count = C.c_size_t(7)
            torch.cuda.synchronize()
            rc = fn(ctx._h, n, fptr, m, ptr(off) if with_off else None, ptr(nbr) if with_nbr else None, capacity, C.byref(count))
            return rc, count.value, _host(off), _host(nbr)

        rc, count, off, nbr = call(False, False, 0)                         # the count alone
        assert (rc, count) == (_lib.TC_OK, total) and (off == 7).all() and (nbr == 7).all()
        for with_off, with_nbr in ((True, True), (True, False), (False, True)):
            rc, count, off, nbr = call(with_off, with_nbr, total - 1)      # too small: the count, nothing else
            assert (rc, count) == (_lib.TC_INVALID_DATA, total) and "capacity" in message() and (off == 7).all() and (nbr == 7).all()
            for capacity in (total, total + 1):
                rc, count, off, nbr = call(with_off, with_nbr, capacity)
                assert (rc, count) == (_lib.TC_OK, total)
                assert np.array_equal(off, want_off) if with_off else (off == 7).all()
                assert (np.array_equal(nbr[:total], want_nbr) if with_nbr else (nbr[:total] == 7).all()) and (nbr[total:] == 7).all()


def test_the_checks_come_in_the_headers_order(ctx):
    L = _lib.load_companion("threecrate_hip_mesh.h")
    v, out = MC.CASES["spike"]["vertices"].copy(), np.full((9, 3), 7, F)
    good = MC.CASES["spike"]["faces"].copy()
    I, U = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED
    message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()

    def config(method=0, iterations=1, lambda_=0.5, mu=-0.53, alpha=0.0, beta=0.5):
        return _lib.MeshSmoothConfigC(method, iterations, lambda_, mu, alpha, beta)

    for road, fn in (("numpy", L.tc_mesh_smooth), ("torch", L.tc_mesh_smooth_device)):
        dv, dout = _to(v, road), _to(out.copy(), road)
        ptr = lambda a: a.ctypes.data if road == "numpy" else a.data_ptr()
        torch.cuda.synchronize()

        def call(cfg, faces=good, n=9, m=None, v_ptr=True, f_ptr=True, o_ptr=True):
            df = _to(faces, road)
            torch.cuda.synchronize()
            return fn(ctx._h, ptr(dv) if v_ptr else None, n, ptr(df) if f_ptr else None, len(faces) if m is None else m,
                      None if cfg is None else C.byref(cfg), ptr(dout) if o_ptr else None)

        bad_index_first, bad_index_last = good.copy(), good.copy()
        bad_index_first[0, 1], bad_index_last[-1, 2] = 9, 0xFFFFFFFF
        # 1 before everything: an empty mesh, a bad method, bad sizes
        for kw in ({"v_ptr": False}, {"f_ptr": False}, {"o_ptr": False}):
            assert call(config(method=3), n=0, m=0, **kw) == I and "NULL" in message()
        assert call(None, n=0, m=0) == I and "config is NULL" in message()
        # 2 before 3, 4 and 5
        assert call(config(method=3, lambda_=float("nan")), n=0, m=2 ** 40) == I and message() == "Mesh is empty"
        assert call(config(method=3), n=2 ** 40, m=0) == I and message() == "Mesh is empty"
        # 3 before 4 and 5
        assert call(config(method=3, lambda_=float("nan")), n=2 ** 40) == I and "method" in message()
        # 4 before 5 and 6, with the reference's messages; only the method's own parameters are read
        assert call(config(0, lambda_=0.0), n=2 ** 40) == I and message() == "lambda must be in (0, 1]"
        assert call(config(1, lambda_=1.0, mu=1.0), faces=bad_index_first) == I and message() == "lambda must be in (0, 1)"
        assert call(config(1, mu=0.0), n=2 ** 40) == I and message() == "mu must be negative"
        assert call(config(2, alpha=2.0, beta=2.0), m=2 ** 40) == I and message() == "alpha must be in [0, 1]"
        assert call(config(2, beta=float("nan")), faces=bad_index_last) == I and message() == "beta must be in [0, 1]"
        assert (_host(dout) == 7).all()             # the failures of checks 1 to 4 wrote nothing
        assert call(config(0, mu=float("nan"), alpha=9.0, beta=-1.0)) == _lib.TC_OK
        assert call(config(2, lambda_=float("nan"), mu=5.0)) == _lib.TC_OK
        assert not (_host(dout) == 7).any()
        dout = _to(out.copy(), road)
        # 5 before 6: the exact bounds
        assert call(config(), n=2 ** 32 - 16, faces=bad_index_first) == U and "n_vertices" in message()
        assert call(config(), m=715827880, faces=bad_index_first) == U and "n_faces" in message()
        # 6: an index out of range at face 0 and at the last face, also with iterations == 0; nothing is written
        for faces in (bad_index_first, bad_index_last):
            for iterations in (0, 1):
                for method in (0, 1, 2):
                    assert call(config(method, iterations), faces=faces) == I and "a face index is >= n_vertices" in message()
        assert (_host(dout) == 7).all()
        total = C.c_size_t(7)
        afn = L.tc_mesh_vertex_adjacency if road == "numpy" else L.tc_mesh_vertex_adjacency_device
        df = _to(bad_index_last, road)
        torch.cuda.synchronize()
        assert afn(ctx._h, 9, ptr(df), 8, None, None, 0, C.byref(total)) == I and "a face index is >= n_vertices" in message() and total.value == 7
        assert afn(ctx._h, 0, ptr(df), 8, None, None, 0, C.byref(total)) == I and message() == "Mesh is empty"
        assert afn(ctx._h, 9, ptr(df), 8, None, None, 0, None) == I and afn(ctx._h, 9, None, 8, None, None, 0, C.byref(total)) == I
        assert afn(ctx._h, 2 ** 32 - 16, ptr(df), 8, None, None, 0, C.byref(total)) == U
    # the same answers through the context's methods
    with pytest.raises(tc.InvalidData, match="Mesh is empty"):
        ctx.smooth_mesh(*MC.EMPTY_STRIP)
    with pytest.raises(tc.InvalidData, match="a face index is >= n_vertices"):
        ctx.smooth_mesh(v, bad_index_first, iterations=0)
    with pytest.raises(tc.InvalidData, match="method"):
        ctx.smooth_mesh(v, good, "cotangent")


@pytest.mark.parametrize("method, params, message", MC.REJECTED, ids=[f"{m}-{p}" for m, p, _ in MC.REJECTED])
def test_every_rejected_parameter(ctx, method, params, message):
    case = MC.CASES["spike"]
    for road in ("numpy", "torch"):
        with pytest.raises(tc.InvalidData, match=message):
            run(ctx, case, road, method, params)


def test_the_accepted_ends_of_the_ranges(ctx):
    case = MC.CASES["spike"]
    for method, params in MC.ACCEPTED_EDGES:
        want = K.smooth(case["vertices"], case["faces"], MC.METHODS[method], **{"iterations": 2, **params})
        for road in ("numpy", "torch"):
            assert same_bits(run(ctx, case, road, method, {"iterations": 2, **params}), want), (method, params)


def test_launch_rows(ctx, expected):
    """per call: one adjacency build; as many sweeps as the method launches; the long-ring row exactly where a ring exceeds the constant"""
    launches = {"laplacian": 1, "taubin": 2, "hc": 2}

    def rows():
        r = {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("mesh_")}
        return r.get("mesh_adjacency", 0), sum(r.get(k, 0) for k in SWEEP_ROWS), r.get("mesh_sweep_long", 0), set(r) - {"mesh_adjacency", "mesh_sweep_long"} - set(SWEEP_ROWS)

    ctx.profile_enable(True)
    try:
        for name in ("block_edges_513", f"rings_{MC.LONG_RING}_first", f"rings_{MC.LONG_RING + 1}_first", "rings_two_hubs", "iterations_0"):
            case = MC.CASES[name]
            deg = np.diff(expected[name][1][0].astype(np.int64))
            for road in ("numpy", "torch"):
                for method, params in case["runs"]:
                    ctx.profile_reset()
                    run(ctx, case, road, method, params)
                    sweeps = launches[method] * params.get("iterations", 10)
                    assert rows() == (1, sweeps, sweeps if deg.max() > MC.LONG_RING else 0, set()), (name, road, method)
        ctx.profile_reset()
        ctx.mesh_adjacency(9, MC.CASES["spike"]["faces"])
        assert rows() == (2, 0, 0, set())           # count, then fill
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


def test_a_call_after_the_other_users_of_the_pinned_block_equals_a_fresh_context(ctx, expected):
    """voxel filter (the count word), plane segmentation (the union), a voxel map and a counted colorization (the regions in front)"""
    pts = np.random.default_rng(3).random((3000, 3), dtype=F)
    ctx.voxel_grid_filter(pts, 0.1)
    ctx.segment_plane(pts, 0.05, 64, seed=1)
    m = ctx.voxel_map(0.1)
    m.insert(pts)
    assert len(m) > 0
    m.close()
    ctx.colorize(pts, [(np.full((4, 4, 3), 200, np.uint8), (2.0, 2.0, 1.5, 1.5), np.eye(4, dtype=F))])
    name = "rings_two_hubs"
    fresh = tc.GpuContext(0)
    try:
        for road in ("numpy", "torch"):
            for method, params, want in expected[name][0]:
                a, b = run(ctx, MC.CASES[name], road, method, params), run(fresh, MC.CASES[name], road, method, params)
                assert a.tobytes() == b.tobytes() and same_bits(a, want)
    finally:
        fresh.close()
    assert ctx.voxel_grid_filter(pts, 0.1).shape[1] == 3        # and the others still work after it


def test_compat_smoothers_equal_the_context_call(ctx, expected):
    case = MC.CASES["spike"]
    mesh = threecrate.TriangleMesh.from_numpy(case["vertices"], case["faces"].astype(np.int64))
    for fn, (method, params, want) in zip((threecrate.smooth_mesh_laplacian, threecrate.smooth_mesh_taubin, threecrate.smooth_mesh_hc), expected["spike"][0]):
        got = fn(mesh)
        assert isinstance(got, threecrate.TriangleMesh) and got is not mesh and np.array_equal(got.faces(), case["faces"])
        assert same_bits(got.vertices(), want) and same_bits(got.vertices(), run(ctx, case, "numpy", method, params))
        assert got.vertices()[4, 2] < 1.0 and np.array_equal(mesh.vertices(), case["vertices"])
        assert same_bits(fn(mesh, 0).vertices(), case["vertices"])
    assert same_bits(threecrate.smooth_mesh_taubin(mesh, 3, 0.4, -0.45).vertices(), K.smooth(case["vertices"], case["faces"], K.TAUBIN, 3, 0.4, -0.45))
    assert same_bits(threecrate.smooth_mesh_hc(mesh, 2, 0.1, 0.3).vertices(), K.smooth(case["vertices"], case["faces"], K.HC, 2, alpha=0.1, beta=0.3))
    for fn, kw, message in ((threecrate.smooth_mesh_laplacian, {"lambda_": 1.5}, r"lambda must be in \(0, 1\]"), (threecrate.smooth_mesh_taubin, {"mu": 0.1}, "mu must be negative"),
                            (threecrate.smooth_mesh_hc, {"alpha": -0.1}, r"alpha must be in \[0, 1\]"), (threecrate.smooth_mesh_hc, {"beta": 1.5}, r"beta must be in \[0, 1\]")):
        with pytest.raises(RuntimeError, match=message):
            fn(mesh, 1, **kw)
    bad = threecrate.TriangleMesh.from_numpy(case["vertices"], np.array([[0, 1, 9]], np.int32))
    with pytest.raises(RuntimeError, match="a face index is >= n_vertices"):
        threecrate.smooth_mesh_laplacian(bad)
