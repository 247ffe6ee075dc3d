"""tc_simplify_clustering on the device against tests/simplify_checker.py: every case of tests/simplify_cases.py on both roads (numpy in:
the host entry point; torch device tensors in: the _device one).  Vertices, faces, normals, colours, the vertex map and the two counts are
bit-EQUAL to the checker's: no tolerance, nothing left out of a comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib
from tests import simplify_cases as SC
from tests import simplify_checker as K

pytestmark = pytest.mark.gpu
F = np.float32
HEADER = "threecrate_hip_simplify.h"
ROWS = ("simplify_classes", "simplify_clusters", "simplify_faces", "simplify_write")
STRATEGY = {0: "centroid", 1: "weighted_average"}
ROADS = ["numpy", "torch"]


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def checker(case, params):
    return K.simplify(case["vertices"], case["faces"], normals=case["normals"], colors=case["colors"], **params)


@pytest.fixture(scope="module")
def expected():
    """the checker's answer to every run of every case, computed once and shared"""
    return {name: [checker(c, p) for p in c["runs"]] for name, c in SC.CASES.items()}


def _to(a, road):
    if a is None or road == "numpy":
        return a
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")


def _host(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def same_bits(a, b):
    """bit for bit, shape and type included (a NaN equals the same NaN, zeros by their sign)"""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run(ctx, case, road, params):
    """-> dict(vertices, faces, normals, colors, map), host arrays"""
    out = ctx.simplify_mesh_clustering(_to(case["vertices"], road), _to(case["faces"], road), params["ratio"], STRATEGY[params["strategy"]],
                                       bool(params["preserve_boundary"]), params["threshold"], normals=_to(case["normals"], road),
                                       colors=_to(case["colors"], road), return_map=True)
    assert all(isinstance(a, torch.Tensor) == (road == "torch") for a in out)
    out = [_host(a) for a in out]
    got = {"vertices": out[0], "faces": out[1], "normals": None, "colors": None, "map": out[-1]}
    rest = out[2:-1]
    if case["normals"] is not None:
        got["normals"] = rest.pop(0)
    if case["colors"] is not None:
        got["colors"] = rest.pop(0)
    assert not rest
    return got


def assert_equal(got, want, what):
    for key in ("vertices", "faces", "normals", "colors", "map"):
        if want[key] is None:
            assert got[key] is None, (what, key)
            continue
        g, w = got[key], want[key]
        rows = np.nonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))[0] if g.shape == w.shape and g.size else None
        assert same_bits(g, w), (what, key, g.shape, w.shape, None if rows is None else (rows[:5], g[rows[:3]], w[rows[:3]]))


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_every_case_equals_the_checker(ctx, expected, name, road):
    case = SC.CASES[name]
    for params, want in zip(case["runs"], expected[name]):
        assert_equal(run(ctx, case, road, params), want, params)


def test_wide_keys_take_the_two_pass_face_sort_on_both_roads(ctx):
    v, f, params = SC.wide_keys()
    assert len(v) > 2 ** 21
    want = K.simplify(v, f, **params)
    assert len(want["sizes"]) > 2 ** 21 and want["cluster_of"][f].min() > 2 ** 21 and want["repeated"] > 0 and want["degenerate"] > 0
    case = {"vertices": v, "faces": f, "normals": None, "colors": None}
    for road in ROADS:
        assert_equal(run(ctx, case, road, params), want, road)


@pytest.mark.parametrize("road", ROADS)
def test_two_calls_are_bit_equal(ctx, road):
    for name in ("classes_open_box", f"cluster_sizes_{SC.LONG_CLUSTER + 1}", "blocks_513"):
        case = SC.CASES[name]
        for params in case["runs"][:4]:
            assert_equal(run(ctx, case, road, params), run(ctx, case, road, params), (name, params))


def _raw(ctx, road):
    L = _lib.load_companion(HEADER)
    fn = L.tc_simplify_clustering if road == "numpy" else L.tc_simplify_clustering_device
    ptr = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
    return fn, ptr


def _message(ctx):
    return _lib.load().tc_last_error_message(ctx._h).decode()


def _config(params):
    return _lib.SimplifyConfigC(params["strategy"], params["preserve_boundary"], params["threshold"], params["ratio"])


@pytest.mark.parametrize("road", ROADS)
def test_count_only_capacities_and_the_copy_of_ratio_zero(ctx, expected, road):
    """the count-only call agrees with the filled one; a capacity one below a count fails and writes nothing but the counts; ratio 0 copies"""
    fn, ptr = _raw(ctx, road)
    I = _lib.TC_INVALID_DATA
    name = "blocks_513"
    case, params, want = SC.CASES[name], SC.CASES[name]["runs"][2], expected[name][2]
    n, m = len(case["vertices"]), len(case["faces"])
    nv_want, nf_want = len(want["vertices"]), len(want["faces"])
    assert 0 < nv_want < n and 0 < nf_want < m
    dv, df, dn, dc = (_to(case[k], road) for k in ("vertices", "faces", "normals", "colors"))

    def call(cfg, cap_v, cap_f, outputs=True, with_map=True):
        out = {"v": np.full((n, 3), 7, F), "n": np.full((n, 3), 7, F), "c": np.full((n, 3), 7, np.uint8), "f": np.full((m, 3), 7, np.uint32),
               "m": np.full(n, 7, np.uint32)}
        dev = {k: _to(a, road) for k, a in out.items()}
        nv, nf = C.c_size_t(7), C.c_size_t(7)
        torch.cuda.synchronize()
        rc = fn(ctx._h, ptr(dv), n, ptr(df), m, ptr(dn), ptr(dc), C.byref(cfg), ptr(dev["v"]) if outputs else None, ptr(dev["n"]), ptr(dev["c"]), cap_v,
                ptr(dev["f"]) if outputs else None, cap_f, ptr(dev["m"]) if outputs and with_map else None, C.byref(nv), C.byref(nf))
        return rc, nv.value, nf.value, {k: _host(a) for k, a in dev.items()}

    cfg = _config(params)
    # exact capacities
    rc, nv, nf, out = call(cfg, nv_want, nf_want)
    assert (rc, nv, nf) == (_lib.TC_OK, nv_want, nf_want)
    assert same_bits(out["v"][:nv], want["vertices"]) and same_bits(out["f"][:nf], want["faces"]) and same_bits(out["n"][:nv], want["normals"])
    assert same_bits(out["c"][:nv], want["colors"]) and same_bits(out["m"], want["map"])
    assert (out["v"][nv:] == 7).all() and (out["f"][nf:] == 7).all() and (out["n"][nv:] == 7).all() and (out["c"][nv:] == 7).all()
    # one below either count: the counts and nothing else
    for cap_v, cap_f, word in ((nv_want - 1, nf_want, "cap_vertices"), (nv_want, nf_want - 1, "cap_faces"), (0, 0, "cap_vertices")):
        rc, nv, nf, out = call(cfg, cap_v, cap_f)
        assert (rc, nv, nf) == (I, nv_want, nf_want) and word in _message(ctx)
        assert all((a == 7).all() for a in out.values())
    # the vertex map alone is an output like the others
    rc, nv, nf, out = call(cfg, 0, 0, outputs=False)
    assert (rc, nv, nf) == (I, nv_want, nf_want)
    # ratio 0: the mesh as given, capacities against n and m
    zero = _config({**params, "ratio": 0.0})
    rc, nv, nf, out = call(zero, n, m)
    assert (rc, nv, nf) == (_lib.TC_OK, n, m)
    assert same_bits(out["v"], case["vertices"]) and same_bits(out["f"], case["faces"]) and same_bits(out["n"], case["normals"])
    assert same_bits(out["c"], case["colors"]) and np.array_equal(out["m"], np.arange(n, dtype=np.uint32))
    rc, nv, nf, out = call(zero, n - 1, m)
    assert (rc, nv, nf) == (I, n, m) and all((a == 7).all() for a in out.values())
    # the count-only call: no output array at all (the attribute outputs go with their inputs, so the inputs go too)
    nv, nf = C.c_size_t(7), C.c_size_t(7)
    for c, counts in ((cfg, (nv_want, nf_want)), (zero, (n, m))):
        assert fn(ctx._h, ptr(dv), n, ptr(df), m, None, None, C.byref(c), None, None, None, 0, None, 0, None, C.byref(nv), C.byref(nf)) == _lib.TC_OK
        assert (nv.value, nf.value) == counts


def test_ratio_zero_through_the_context(ctx):
    case = SC.CASES["blocks_257"]                     # the unreferenced vertex stays
    for road in ROADS:
        got = run(ctx, case, road, SC.run(0.0))
        assert_equal(got, checker(case, SC.run(0.0)), road)
        assert len(got["vertices"]) == 257


@pytest.mark.parametrize("road", ROADS)
def test_the_order_of_checks_with_a_live_context(ctx, road):
    fn, ptr = _raw(ctx, road)
    I, U = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED
    message = lambda: _message(ctx)
    v, f = SC.GRID_V, SC.GRID_F
    n, m = len(v), len(f)
    nrm, col = SC.attributes(n, 1)
    dv, df, dn, dc = _to(v, road), _to(f, road), _to(nrm, road), _to(col, road)
    sentinel = {"v": np.full((n, 3), 7, F), "n": np.full((n, 3), 7, F), "c": np.full((n, 3), 7, np.uint8), "f": np.full((m, 3), 7, np.uint32)}
    dev = {k: _to(a, road) for k, a in sentinel.items()}
    nv, nf = C.c_size_t(7), C.c_size_t(7)

    def call(cfg, n=n, m=m, v_ptr=True, f_ptr=True, normals=False, out_normals=False, colors=False, out_colors=False, counts=(True, True), faces=df, vertices=dv):
        torch.cuda.synchronize()
        return fn(ctx._h, ptr(vertices) if v_ptr else None, n, ptr(faces) if f_ptr else None, m, ptr(dn) if normals else None, ptr(dc) if colors else None,
                  None if cfg is None else C.byref(cfg), ptr(dev["v"]), ptr(dev["n"]) if out_normals else None, ptr(dev["c"]) if out_colors else None, n,
                  ptr(dev["f"]), m, None, C.byref(nv) if counts[0] else None, C.byref(nf) if counts[1] else None)

    def config(strategy=0, preserve_boundary=1, threshold=K.DEFAULT_ANGLE, ratio=0.5):
        return _lib.SimplifyConfigC(strategy, preserve_boundary, threshold, ratio)

    bad = config(strategy=2, ratio=float("nan"))
    # 1 before everything
    for kw in ({"v_ptr": False}, {"f_ptr": False}, {"counts": (False, True)}, {"counts": (True, False)}):
        assert call(bad, n=0, m=0, **kw) == I and "NULL" in message()
    assert call(None, n=0, m=0) == I and "config is NULL" in message()
    for kw in ({"normals": True}, {"out_normals": True}):
        assert call(bad, n=0, **kw) == I and "out_normals goes with normals" in message()
    for kw in ({"colors": True}, {"out_colors": True}):
        assert call(bad, m=0, **kw) == I and "out_colors goes with colors" in message()
    # 2 before 3, 4, 5
    assert call(bad, n=0, m=2 ** 40) == I and message() == "Mesh is empty"
    assert call(bad, n=2 ** 40, m=0) == I and message() == "Mesh is empty"
    # 3 before 4 and 5
    assert call(bad, n=2 ** 40) == I and "strategy" in message()
    assert call(config(preserve_boundary=2, ratio=-1.0), n=2 ** 40) == I and "preserve_boundary" in message()
    # 4 before 5 and 6: the ratio, then the threshold
    assert call(config(ratio=1.5, threshold=float("nan")), n=2 ** 40) == I and message() == "Reduction ratio must be between 0.0 and 1.0"
    assert call(config(threshold=float("inf")), m=2 ** 40) == I and "feature_angle_threshold" in message()
    # 5 before 6: the exact bounds
    bad_faces = _to(SC.with_index(n), road)
    assert call(config(), n=2 ** 32 - 16, faces=bad_faces) == U and "n_vertices" in message()
    assert call(config(), m=1431655760, faces=bad_faces) == U and "n_faces" in message()
    assert (nv.value, nf.value) == (7, 7) and all((_host(a) == 7).all() for a in dev.values())
    # 6, 7 and the messages of the table
    for name, vertices, faces, params, status, text in SC.LIMITS:
        lv, lf = _to(vertices, road), _to(faces, road)         # (named: the arrays live until the call has returned)
        torch.cuda.synchronize()
        got = fn(ctx._h, ptr(lv), len(vertices), ptr(lf), len(faces), None, None, C.byref(_config(params)), ptr(dev["v"]), None, None,
                 n + 2, ptr(dev["f"]), m, None, C.byref(nv), C.byref(nf))
        assert got == status and text in message(), (name, got, message())
    assert (nv.value, nf.value) == (7, 7) and all((_host(a) == 7).all() for a in dev.values())
    # the same answers through the context's methods
    for name, vertices, faces, params, status, text in SC.LIMITS:
        with pytest.raises(tc.Unsupported if status == U else tc.InvalidData, match=text.replace(".", r"\.")):
            ctx.simplify_mesh_clustering(_to(vertices, road), _to(faces, road), params["ratio"], feature_angle_threshold=params["threshold"])
    with pytest.raises(tc.InvalidData, match="Mesh is empty"):
        ctx.simplify_mesh_clustering(v, f[:0], 0.5)
    with pytest.raises(tc.Unsupported):
        ctx.simplify_mesh_clustering(v, f, 0.5, "minimum_error")
    with pytest.raises(tc.InvalidData, match="strategy"):
        ctx.simplify_mesh_clustering(v, f, 0.5, "median")


def test_launch_rows(ctx):
    """one launch set per call: each of the three stage rows once, the write-out once where there is something to write; ratio 0 stops after
    the class stage's checks"""
    def rows():
        r = {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("simplify_")}
        return tuple(r.get(k, 0) for k in ROWS), set(r) - set(ROWS)

    ctx.profile_enable(True)
    try:
        for name in ("blocks_513", f"cluster_sizes_{SC.LONG_CLUSTER + 1}", "classes_box"):
            case = SC.CASES[name]
            for road in ROADS:
                ctx.profile_reset()
                run(ctx, case, road, case["runs"][0])
                assert rows() == ((1, 1, 1, 1), set()), (name, road)
        ctx.profile_reset()
        run(ctx, SC.CASES["blocks_513"], "numpy", SC.run(0.0))
        assert rows() == ((1, 0, 0, 0), set())
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


def test_compat_agrees_with_the_context(ctx):
    case = SC.CASES["classes_open_box"]
    mesh = threecrate.TriangleMesh.from_numpy(case["vertices"], case["faces"])
    for strategy in ("centroid", "weighted_average"):
        for pb in (True, False):
            out = threecrate.ClusteringSimplifier("uniform", strategy, pb, 0.5).simplify(mesh, 0.6)
            v, f = ctx.simplify_mesh_clustering(case["vertices"], case["faces"], 0.6, strategy, pb, 0.5)
            assert isinstance(out, threecrate.TriangleMesh) and same_bits(out.vertices(), v) and same_bits(out.faces(), f)
            assert 0 < out.face_count < mesh.face_count
    default = threecrate.ClusteringSimplifier().simplify(mesh, 0.6)
    v, f = ctx.simplify_mesh_clustering(case["vertices"], case["faces"], 0.6)
    assert same_bits(default.vertices(), v) and same_bits(default.faces(), f)
    with pytest.raises(RuntimeError, match="Reduction ratio must be between 0.0 and 1.0"):
        threecrate.ClusteringSimplifier().simplify(mesh, 1.5)
    with pytest.raises(RuntimeError, match="Mesh is empty"):
        threecrate.ClusteringSimplifier().simplify(threecrate.TriangleMesh(), 0.5)
