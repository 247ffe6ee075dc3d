"""The Poisson surface on the device (include/threecrate_hip_poisson.h) against tests/poisson_checker.py on the cases of
tests/poisson_cases.py, whose budgets tests/test_poisson_cpu.py measured on the checker alone.
  bit for bit with the checker's exact mode: density, occupied_nodes, and b -- through chi at max_iterations = 1 (chi_1 = alpha b: no
      development hook; a wrong b or a wrong first inner product moves it)
  iterations: the exact checker's, or within one where its residual at the stop lies within 10 % of the tolerance
  the true residual ||b - A chi|| / ||b||, recomputed here in f64 from the device's chi: at most 4 x the exact checker's
  chi and iso_value against the f64 checker: at most 4 x the recorded distance of the exact checker from it
  the mesh; two calls are equal; the host road equals the device road; the profile rows
The stencil row counts LAUNCHES: the host enqueues rounds in chunks of 16 and looks at the stop flag between chunks, so a call that stops
after `it` iterations has launched min(max_iterations, 16 ceil(it / 16)) rounds (16 when it is 0); the rounds after the stop return at once."""
import ctypes as C

import numpy as np
import pytest

from tests import poisson_cases as CS
from tests import poisson_checker as PC
from tests.test_poisson_cpu import LONG_RUN, MEASURED_CASES, longest_run, near_tolerance

pytestmark = pytest.mark.gpu
F = np.float32
CHUNK = 16


@pytest.fixture(scope="module")
def ctx():
    import threecrate_amd as tc
    c = tc.GpuContext(0)
    yield c
    c.close()


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def launches_expected(it, max_it):
    return min(max_it, max(1, -(-it // CHUNK)) * CHUNK)


@pytest.mark.parametrize("name", MEASURED_CASES)
def test_field_against_the_checker(ctx, name):
    c, ex, f64 = CS.case(name), CS.expected(name, "exact"), CS.expected(name, "f64")
    p, q, cfg, N = c["points"], c["normals"], c["cfg"], ex["N"]
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.poisson_field(p, q, cfg)
    rows = ctx.profile_read()
    ctx.profile_enable(False)
    # the grid
    assert got["dims"] == (N, N, N) and np.array_equal(np.array(got["origin"], F), ex["origin"]) and got["voxel_size"] == (float(ex["h"]),) * 3
    # bit for bit: density, occupied nodes, b through chi_1
    assert np.array_equal(got["density"].reshape(-1).view(np.uint32), ex["W"].view(np.uint32))
    assert got["occupied_nodes"] == ex["occupied_nodes"]
    one = dict(cfg, max_iterations=1)
    chi1 = ctx.poisson_field(p, q, one, want_density=False)
    want1 = PC.run(p, q, one, "exact")
    assert chi1["iterations"] == 1 and np.array_equal(chi1["chi"].reshape(-1).view(np.uint32), want1["chi"].view(np.uint32))
    # iterations
    slack = 1 if near_tolerance(name) else 0
    print(name, "iterations", got["iterations"], ex["iterations"], "rel", got["rel_residual"], ex["rel_residual"])
    assert abs(got["iterations"] - ex["iterations"]) <= slack
    if got["iterations"] == ex["iterations"]:
        # the recurrence value is f32(sqrt(rr / bb)): one f32 rounding (2^-24) over an f64 value that differs from the checker's by the order
        # of its sums (~1e-13) and by what that does to an f32 alpha or beta once in a while; 2^-22 leaves room for neither a missing sqrt
        # nor a stale value
        assert got["rel_residual"] == pytest.approx(ex["rel_residual"], rel=2.0 ** -22)
    # the true residual
    chi = got["chi"].reshape(-1)
    pw = cfg["point_weight"]
    mine, theirs = PC.true_residual(chi, ex["b"], ex["W"], pw, N), PC.true_residual(ex["chi"], ex["b"], ex["W"], pw, N)
    print(name, "true residual", mine, theirs)
    assert mine <= 4 * theirs
    # chi and the iso value against the f64 checker
    chi_d = PC.rel_max(chi, f64["chi"])
    iso_d = abs(got["iso_value"] - f64["iso_value"]) / np.abs(f64["chi"]).max()
    print(name, "chi", chi_d, "budget", 4 * CS.MEASURED[name][0], "iso", iso_d, "budget", 4 * CS.MEASURED[name][1])
    assert chi_d <= 4 * CS.MEASURED[name][0] and iso_d <= 4 * CS.MEASURED[name][1]
    # two calls are equal; the device road equals the host road
    again = ctx.poisson_field(p, q, cfg)
    dev = ctx.poisson_field(to_dev(p), to_dev(q), cfg)
    for other in (again, dev):
        for k in ("chi", "density"):
            assert np.array_equal(host(other[k]).view(np.uint32), got[k].view(np.uint32)), k
        for k in ("iterations", "rel_residual", "iso_value", "occupied_nodes", "origin", "voxel_size", "dims"):
            assert other[k] == got[k], k
    # the profile rows
    assert rows["poisson_check"][0] == rows["poisson_splat_key"][0] == rows["poisson_splat_fold"][0] == rows["poisson_rhs"][0] == rows["poisson_iso"][0] == 1
    assert rows["poisson_stencil"][0] == rows["poisson_update"][0] == launches_expected(got["iterations"], cfg["max_iterations"])
    # (a row keeps its name across profile_reset with 0 launches: count launches, not names)
    long_launches = rows.get("poisson_fold_long", (0, 0.0))[0]
    assert long_launches == (1 if longest_run(name) > LONG_RUN else 0) == (1 if c["family"] == "dense_node" else 0)


@pytest.mark.parametrize("name", MEASURED_CASES)
def test_mesh(ctx, name):
    c, ex = CS.case(name), CS.expected(name, "exact")
    p, q, cfg, N = c["points"], c["normals"], c["cfg"], ex["N"]
    v, f, stats = ctx.poisson_reconstruct(p, q, cfg, return_stats=True)
    assert len(v) > 0 and len(f) > 0 and f.max() < len(v)
    # = the field, then marching cubes, called separately
    field = ctx.poisson_field(p, q, cfg)
    assert stats == {k: field[k] for k in stats}
    valid = None
    if cfg["min_density"] > 0:
        valid = (field["density"] >= F(cfg["min_density"])).astype(np.uint8)
        assert int(valid.sum()) == int((ex["W"] >= F(cfg["min_density"])).sum()) and 0 < valid.sum() < valid.size
    v2, _, f2 = ctx.marching_cubes(field["chi"], voxel_size=field["voxel_size"], origin=field["origin"], iso_level=field["iso_value"], normals=False, weld=True,
                                   valid=valid, layout="x_fastest")
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(f, f2)
    # the device road and a second call
    dv, df = ctx.poisson_reconstruct(to_dev(p), to_dev(q), cfg)
    assert np.array_equal(host(dv).view(np.uint32), v.view(np.uint32)) and np.array_equal(host(df).view(np.uint32), f)
    if c["family"] == "sphere":
        assert PC.is_closed(f) and PC.euler(v, f) == 2
        radial = float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - CS.RADIUS).max())
        bound = 2 * CS.RADIAL[cfg["depth"]] + float(ex["h"]) / 4
        print(name, "radial", radial, "bound", bound)
        assert radial <= bound
        # the pinned winding: right-hand normals against the outward input normals
        assert PC.signed_volume(v, f) < 0
        a, b, cc = (v[f[:, k]].astype(np.float64) for k in range(3))
        assert (np.einsum("ij,ij->i", np.cross(b - a, cc - a), (a + b + cc) / 3) <= 0).all()
    if c["family"] == "plane_patch":
        assert not PC.is_closed(f)                              # trimmed: an open surface


def test_capacity_protocol(ctx):
    from threecrate_amd import _lib
    c = CS.case("sphere_d3_pw0")
    L = _lib.load_companion("threecrate_hip_poisson.h")
    cfg = _lib.PoissonConfigC(3, 1.1, 0.0, 200, 1e-5, 0.0)
    nv, nf, stats = C.c_size_t(0), C.c_size_t(0), _lib.PoissonStatsC()
    p, q = c["points"], c["normals"]
    head = (ctx._h, p.ctypes.data, q.ctypes.data, len(p), C.byref(cfg))
    assert L.tc_poisson_reconstruct(*head, None, None, 0, 0, C.byref(nv), C.byref(nf), C.byref(stats)) == _lib.TC_OK
    v, f = np.full((nv.value, 3), 7, F), np.full((nf.value, 3), 7, np.uint32)
    nv2, nf2 = C.c_size_t(0), C.c_size_t(0)
    assert L.tc_poisson_reconstruct(*head, v.ctypes.data, f.ctypes.data, nv.value - 1, nf.value, C.byref(nv2), C.byref(nf2), C.byref(stats)) == _lib.TC_INVALID_DATA
    assert (nv2.value, nf2.value) == (nv.value, nf.value) and (v == 7).all() and (f == 7).all()
    assert L.tc_poisson_reconstruct(*head, v.ctypes.data, f.ctypes.data, nv.value, nf.value, C.byref(nv2), C.byref(nf2), C.byref(stats)) == _lib.TC_OK
    assert (f < nv.value).all()


def test_depth_6_sphere(ctx):
    c = CS.case("sphere_d6")
    ex = CS.expected("sphere_d6", "exact")
    got = ctx.poisson_field(c["points"], c["normals"], c["cfg"])
    assert got["iterations"] == ex["iterations"] == 40
    assert np.array_equal(got["density"].reshape(-1).view(np.uint32), ex["W"].view(np.uint32))
    # the checker's own two modes differ by this much after 40 iterations; the device gets 4 x that
    f64 = CS.expected("sphere_d6", "f64")
    assert PC.rel_max(got["chi"], f64["chi"]) <= 4 * PC.rel_max(ex["chi"], f64["chi"])
    v, f = ctx.poisson_reconstruct(c["points"], c["normals"], c["cfg"])
    assert len(v) and PC.is_closed(f) and PC.signed_volume(v, f) < 0


def test_depth_8_loop_smoke(ctx):
    """three iterations at depth 8: the indexing of 2^24 nodes and a partial chunk; chi against the exact checker at the same three"""
    c = CS.depth8()
    got = ctx.poisson_field(c["points"], c["normals"], c["cfg"], want_density=False)
    want = PC.run(c["points"], c["normals"], c["cfg"], "exact")
    assert got["iterations"] == want["iterations"] == 3 and got["dims"] == (256, 256, 256)
    assert got["occupied_nodes"] == want["occupied_nodes"]
    assert PC.rel_max(got["chi"], want["chi"]) <= 1e-6          # the same f32 operations; only the order inside the f64 inner products differs


def test_bad_input_through_every_road(ctx):
    import threecrate_amd as tc
    from threecrate_amd import _lib, compat
    L = _lib.load_companion("threecrate_hip_poisson.h")
    good = CS.case("small_11")
    for name, (p, q, cfg, ok) in CS.bad_inputs().items():
        cc = _lib.PoissonConfigC(cfg["depth"], cfg["scale"], cfg["point_weight"], cfg["max_iterations"], cfg["tolerance"], cfg["min_density"])
        N = 1 << min(max(cfg["depth"], 2), 8)
        for dev in (False, True):
            P, Q = (to_dev(p), to_dev(q)) if dev else (p, q)
            chi = to_dev(np.full(N ** 3, 7, F)) if dev else np.full(N ** 3, 7, F)
            ptr = (lambda a: a.data_ptr()) if dev else (lambda a: a.ctypes.data)
            grid, stats = _lib.McGridC(), _lib.PoissonStatsC(7, 7.0, 7.0, 7)
            fn = L.tc_poisson_field_device if dev else L.tc_poisson_field
            rc = fn(ctx._h, ptr(P), ptr(Q), len(p), C.byref(cc), C.byref(grid), ptr(chi), None, C.byref(stats))
            assert (rc == _lib.TC_OK) == ok and rc in (_lib.TC_OK, _lib.TC_INVALID_DATA), (name, dev, rc)
            nv, nf = C.c_size_t(7), C.c_size_t(7)
            fn2 = L.tc_poisson_reconstruct_device if dev else L.tc_poisson_reconstruct
            stats2 = _lib.PoissonStatsC(7, 7.0, 7.0, 7)
            rc2 = fn2(ctx._h, ptr(P), ptr(Q), len(p), C.byref(cc), None, None, 0, 0, C.byref(nv), C.byref(nf), C.byref(stats2))
            assert rc2 == rc, (name, dev)
            if not ok:                                          # nothing is written
                assert (host(chi) == 7).all() and stats.iterations == 7 and stats2.occupied_nodes == 7 and (nv.value, nf.value) == (7, 7)
                assert tuple(grid.dims) == (0, 0, 0)
            # the Python roads
            if ok:
                assert len(ctx.poisson_reconstruct(P, Q, cfg)[0]) > 0
            else:
                with pytest.raises(tc.InvalidData):
                    ctx.poisson_reconstruct(P, Q, cfg)
                with pytest.raises(tc.InvalidData):
                    ctx.poisson_field(P, Q, cfg)
        cloud = compat.NormalPointCloud(np.ascontiguousarray(np.concatenate([p, q], 1), F))
        pc = compat.PoissonConfig(**cfg)
        if ok:
            assert compat.poisson_reconstruct(cloud, pc).face_count > 0
        else:
            with pytest.raises((RuntimeError, ValueError)):
                compat.poisson_reconstruct(cloud, pc)
        # the context serves the next call
        assert ctx.poisson_field(good["points"], good["normals"], good["cfg"])["iterations"] == CS.expected("small_11")["iterations"]
    with pytest.raises(RuntimeError):
        compat.poisson_reconstruct(compat.NormalPointCloud())


def test_compat_with_normals_chains_the_normals_call():
    from threecrate_amd import compat
    p, _ = CS.sphere(2000)
    mesh = compat.poisson_reconstruct_with_normals(compat.PointCloud.from_numpy(p), 10, compat.PoissonConfig(depth=4))
    assert mesh.vertex_count > 0 and mesh.face_count > 0
    assert compat.PoissonConfig().depth == 6
