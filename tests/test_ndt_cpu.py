"""NDT registration without a GPU: the checker (tests/ndt_checker.py) against the reference's own unit tests
(ndt_registration.rs:299-390) and a few literals, the names, defaults and null-context behaviour of its surface
(include/threecrate_hip_ndt.h), and the preconditions of the inputs of tests/test_gpu_ndt.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import ndt_checker as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def grid_cloud(nx, ny, nz, scale=1.0):
    return np.array([[ix * scale, iy * scale, iz * scale] for ix in range(nx) for iy in range(ny) for iz in range(nz)], F)


# ---- the reference's unit tests through the checker ----
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identity_on_the_grid(dtype):
    t = grid_cloud(5, 5, 5)
    r = NC.register(t, t, None, resolution=2.0, min_points_per_voxel=2, dtype=dtype)
    assert r["score"] > 0 and r["iterations"] > 0
    assert np.linalg.norm(r["pose"][4:7]) < 1.0
    assert abs(np.linalg.norm(r["pose"][:4].astype(np.float64)) - 1.0) < 1e-5


def test_small_translation():
    t = grid_cloud(6, 6, 6)
    s = (t + np.array([0.3, 0.2, 0.1], F)).astype(F)
    r = NC.register(s, t, None, resolution=2.0, step_size=0.5, max_iterations=50, epsilon=1e-5, min_points_per_voxel=3)
    assert r["score"] > 0 and r["iterations"] <= 50


def test_errors_in_the_reference_order():
    t = grid_cloud(4, 4, 4)
    with pytest.raises(NC.NdtError, match="Source point cloud is empty"):
        NC.register(np.zeros((0, 3), F), np.zeros((0, 3), F))
    with pytest.raises(NC.NdtError, match="too few points"):
        NC.register(t, np.array([[0, 0, 0], [1, 1, 1]], F))
    with pytest.raises(NC.NdtError, match="voxel grid is empty"):
        NC.register(t, t, resolution=0.5)                       # one point per voxel, five wanted


def test_defaults():
    sig = inspect.signature(NC.register).parameters
    assert [sig[k].default for k in ("resolution", "step_size", "max_iterations", "epsilon", "min_points_per_voxel")] == [1.0, 0.1, 35, 1e-4, 5]


# ---- literals ----
def test_euler_quaternion_is_rz_ry_rx():
    r, p, y = 0.3, -0.2, 0.7
    rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    q = NC.euler_quaternion(r, p, y, np.float64)
    assert np.abs(NC.rotation_matrix(q, np.float64) - rz @ ry @ rx).max() < 1e-15
    v = np.array([0.3, -1.0, 2.0])
    assert np.abs(NC.rotate(q, v, np.float64) - rz @ ry @ rx @ v).max() < 1e-15


def test_composition_applies_the_update_on_the_left():
    dq, dt = NC.euler_quaternion(0.1, 0.2, -0.3, np.float64), np.array([1.0, -2.0, 0.5])
    pose = np.r_[NC.euler_quaternion(-0.4, 0.1, 0.2, np.float64), [0.3, 0.2, 0.1]]
    new = NC.compose(dq, dt, pose, np.float64)
    d4 = NC.matrix4(np.r_[dq, dt])
    assert np.abs(NC.matrix4(new) - d4 @ NC.matrix4(pose)).max() < 1e-15


def test_lu_solve_pivots():
    a = np.array([[0, 2, 1, 0, 0, 1], [1, 0, 0, 3, 0, 0], [4, 1, 0, 0, 1, 0], [0, 0, 5, 1, 0, 2], [1, 1, 1, 0, 0.5, 0], [0, 3, 0, 1, 1, 6]], np.float64)
    b = np.arange(1.0, 7.0)
    assert a[0, 0] == 0                                         # no solve without a row exchange
    assert np.abs(NC.lu_solve(a, b, np.float64) - np.linalg.solve(a, b)).max() < 1e-13
    assert np.abs(NC.lu_solve(a, b, np.float32) - np.linalg.solve(a, b)).max() < 1e-5
    assert NC.lu_solve(np.zeros((6, 6)), b, np.float64) is None


def test_keys_floor_and_do_not_truncate():
    res = 0.5
    p = np.array([[-0.1, -res, -1e-7], [0.0, 0.49999, 0.5], [-0.5000001, 1.0, -1.0]], F)
    assert NC.keys_of(p, res, np.float32).tolist() == [[-1, -1, -1], [0, 0, 1], [-2, 2, -2]]


def test_zero_iterations():
    t = grid_cloud(5, 5, 5)
    init = NC.start_pose()
    r = NC.register(t, t, init, resolution=2.0, min_points_per_voxel=2, max_iterations=0)
    assert r["iterations"] == 0 and r["score"] == 0 and not r["converged"] and np.array_equal(r["pose"], init)


def test_the_reported_score_belongs_to_the_last_evaluated_pose():
    src, tgt, init = NC.surface_pair(4096, 2048, 0.5)
    r = NC.register(src, tgt, init, resolution=0.5, max_iterations=1, dtype=np.float64)
    s0 = NC.evaluate(src, NC.build(tgt, 0.5, 5, np.float64), init, 0.5, np.float64)[0]
    assert r["score"] == s0 and not np.array_equal(r["pose"], init.astype(np.float64))


# ---- what is this feature's own of the surface (tests/test_abi_surfaces.py holds header, table, Rust file and library together) ----
def test_rust_facade_has_the_reference_names_and_defaults():
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ("ndt_registration", "ndt_registration_default"):
        assert re.search(r"pub fn " + fn + r"\(", lib_rs), fn
    for st in ("NdtConfig", "NdtResult"):
        assert re.search(r"pub struct " + st + r"\b", lib_rs), st
    assert re.search(r"resolution: 1\.0, step_size: 0\.1, max_iterations: 35, epsilon: 1e-4, min_points_per_voxel: 5", lib_rs)


def test_every_ndt_export_returns_a_status_and_writes_nothing_without_a_context():
    L = _lib.load()
    pts = np.zeros((8, 3), F)
    cfg = _lib.NdtConfigC(1.0, 0.1, 35, 1e-4, 5)
    r = _lib.NdtResultC()
    r.iterations, r.score, r.n_voxels = 7, 7.0, 7
    for fn in (L.tc_ndt_registration, L.tc_ndt_registration_device):
        assert fn(None, pts.ctypes.data, 8, pts.ctypes.data, 8, None, C.byref(cfg), C.byref(r)) == _lib.TC_INVALID_DATA
    assert (r.iterations, r.score, r.n_voxels) == (7, 7.0, 7)
    nv = C.c_size_t(7)
    for fn in (L.tc_ndt_voxels, L.tc_ndt_voxels_device):
        assert fn(None, pts.ctypes.data, 8, 1.0, 5, None, None, None, None, 0, C.byref(nv)) == _lib.TC_INVALID_DATA
    assert nv.value == 7


def test_python_surface():
    import threecrate_amd as tc
    import threecrate_amd.compat as threecrate
    sig = inspect.signature(tc.GpuContext.ndt_registration).parameters
    assert list(sig)[1:] == ["source", "target", "init", "resolution", "step_size", "max_iterations", "epsilon", "min_points_per_voxel"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, 1.0, 0.1, 35, 1e-4, 5]
    sig = inspect.signature(tc.GpuContext.ndt_voxels).parameters
    assert list(sig)[1:] == ["target", "resolution", "min_points_per_voxel"] and sig["min_points_per_voxel"].default == 5
    for name in ("ndt_registration", "ndt_registration_default", "NdtConfig", "NdtResult"):
        assert hasattr(tc, name), name
    cfg = tc.NdtConfig()
    assert (cfg.resolution, cfg.step_size, cfg.max_iterations, cfg.epsilon, cfg.min_points_per_voxel) == (1.0, 0.1, 35, 1e-4, 5)
    assert list(inspect.signature(tc.ndt_registration).parameters)[:4] == ["source", "target", "init", "config"]
    assert "ndt_registration" in threecrate.__all__ and "NdtResult" in threecrate.__all__
    sig = inspect.signature(threecrate.ndt_registration).parameters                       # threecrate-python/src/lib.rs:1166-1174
    assert list(sig) == ["source", "target", "init_transform", "resolution", "step_size", "max_iterations", "epsilon", "min_points_per_voxel"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, 1.0, 0.1, 35, 1e-4, 5]
    r = threecrate.NdtResult(tc.NdtResult(NC.IDENTITY.copy(), 12.5, 3, True))
    assert repr(r) == "NdtResult(converged=true, score=12.500000, iterations=3)"
    assert r.transformation().dtype == np.float32 and np.array_equal(r.transformation(), np.eye(4, dtype=F))
    assert (r.score, r.iterations, r.converged) == (12.5, 3, True)
    assert "NDT, " not in threecrate.__doc__.split("Everything else")[1]                 # no longer listed as out of scope


# ---- preconditions of the GPU inputs, by the checker alone ----
FAMILIES = {            # name: (n_target, n_source, resolution)
    "small": (4096, 2048, 0.5),
    "large": (20000, 10000, 0.25),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_one_step_inputs_are_clean_and_well_conditioned(family):
    """(a) no transformed coordinate within FACE_MARGIN of a face, the same keys in f32 and f64; (b) the same iterations and converged; (c) the
    f32-to-f64 distances of the one-step pose and score, printed: the GPU tests take 4 x their family's maximum as their budget."""
    nt, ns, res = FAMILIES[family]
    src, tgt, init = NC.surface_pair(nt, ns, res)
    a = NC.register(src, tgt, init, resolution=res, max_iterations=1, dtype=np.float32)
    b = NC.register(src, tgt, init, resolution=res, max_iterations=1, dtype=np.float64)
    assert b["evals"][0]["face"] >= NC.FACE_MARGIN and np.array_equal(a["evals"][0]["keys"], b["evals"][0]["keys"])
    assert np.array_equal(NC.keys_of(tgt, res, np.float32), NC.keys_of(tgt, res, np.float64))
    assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"]) == (1, False)
    assert a["n_voxels"] == b["n_voxels"] and a["n_hits"] == b["n_hits"] and b["n_hits"] > 0.9 * ns
    g = NC.build(tgt, res, 5, np.float64)
    H = NC.evaluate(src, g, init, res, np.float64)[2]
    cond = np.linalg.cond(H + np.eye(6) * 1e-6)
    fro, rel = NC.distances(a, b)
    print(f"{family}: {b['n_voxels']} voxels, {b['n_hits']} hits, cond(H) = {cond:.0f}, |delta32 - delta64| = {np.linalg.norm(a['deltas'][0] - b['deltas'][0]):.2e}, "
          f"pose {fro:.2e}, score {rel:.2e}")
    assert cond < 1e3 and 0 < fro < 1e-5 and rel < 1e-4


def test_default_loop_input_is_clean():
    nt, ns, res = FAMILIES["small"]
    src, tgt, init = NC.surface_pair(nt, ns, res, max_iterations=35)
    a = NC.register(src, tgt, init, resolution=res, dtype=np.float32)
    b = NC.register(src, tgt, init, resolution=res, dtype=np.float64)
    assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"]) and b["converged"] and 2 < b["iterations"] < 35
    assert min(r["face"] for r in b["evals"]) >= NC.FACE_MARGIN
    assert all(np.array_equal(x["keys"], y["keys"]) for x, y in zip(a["evals"], b["evals"]))
    fro, rel = NC.distances(a, b)
    print(f"default loop: {b['iterations']} iterations, pose {fro:.2e}, score {rel:.2e}")
    # the registration works: the source ends nearer to the surface than it started
    off = lambda p: np.abs(p[:, 2] - (0.4 * np.sin(1.7 * p[:, 0]) * np.cos(1.3 * p[:, 1]) + 0.15 * p[:, 0])).mean()
    assert off(NC.apply(b["pose"], src, np.float64)) < 0.5 * off(NC.apply(init, src, np.float64))
