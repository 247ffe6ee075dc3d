"""TSDF fusion and surface extraction without a GPU: the numpy checker (tests/tsdf_checker.py) against the figures measured on the
reference's own scene, the reference's five unit tests restated on it, the recurrence and the edge rules by hand, the library's
validation (which comes before any device work), the facade's surface -- and, for every input of tests/test_gpu_tsdf.py, the proof that
it contains what it is there for and that every checker mutant differs from the checker on at least one of them."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import tsdf_checker as T

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(depths, rgb=None, max_weight=100):
    intr = T.Intrinsics(*T.SCENE_CAMERA)
    vol, w2c = T.scene_volume(max_weight), T.world_to_camera(T.IDENTITY_POSE)
    out = [T.integrate(vol, T.constant_depth(intr, d), intr, w2c, rgb) for d in depths]
    return vol, out


@pytest.fixture(scope="module")
def scene03():
    return _scene([0.3])


# ---- the figures of the reference's scene: 32^3 voxels of 0.02, tau 0.1, origin (-0.32, -0.32, 0), 640 x 480, identity pose ----
def test_checker_reproduces_the_measured_figures(scene03):
    vol, (r,) = scene03
    assert r["n_updated"] == 11146 == int((vol.weight > 0).sum())
    xyz, _, _ = T.extract(vol, 0.0, 0)
    assert len(xyz) == 3231 and round(float(xyz[:, 2].astype(np.float64).mean()), 4) == 0.4125
    xyz, _, _ = T.extract(vol, 0.0, T.OBSERVED_EDGES)
    assert len(xyz) == 925 and round(float(xyz[:, 2].astype(np.float64).mean()), 4) == 0.3000
    vol, (r,) = _scene([0.5])
    xyz, _, _ = T.extract(vol)
    assert r["n_updated"] == 11146 and len(xyz) == 10978 and round(float(xyz[:, 2].astype(np.float64).mean()), 4) == 0.5039


def test_the_references_bound_holds_only_through_its_conversion_accident():
    """The second row of the table: the shader as it is -- no c_z test, u32() of a negative or NaN coordinate clamped to 0 -- fuses 20 029
    voxels (every voxel left of or above the frustum with pixel column / row 0), and only then does the shader's extraction rule give a
    mean z inside the reference's 0.2 < mean z < 0.4."""
    intr = T.Intrinsics(*T.SCENE_CAMERA)
    vol = T.scene_volume()
    r = T.integrate(vol, T.constant_depth(intr, 0.3), intr, T.world_to_camera(T.IDENTITY_POSE), shader_conversion=True)
    xyz, _, _ = T.extract(vol, 0.0, 0)
    z = float(xyz[:, 2].astype(np.float64).mean())
    assert r["n_updated"] == 20029 == int((vol.weight > 0).sum()) and len(xyz) == 5063
    assert round(z, 3) == 0.380 and 0.2 < z < 0.4


# ---- the reference's five unit tests (tsdf.rs:890-1144) on the checker ----
def test_basic_integration_updates_voxels_and_returns_all_of_them():
    vol, (r,) = _scene([0.5])
    assert vol.tsdf.shape == vol.weight.shape == (32 * 32 * 32,) and vol.rgb.shape == (32 * 32 * 32, 3)
    assert r["n_updated"] > 0 and (vol.weight > 0).sum() == r["n_updated"]


def test_multiple_integrations_raise_the_weight():
    vol, rs = _scene([0.25, 0.3, 0.35])
    assert vol.weight.max() == 3 > 1
    assert [r["n_updated"] for r in rs] == [11146] * 3
    assert len(T.extract(vol, 0.0, 0)[0]) == 3231 and len(T.extract(vol, 0.0, T.OBSERVED_EDGES)[0]) == 925


def test_a_red_image_gives_red_points():
    red = np.zeros((480, 640, 3), np.uint8)
    red[..., 0] = 255
    vol, _ = _scene([0.3], rgb=red)
    xyz, rgb, _ = T.extract(vol)
    assert len(xyz) > 0 and (rgb[:, 0] > 200).sum() > 0
    assert (rgb == (255, 0, 0)).all()          # alpha = 1 on the first frame: the pixel itself


def test_coordinate_system_bounds():
    vol = T.scene_volume()
    hi = vol.origin + np.asarray(vol.res, F) * vol.vs
    assert np.allclose(hi, (0.32, 0.32, 0.64), atol=0.01)
    p = np.array([0.1, 0.2, 0.3, 1.0])
    m = T.world_to_camera(T.IDENTITY_POSE).reshape(3, 4).astype(np.float64)
    assert np.allclose(m @ p, p[:3], atol=1e-3)


def test_mean_z_bound_holds_with_observed_edges_and_not_without(scene03):
    """The reference asserts 0.2 < mean z < 0.4 for depth 0.3.  With the shader's extraction rule on a cleanly integrated frustum the
    mean is 0.4125: unobserved voxels beside observed voxels BEHIND the surface read as + truncation, so every such pair is a sign
    change, and the frustum's boundary behind the surface becomes a sheet of points that pulls the mean up.  (The reference passes its
    own bound only because its shader fuses every voxel left of or above the frustum with pixel column / row 0.)  With
    TC_TSDF_OBSERVED_EDGES the sheet is gone and the points sit on the surface."""
    vol, _ = scene03
    z = T.extract(vol, 0.0, T.OBSERVED_EDGES)[0][:, 2].astype(np.float64)
    assert 0.2 < z.mean() < 0.4 and np.allclose(z, 0.3, atol=1e-6)
    z = T.extract(vol, 0.0, 0)[0][:, 2].astype(np.float64)
    assert not z.mean() < 0.4 and round(float(z.mean()), 4) == 0.4125


# ---- the recurrence ----
def test_recurrence_at_the_cap():
    """max_weight 3, five frames: alpha is 1, 1/2, 1/3, then stays 1/3"""
    vol, _ = _scene([0.30, 0.32, 0.34, 0.36, 0.38], max_weight=3)
    seen = vol.weight > 0
    assert set(np.unique(vol.weight[seen])) == {3}
    i = np.nonzero(seen)[0][0]
    x, y, z = (c[i] for c in vol.coords())
    cz = F(z) * vol.vs + vol.origin[2]
    tsdf, w = F(1.0), 0
    for d in (0.30, 0.32, 0.34, 0.36, 0.38):
        t = min(max(F(d) - cz, -vol.tau), vol.tau)
        w = min(w + 1, 3)
        alpha = F(1.0) / F(w)
        tsdf = (F(1.0) - alpha) * tsdf + alpha * t
    assert alpha == F(1.0) / F(3.0) and vol.tsdf[i] == tsdf


def test_a_black_pixel_leaves_the_colour_alone():
    intr = T.Intrinsics(*T.SCENE_CAMERA)
    vol, w2c = T.scene_volume(), T.world_to_camera(T.IDENTITY_POSE)
    green = np.zeros((480, 640, 3), np.uint8)
    green[..., 1] = 200
    T.integrate(vol, T.constant_depth(intr, 0.3), intr, w2c, green)
    before = vol.rgb.copy()
    T.integrate(vol, T.constant_depth(intr, 0.3), intr, w2c, np.zeros((480, 640, 3), np.uint8))
    assert vol.weight.max() == 2 and np.array_equal(vol.rgb, before) and (before[vol.weight > 0] == (0, 200, 0)).all()
    blue = np.zeros((480, 640, 3), np.uint8)
    blue[..., 2] = 90
    T.integrate(vol, T.constant_depth(intr, 0.3), intr, w2c, blue)
    third = F(1.0) / F(3.0)
    g = np.uint8(min(max((F(1.0) - third) * F(200.0) + third * F(0.0), F(0.0)), F(255.0)))
    b = np.uint8(min(max((F(1.0) - third) * F(0.0) + third * F(90.0), F(0.0)), F(255.0)))
    assert (vol.rgb[vol.weight > 0] == (0, g, b)).all()


# ---- extraction's edge rules by hand: a 2 x 2 x 2 volume is one cube ----
def _one_cube(values, weights=None, iso=0.0, flags=0, mutant=None):
    vol = T.Volume(0.5, 0.1, (2, 2, 2), (1.0, 2.0, 3.0))
    vol.load(np.asarray(values, F), np.ones(8, np.uint8) if weights is None else weights)
    return T.extract(vol, iso, flags, mutant)


def test_edge_rules_by_hand():
    pos = [F(0.5)] * 8
    # a crossing with |va - vb| < 1e-5 along 000-100: the midpoint, not the interpolation
    v = list(pos)
    v[0], v[1] = F(-3e-6), F(3e-6)
    xyz, _, cnt = _one_cube(v)
    assert cnt.tolist() == [3] and xyz[0].tolist() == [1.25, 2.0, 3.0]          # 0.5 (1.0 + 1.5)
    assert xyz[1].tolist()[0] == 1.0 and xyz[1].tolist()[2] == 3.0 and 2.0 <= xyz[1][1] < 2.0001         # 000-010: interpolated, nearly at 000
    # va = 0 exactly: the product is 0 on all three edges of corner 000, s = 0 / (0 - vb) = -0 -> clamped: the corner itself
    v = list(pos)
    v[0] = F(0.0)
    xyz, _, cnt = _one_cube(v)
    assert cnt.tolist() == [3] and (xyz == (1.0, 2.0, 3.0)).all()
    # two positive values whose product underflows to 0 emit: the rule is the f32 product, not the signs
    v = list(pos)
    v[6], v[7] = F(1e-30), F(1e-30)
    assert F(1e-30) * F(1e-30) == 0 and F(1e-30) * F(0.5) > 0
    xyz, _, cnt = _one_cube(v)
    assert cnt.tolist() == [1] and xyz[0].tolist() == [1.25, 2.5, 3.5]          # 011-111, |va - vb| = 0: the midpoint
    # an unobserved corner reads + truncation, not truncation - iso: with iso 0.2 > tau the two differ in sign, and 0.5 - 0.2 > 0
    w = np.ones(8, np.uint8)
    w[1] = 0
    assert _one_cube(pos, w, iso=0.2)[2].tolist() == [0] and _one_cube(pos, w, iso=0.2, mutant="tau_minus_iso")[2].tolist() == [3]
    # ... and beside an observed negative corner it is a sign change, unless both ends must be observed
    neg = [F(-0.05)] * 8
    assert _one_cube(neg, w)[2].tolist() == [3] and _one_cube(neg, w, flags=T.OBSERVED_EDGES)[2].tolist() == [0]
    # a base voxel without weight emits nothing, whatever its neighbours say
    w = np.ones(8, np.uint8)
    w[0] = 0
    assert _one_cube([F(-0.5)] + pos[1:], w)[2].tolist() == [0]


def test_edge_order_is_the_shaders():
    """every corner its own value: one sign change per edge in turn names the edge by the point it emits"""
    for e, (a, b, axis) in enumerate(T.EDGES):
        v = [F(0.5)] * 8
        v[a] = F(-0.5)
        xyz, _, cnt = _one_cube(v)
        corner = lambda c: np.array([1.0 + 0.5 * (c & 1), 2.0 + 0.5 * ((c >> 1) & 1), 3.0 + 0.5 * (c >> 2)])
        mids = [0.5 * (corner(p) + corner(q)) for p, q, _ in T.EDGES if a in (p, q)]
        assert cnt.tolist() == [3] and b == a + (1 << axis)
        assert np.allclose(xyz, mids)           # in the order of T.EDGES


# ---- the library's validation: before any device work, so it answers without a GPU ----
def _cfg(voxel_size=0.02, tau=0.1, res=(4, 4, 4), origin=(0, 0, 0), max_weight=100):
    return _lib.TsdfVolumeConfigC(voxel_size, tau, (C.c_uint32 * 3)(*res), (C.c_float * 3)(*origin), max_weight)


VALIDATION_ROWS = [
    ("voxel_size 0", dict(voxel_size=0.0)), ("voxel_size negative", dict(voxel_size=-1.0)), ("voxel_size NaN", dict(voxel_size=float("nan"))),
    ("voxel_size inf", dict(voxel_size=float("inf"))), ("truncation 0", dict(tau=0.0)), ("truncation NaN", dict(tau=float("nan"))),
    ("truncation inf", dict(tau=float("inf"))), ("resolution 0", dict(res=(4, 0, 4))), ("origin NaN", dict(origin=(0, float("nan"), 0))),
    ("origin inf", dict(origin=(float("inf"), 0, 0))), ("max_weight 0", dict(max_weight=0)), ("max_weight 256", dict(max_weight=256)),
    ("far corner overflows", dict(voxel_size=1e38, res=(4, 4, 4))), ("far corner overflows with the origin", dict(voxel_size=1e38, res=(2, 2, 2), origin=(3e38, 0, 0))),
]


@pytest.mark.parametrize("name,kw", VALIDATION_ROWS, ids=[r[0] for r in VALIDATION_ROWS])
def test_create_rejects_a_bad_config(name, kw):
    """(Without a context a good config is TC_INVALID_DATA as well: what this shows is that no row crashes or hands out a handle.  The rows
    are told apart from a good config, by their messages, in tests/test_gpu_tsdf.py::test_validation_rows_with_their_messages, which
    takes them from here.)"""
    L, out = _lib.load(), C.c_void_p(7)
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg(**kw)), C.byref(out)) == _lib.TC_INVALID_DATA and not out.value


def test_create_checks_the_config_before_it_needs_a_device():
    """without a context every answer is an error; WHICH one shows that the config was read first: 2^28 voxels are a config without
    a context (TC_INVALID_DATA), one voxel more is TC_UNSUPPORTED"""
    L, out = _lib.load(), C.c_void_p(7)
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg(res=(1 << 14, 1 << 14, 1))), C.byref(out)) == _lib.TC_INVALID_DATA and not out.value
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg(res=(1 << 14, 1 << 14, 2))), C.byref(out)) == _lib.TC_UNSUPPORTED
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg(res=((1 << 28) + 1, 1, 1))), C.byref(out)) == _lib.TC_UNSUPPORTED
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg(res=(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF))), C.byref(out)) == _lib.TC_UNSUPPORTED
    assert L.tc_tsdf_volume_create(None, None, C.byref(out)) == _lib.TC_INVALID_DATA
    assert L.tc_tsdf_volume_create(None, C.byref(_cfg()), None) == _lib.TC_INVALID_DATA


def test_every_call_on_a_null_handle_is_invalid_data_and_writes_nothing():
    L = _lib.load()
    buf = np.full(64, 7, np.uint8)
    k, m, n = _lib.CameraIntrinsicsC(1, 1, 0, 0, 4, 4), (C.c_float * 12)(), C.c_size_t(7)
    L.tc_tsdf_volume_destroy(None)
    assert L.tc_tsdf_volume_reset(None) == _lib.TC_INVALID_DATA
    for fn in (L.tc_tsdf_integrate, L.tc_tsdf_integrate_device):
        assert fn(None, buf.ctypes.data, None, C.byref(k), m, C.byref(n)) == _lib.TC_INVALID_DATA
    for fn in (L.tc_tsdf_volume_download, L.tc_tsdf_volume_download_device, L.tc_tsdf_volume_upload, L.tc_tsdf_volume_upload_device):
        assert fn(None, buf.ctypes.data, buf.ctypes.data, None) == _lib.TC_INVALID_DATA
    for fn in (L.tc_tsdf_extract_surface, L.tc_tsdf_extract_surface_device):
        assert fn(None, 0.0, 0, buf.ctypes.data, None, 1, C.byref(n)) == _lib.TC_INVALID_DATA
    assert n.value == 7 and (buf == 7).all()


# ---- the facade ----
def test_python_surface():
    import threecrate_amd as tc
    sig = inspect.signature(tc.GpuContext.tsdf_volume).parameters
    assert list(sig)[1:] == ["voxel_size", "truncation_distance", "resolution", "origin", "max_weight"]
    assert (sig["origin"].default, sig["max_weight"].default) == ((0, 0, 0), 100)
    assert issubclass(tc.TsdfVolume, tc.api._Handle) and tc.TsdfVolume._destroy == "tc_tsdf_volume_destroy"
    sig = inspect.signature(tc.TsdfVolume.integrate).parameters
    assert list(sig)[1:] == ["depth", "intrinsics", "camera_pose", "color", "world_to_camera", "count"]
    assert [sig[k].default for k in list(sig)[3:]] == [None, None, None, False]
    sig = inspect.signature(tc.TsdfVolume.extract_surface).parameters
    assert (sig["iso_value"].default, sig["observed_only"].default) == (0.0, False)
    for name in ("reset", "voxels", "load"):
        assert callable(getattr(tc.TsdfVolume, name))
    for name in ("CameraIntrinsics", "TsdfVolume", "create_tsdf_volume", "gpu_tsdf_integrate", "gpu_tsdf_extract_surface"):
        assert hasattr(tc, name) and name in tc.__all__, name
    k = tc.CameraIntrinsics(525.0, 525.0, 319.5, 239.5, 640, 480)
    assert k.depth_scale == 1.0
    assert list(inspect.signature(tc.gpu_tsdf_integrate).parameters) == ["gpu_context", "volume", "depth_image", "color_image", "camera_pose", "intrinsics"]
    assert list(inspect.signature(tc.gpu_tsdf_extract_surface).parameters) == ["gpu_context", "volume", "voxels", "iso_value"]


def test_pose_inversion_is_float64_rounded_once_and_a_singular_pose_is_the_references_error():
    import threecrate_amd as tc
    p = T.POSES["skew"]
    m = tc.TsdfVolume._world_to_camera(p, None)
    assert m.dtype == np.float32 and np.array_equal(m, T.world_to_camera(p))
    assert np.array_equal(tc.TsdfVolume._world_to_camera(None, None), np.eye(4, dtype=F)[:3].reshape(12))
    assert np.array_equal(tc.TsdfVolume._world_to_camera(None, m.reshape(3, 4)), m)
    with pytest.raises(tc.GpuError, match="Failed to invert camera pose matrix"):
        tc.TsdfVolume._world_to_camera(np.zeros((4, 4)), None)
    with pytest.raises(tc.InvalidData):
        tc.TsdfVolume._world_to_camera(p, m)


def test_rust_facade_has_the_reference_names():
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ("create_tsdf_volume", "gpu_tsdf_integrate", "gpu_tsdf_extract_surface"):
        assert re.search(r"^pub fn " + fn + r"\(", lib_rs, re.M), fn
    for st in ("TsdfVolume", "TsdfVoxel", "CameraIntrinsics", "TsdfVolumeGpu"):
        assert re.search(r"^pub struct " + st + r"\b", lib_rs, re.M), st
    assert re.search(r"^pub struct TsdfVolumeGpu<'a> \{[^}]*PhantomData<&'a HipContext>", lib_rs, re.M)     # cannot outlive its context
    body = lib_rs[lib_rs.index("impl<'a> TsdfVolumeGpu<'a>"):]
    for fn in ("new", "integrate", "download_voxels", "extract_surface"):
        assert re.search(r"pub fn " + fn + r"\(", body), fn
    assert re.search(r"pub depth_scale: f32", lib_rs)


def test_block_constants_are_the_ones_the_tests_name():
    h = open(os.path.join(ROOT, "threecrate_amd", "csrc", "tc_internal.h")).read()
    assert re.search(r"constexpr int kTsdfBlock = 256, kTsdfRun = 64;", h)
    assert 256 // 64 == T.CUBE_BLOCK_RUNS
    blocks = lambda rx, ry, rz: -(-(-(-(rx - 1) // 64) * (ry - 1) * (rz - 1)) // T.CUBE_BLOCK_RUNS)
    assert blocks(*T.MANY_BLOCKS) > 2049
    # the smallest volume that gets there: a run costs at least two voxels per (ry, rz) pair (rx = 2 gives one run per row of cubes, a wider
    # row the same run for more voxels, and a second run only from rx = 66), so search 2 x ry x rz
    need = 2049 * T.CUBE_BLOCK_RUNS + 1                                             # runs
    least_rz = lambda ry: max(ry, -(-need // (ry - 1)) + 1)                         # the first rz >= ry with enough rows of cubes
    assert all(blocks(2, ry, least_rz(ry)) > 2049 and (least_rz(ry) == ry or blocks(2, ry, least_rz(ry) - 1) <= 2049) for ry in range(2, 200))
    best = min((2 * ry * least_rz(ry), (2, ry, least_rz(ry))) for ry in range(2, 200))
    assert best == (T.MANY_BLOCKS[0] * T.MANY_BLOCKS[1] * T.MANY_BLOCKS[2], T.MANY_BLOCKS) == (16766, (2, 83, 101))


# ---- what every GPU input is there for, by the checker alone ----
@pytest.fixture(scope="module")
def integration_runs():
    """name -> (volume after its frames, the per-frame dicts, the state before the last frame)"""
    runs = {}
    for name, (vol, frames) in T.integration_cases().items():
        rs = []
        for depth, rgb, intr, m in frames:
            before = vol.copy()
            rs.append(T.integrate(vol, depth, intr, m, rgb))
        runs[name] = (vol, rs, before)
    return runs


def test_integration_inputs_contain_what_they_are_there_for(integration_runs):
    total = {k: 0 for k in ("half", "behind", "before_image", "beyond_image", "zero_depth", "negative_depth", "nan_depth", "inf_depth")}
    for name, (vol, rs, before) in integration_runs.items():
        print(f"{name}: {rs}")
        for r in rs:
            for k in total:
                total[k] += r[k]
        if "away" in name:
            assert rs[0]["n_updated"] == 0 and rs[0]["behind"] == vol.n
            assert np.array_equal(vol.tsdf, before.tsdf) and np.array_equal(vol.weight, before.weight)
        else:
            assert rs[-1]["n_updated"] > 0, name
    assert all(v > 0 for v in total.values()), total
    # the one case with everything: a pixel changed by the + 0.5, and voxels skipped by every rule but "behind" (the camera is in front)
    r = integration_runs["32x32x32 identity"][1][0]
    assert min(r["half"], r["before_image"], r["beyond_image"], r["zero_depth"], r["negative_depth"], r["nan_depth"], r["inf_depth"]) > 0
    assert r["behind"] == 0
    # every case whose image has the three flawed pixels samples each of them, or says which it does not (small volumes see few pixels)
    for name in ("32x32x32 skew", "32x32x32 inside"):
        r = integration_runs[name][1][0]
        assert min(r["zero_depth"], r["negative_depth"], r["nan_depth"], r["inf_depth"]) > 0, (name, r)
    r = integration_runs["32x32x32 inside"][1][0]
    assert r["behind"] > 0 and r["n_updated"] > 0
    vol, rs, _ = integration_runs["32x32x32 corner"]
    x, y, z = vol.coords()
    seen = vol.weight > 0
    assert 0 < seen.sum() < vol.n // 16 and x[seen].min() >= 16 and y[seen].min() >= 16          # a corner only
    # wide rows: whole runs of 64 voxels without an updated voxel beside runs with some (the wave-level skip has both to serve)
    vol, _, _ = integration_runs["257x5x3 identity"]
    per_run = [(vol.weight.reshape(3, 5, 257)[:, :, s:s + 64] > 0).sum() for s in range(0, 257, 64)]
    assert min(per_run) == 0 < max(per_run)
    # three frames: the weights reach the cap and no further; the colour was left alone somewhere and changed somewhere
    for mw in (1, 3, 255):
        vol, rs, _ = integration_runs[f"65x4x5 three frames max_weight {mw}"]
        assert vol.weight.max() == min(mw, 3) and len(rs) == 3
    vol, _, _ = integration_runs["32x32x32 three frames"]
    seen = vol.weight > 0
    assert (vol.rgb[seen].any(1)).any() and (~vol.rgb[seen].any(1)).any() and len(np.unique(vol.weight)) == 4


EXTRACTION_INPUTS = T.RESOLUTIONS + [T.MANY_BLOCKS]


def test_extraction_inputs_contain_what_they_are_there_for():
    seen_counts = set()
    for res in EXTRACTION_INPUTS:
        vol = T.extraction_state(res)
        for iso in (0.0, 0.03, -0.03):
            for flags in (0, T.OBSERVED_EDGES):
                xyz, rgb, cnt = T.extract(vol, iso, flags)
                assert len(xyz) == len(rgb) == cnt.sum()
                if min(res) >= 2:
                    seen_counts |= set(cnt.tolist())
        print(f"{res}: {len(T.extract(vol)[0])} points from {max(0, res[0] - 1) * max(0, res[1] - 1) * max(0, res[2] - 1)} cubes")
    assert {0, 1} <= seen_counts and max(seen_counts) >= 6
    for res in [r for r in EXTRACTION_INPUTS if min(r) < 2]:
        assert len(T.extract(T.extraction_state(res))[0]) == 0          # no cube: an empty result
    vol = T.extraction_state((65, 4, 5))
    rx, ry, rz = vol.res
    t, w = vol.tsdf.reshape(rz, ry, rx), vol.weight.reshape(rz, ry, rx)
    # an unobserved voxel beside an observed negative one (along x): the pair the flag is about
    assert ((w[:, :, 1:] == 0) & (w[:, :, :-1] > 0) & (t[:, :, :-1] < 0)).any()
    both = (w[:, :, 1:] > 0) & (w[:, :, :-1] > 0)
    a, b = t[:, :, :-1], t[:, :, 1:]
    with np.errstate(all="ignore"):
        assert (both & (a * b <= 0) & (np.abs(a - b) < F(1e-5)) & (a != b)).any()             # a crossing nearer than 1e-5
        assert (both & (a == 0) & (b != 0)).any()                                             # va = 0 exactly
        assert (both & (a * b == 0) & (a != 0) & (b != 0)).any()                              # a product that underflows
    assert (t == F(0.03)).any() and (t == F(-0.03)).any()                                     # exact zeros at the other iso values


def test_every_mutant_differs_from_the_checker_on_some_gpu_input(integration_runs):
    table = {}
    for mutant in T.INTEGRATE_MUTANTS:
        hits = []
        for name, (vol, frames) in T.integration_cases().items():
            for depth, rgb, intr, m in frames:
                T.integrate(vol, depth, intr, m, rgb, mutant=mutant)
            good = integration_runs[name][0]
            if not (np.array_equal(vol.tsdf, good.tsdf) and np.array_equal(vol.weight, good.weight) and np.array_equal(vol.rgb, good.rgb)):
                hits.append(name)
        table[mutant] = hits
    for mutant in T.EXTRACT_MUTANTS:
        hits = []
        for res in EXTRACTION_INPUTS:
            vol = T.extraction_state(res)
            for iso in (0.0, 0.03, -0.03):
                for flags in (0, T.OBSERVED_EDGES):
                    g, m = T.extract(vol, iso, flags), T.extract(vol, iso, flags, mutant=mutant)
                    if not (np.array_equal(g[0].view(np.uint32), m[0].view(np.uint32)) and np.array_equal(g[1], m[1])):
                        hits.append((res, iso, flags))
        table[mutant] = hits
    for mutant, hits in table.items():
        print(f"{mutant:24s} differs on {len(hits)} inputs, first: {hits[:1]}")
    assert all(table.values()), [m for m, h in table.items() if not h]
