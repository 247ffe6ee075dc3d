"""TSDF fusion and surface extraction on the device (csrc/tsdf.hip, include/threecrate_hip_tsdf.h) against the numpy checker
(tests/tsdf_checker.py), bit for bit: the checker performs the header's operations in the header's order in float32, the library is
built without contraction and divides with the IEEE division, so there is no tolerance to give.  tests/test_tsdf_cpu.py proves on
the checker alone what each input below contains.

Integration: rows of 1, 2, 63, 64, 65 and 257 voxels (either side of a run of kTsdfRun = 64, several runs per row, rows with runs
nothing projects into) with 1..5 rows and slices, and 32^3; five poses; depth with zeros, a NaN, an inf and a negative pixel; three
coloured frames at max_weight 1, 3, 255; the numpy and the torch road.  Extraction runs on states set through upload, so that it is
tested on its own: the same shapes, one volume of more than 2 049 cube blocks (a block is kTsdfBlock / kTsdfRun = 4 runs) with the fused
and the two-level scan, three iso values, both flag values."""
import ctypes as C

import numpy as np
import pytest

import threecrate_amd as tc
from threecrate_amd import _lib
from tests import tsdf_checker as T

pytestmark = pytest.mark.gpu

F = np.float32
CASES = T.integration_cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(ctx, vol):
    return ctx.tsdf_volume(float(vol.vs), float(vol.tau), vol.res, [float(o) for o in vol.origin], vol.max_weight)


def intrinsics(i):
    return tc.CameraIntrinsics(float(i.fx), float(i.fy), float(i.cx), float(i.cy), i.width, i.height)


def assert_state(v, vol, what=""):
    tsdf, weight, rgb = v.voxels()
    rx, ry, rz = vol.res
    assert tsdf.shape == (rz, ry, rx) and weight.shape == (rz, ry, rx) and rgb.shape == (rz, ry, rx, 3)
    bad = np.nonzero(bits(tsdf).ravel() != bits(vol.tsdf))[0]
    assert bad.size == 0, f"{what}: {bad.size} tsdf values differ, first voxel {bad[:1]}: {tsdf.ravel()[bad[:1]]} != {vol.tsdf[bad[:1]]}"
    assert np.array_equal(weight.ravel(), vol.weight), what
    assert np.array_equal(rgb.reshape(-1, 3), vol.rgb), what


def assert_points(got, want, what=""):
    (xyz, rgb), (wxyz, wrgb, _) = got, want
    assert xyz.shape == wxyz.shape and rgb.shape == wrgb.shape, f"{what}: {len(xyz)} points, the checker has {len(wxyz)}"
    assert xyz.dtype == np.float32 and rgb.dtype == np.uint8
    bad = np.nonzero((bits(xyz) != bits(wxyz)).any(1))[0]
    assert bad.size == 0, f"{what}: {bad.size} points differ, first {bad[:1]}: {xyz[bad[:1]]} != {wxyz[bad[:1]]}"
    assert np.array_equal(rgb, wrgb), what


# ---- integration ----
@pytest.mark.parametrize("name", sorted(CASES))
def test_integration_equals_the_checker_bit_for_bit(ctx, name):
    vol, frames = CASES[name]
    vol = vol.copy()
    v = make(ctx, vol)
    try:
        assert_state(v, vol, "initial state")
        for k, (depth, rgb, intr, m) in enumerate(frames):
            before = v.voxels()
            n = v.integrate(depth, intrinsics(intr), world_to_camera=m, color=rgb, count=True)
            r = T.integrate(vol, depth, intr, m, rgb)
            print(f"{name} frame {k}: {n} voxels updated")
            assert n == r["n_updated"]
            assert_state(v, vol, f"frame {k}")
            if "away" in name:
                assert n == 0 and all(np.array_equal(bits(a), bits(b)) if a.dtype == F else np.array_equal(a, b) for a, b in zip(before, v.voxels()))
    finally:
        v.close()


@pytest.mark.parametrize("name", ["32x32x32 three frames", "65x4x5 three frames max_weight 3", "257x5x3 identity"])
def test_torch_road_gives_the_numpy_roads_bits(ctx, name):
    import torch
    vol, frames = CASES[name]
    a, b = make(ctx, vol), make(ctx, vol)
    try:
        for depth, rgb, intr, m in frames:
            na = a.integrate(depth, intrinsics(intr), world_to_camera=m, color=rgb, count=True)
            d = torch.from_numpy(depth).cuda()
            c = None if rgb is None else torch.from_numpy(rgb).cuda()
            nb = b.integrate(d, intrinsics(intr), world_to_camera=m, color=c)            # enqueued only
            assert nb is None
            nb = None
        for x, y in zip(a.voxels(), b.voxels()):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        # the counted device call, and the two kinds do not mix
        b.reset()
        depth, rgb, intr, m = frames[0]
        assert b.integrate(torch.from_numpy(depth).cuda(), intrinsics(intr), world_to_camera=m, count=True) == T.integrate(vol.copy(), depth, intr, m)["n_updated"]
        with pytest.raises(Exception):
            b.integrate(torch.from_numpy(depth).cuda(), intrinsics(intr), world_to_camera=m, color=np.zeros((intr.height, intr.width, 3), np.uint8))
        with pytest.raises(Exception):
            b.integrate(depth, intrinsics(intr), world_to_camera=m, color=torch.zeros((intr.height, intr.width, 3), dtype=torch.uint8).cuda())
    finally:
        a.close(); b.close()


def test_camera_pose_is_inverted_by_the_facade(ctx):
    vol, frames = CASES["32x32x32 skew"]
    vol = vol.copy()
    depth, rgb, intr, m = frames[0]
    v = make(ctx, vol)
    try:
        v.integrate(depth, intrinsics(intr), camera_pose=T.POSES["skew"])
        T.integrate(vol, depth, intr, T.world_to_camera(T.POSES["skew"]))
        assert_state(v, vol)
    finally:
        v.close()


def test_reference_scene_and_its_call_shapes(ctx):
    """the reference's own scene through create_tsdf_volume / gpu_tsdf_integrate / gpu_tsdf_extract_surface: the measured figures"""
    intr = T.Intrinsics(*T.SCENE_CAMERA)
    v = tc.create_tsdf_volume(ctx=ctx, **T.SCENE)
    try:
        voxels = tc.gpu_tsdf_integrate(ctx, v, T.constant_depth(intr, 0.3), None, np.eye(4, dtype=F), tc.CameraIntrinsics(*T.SCENE_CAMERA))
        assert int((voxels[1] > 0).sum()) == 11146 and voxels[0].size == 32 ** 3
        xyz, rgb = tc.gpu_tsdf_extract_surface(ctx, v, None, 0.0)
        assert len(xyz) == 3231 and round(float(xyz[:, 2].astype(np.float64).mean()), 4) == 0.4125
        xyz, rgb = v.extract_surface(0.0, observed_only=True)
        assert len(xyz) == 925 and round(float(xyz[:, 2].astype(np.float64).mean()), 4) == 0.3
        xyz2, _ = tc.gpu_tsdf_extract_surface(ctx, v, voxels, 0.0)
        assert len(xyz2) == 3231
    finally:
        v.close()


# ---- extraction, on uploaded states ----
EXTRACTION_INPUTS = T.RESOLUTIONS + [T.MANY_BLOCKS]


def _check_extraction(ctx, res):
    vol = T.extraction_state(res)
    v = make(ctx, vol)
    try:
        v.load(vol.tsdf, vol.weight, vol.rgb)
        assert_state(v, vol, "download(upload(x))")
        for iso in (0.0, 0.03, -0.03):
            for observed in (False, True):
                want = T.extract(vol, iso, T.OBSERVED_EDGES if observed else 0)
                assert_points(v.extract_surface(iso, observed_only=observed), want, f"{res} iso {iso} observed_only {observed}")
        return len(T.extract(vol)[0])
    finally:
        v.close()


@pytest.mark.parametrize("res", EXTRACTION_INPUTS, ids=lambda r: "x".join(map(str, r)))
def test_extraction_equals_the_checker_bit_for_bit(ctx, res):
    n = _check_extraction(ctx, res)
    print(f"{res}: {n} points")
    assert (n == 0) == (min(res) < 2 or res == (2, 2, 2))


def test_extraction_with_the_two_level_scan(ctx, monkeypatch):
    """more than 2 049 cube blocks are two scan tiles; TC_SCAN_FUSED_MAX=1 (read per call) sends them through the two-level scan"""
    monkeypatch.setenv("TC_SCAN_FUSED_MAX", "1")
    assert _check_extraction(ctx, T.MANY_BLOCKS) > 0


def test_extraction_on_the_device_road(ctx):
    import torch
    vol = T.extraction_state((65, 4, 5))
    v = make(ctx, vol)
    try:
        v.load(torch.from_numpy(vol.tsdf).cuda(), torch.from_numpy(vol.weight).cuda(), torch.from_numpy(vol.rgb).cuda())
        assert_state(v, vol)
        xyz, rgb = v.extract_surface(0.0, device="cuda")
        assert_points((xyz.cpu().numpy(), rgb.cpu().numpy()), T.extract(vol))
        # the state as device arrays
        L, n = _lib.load(), vol.n
        t, w, c = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty((n, 3), dtype=torch.uint8, device="cuda")
        ctx._check(L.tc_tsdf_volume_download_device(v._h, t.data_ptr(), w.data_ptr(), c.data_ptr()))
        assert np.array_equal(bits(t.cpu().numpy()), bits(vol.tsdf)) and np.array_equal(w.cpu().numpy(), vol.weight) and np.array_equal(c.cpu().numpy(), vol.rgb)
        # rgb NULL means zeros
        v.load(vol.tsdf, vol.weight)
        assert not v.voxels()[2].any()
    finally:
        v.close()


def test_capacity_rule_and_the_empty_result(ctx):
    L = _lib.load()
    vol = T.extraction_state((65, 4, 5))
    want = T.extract(vol)
    n_want = len(want[0])
    v = make(ctx, vol)
    try:
        n = C.c_size_t(0)
        # an untouched volume: nothing, and TC_OK
        xyz, rgb = v.extract_surface()
        assert xyz.shape == (0, 3) and rgb.shape == (0, 3)
        v.load(vol.tsdf, vol.weight, vol.rgb)
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, None, None, 0, C.byref(n)) == _lib.TC_OK and n.value == n_want         # the count call
        xyz, rgb = np.full((n_want, 3), 7, F), np.full((n_want, 3), 7, np.uint8)
        n.value = 0
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, rgb.ctypes.data, n_want - 1, C.byref(n)) == _lib.TC_INVALID_DATA     # one short
        assert n.value == n_want and (xyz == 7).all() and (rgb == 7).all()
        assert "capacity" in L.tc_last_error_message(ctx._h).decode()
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, rgb.ctypes.data, n_want, C.byref(n)) == _lib.TC_OK                  # exact
        assert_points((xyz, rgb), want)
        xyz[:] = 7
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, None, n_want, C.byref(n)) == _lib.TC_OK                             # one array only
        assert np.array_equal(bits(xyz), bits(want[0]))
        # a generous capacity costs nothing: the host road stages exactly the result
        xyz[:] = 7
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, rgb.ctypes.data, 2 ** 64 - 1, C.byref(n)) == _lib.TC_OK and n.value == n_want
        assert_points((xyz, rgb), want)
    finally:
        v.close()


def test_validation_rows_with_their_messages(ctx):
    L = _lib.load()
    msg = lambda: L.tc_last_error_message(ctx._h).decode()
    # every row of tests/test_tsdf_cpu.py::VALIDATION_ROWS, told apart from a good config by its message (the good one: the handle below)
    from tests.test_tsdf_cpu import VALIDATION_ROWS
    words = {"voxel_size": "voxel_size must", "truncation": "truncation_distance must", "resolution": "resolution must", "origin": "origin must",
             "max_weight": "max_weight must", "far corner": "must be finite"}
    assert len(VALIDATION_ROWS) == 14
    for name, kw in VALIDATION_ROWS:
        args = dict(voxel_size=0.02, truncation_distance=0.1, resolution=(4, 4, 4))
        args.update({{"tau": "truncation_distance", "res": "resolution"}.get(k, k): v for k, v in kw.items()})
        (word,) = [w for key, w in words.items() if name.startswith(key)]
        with pytest.raises(tc.InvalidData, match=word):
            ctx.tsdf_volume(**args)
    with pytest.raises(tc.Unsupported, match="2\\^28"):
        ctx.tsdf_volume(0.02, 0.1, (1 << 14, 1 << 14, 2))
    v = ctx.tsdf_volume(0.02, 0.1, (4, 4, 4), max_weight=5)
    try:
        depth, m, n = np.ones((4, 4), F), (C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), C.c_size_t(0)
        good = dict(fx=4.0, fy=4.0, cx=1.5, cy=1.5, width=4, height=4)
        for kw, word in ((dict(fx=float("nan")), "intrinsics"), (dict(cy=float("inf")), "intrinsics"), (dict(width=0), "width"), (dict(height=0), "width")):
            k = _lib.CameraIntrinsicsC(**{**good, **kw})
            for fn in (L.tc_tsdf_integrate, L.tc_tsdf_integrate_device):
                assert fn(v._h, depth.ctypes.data, None, C.byref(k), m, C.byref(n)) == _lib.TC_INVALID_DATA and word in msg()
        k = _lib.CameraIntrinsicsC(**good)
        bad = (C.c_float * 12)(*([1.0] * 11 + [float("nan")]))
        assert L.tc_tsdf_integrate(v._h, depth.ctypes.data, None, C.byref(k), bad, None) == _lib.TC_INVALID_DATA and "world_to_camera" in msg()
        assert L.tc_tsdf_integrate(v._h, None, None, C.byref(k), m, None) == _lib.TC_INVALID_DATA and "NULL" in msg()
        assert L.tc_tsdf_integrate(v._h, depth.ctypes.data, None, None, m, None) == _lib.TC_INVALID_DATA
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 2, None, None, 0, C.byref(n)) == _lib.TC_INVALID_DATA and "flag" in msg()
        assert L.tc_tsdf_extract_surface(v._h, float("nan"), 0, None, None, 0, C.byref(n)) == _lib.TC_INVALID_DATA and "iso_value" in msg()
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, None, None, 0, None) == _lib.TC_INVALID_DATA
        # upload: a weight above max_weight is refused on the host road and the volume stays as it was
        w = np.full(64, 5, np.uint8)
        v.load(np.zeros(64, F), w)
        w[63] = 6
        with pytest.raises(tc.InvalidData, match="max_weight"):
            v.load(np.ones(64, F), w)
        assert not v.voxels()[0].any() and (v.voxels()[1] == 5).all()
        with pytest.raises(tc.InvalidData):
            v.load(np.zeros(63, F), w[:63])
        with pytest.raises(tc.InvalidData):
            v.integrate(np.ones((4, 5), F), tc.CameraIntrinsics(**good))
    finally:
        v.close()


def test_reset_restores_the_initial_bits_and_two_volumes_leave_each_other_alone(ctx):
    vol_a, frames = CASES["32x32x32 three frames"]
    vol_a, vol_b = vol_a.copy(), T.extraction_state((65, 4, 5))
    a, b = make(ctx, vol_a), make(ctx, vol_b)
    try:
        b.load(vol_b.tsdf, vol_b.weight, vol_b.rgb)
        for depth, rgb, intr, m in frames:
            a.integrate(depth, intrinsics(intr), world_to_camera=m, color=rgb)
            T.integrate(vol_a, depth, intr, m, rgb)
            assert_points(b.extract_surface(), T.extract(vol_b))
        assert_state(a, vol_a)
        assert_state(b, vol_b)
        assert_points(a.extract_surface(0.0, observed_only=True), T.extract(vol_a, 0.0, T.OBSERVED_EDGES))
        a.reset()
        vol_a.reset()
        assert_state(a, vol_a, "after reset")
        tsdf, weight, rgb = a.voxels()
        assert (bits(tsdf) == 0x3F800000).all() and not weight.any() and not rgb.any()
        assert_state(b, vol_b)
    finally:
        a.close(); b.close()


def _fusion(c):
    vol, frames = CASES["32x32x32 three frames"]
    v = make(c, vol)
    try:
        counts = [v.integrate(depth, intrinsics(intr), world_to_camera=m, color=rgb, count=True) for depth, rgb, intr, m in frames]
        return [np.asarray(counts)] + list(v.voxels()) + list(v.extract_surface()) + list(v.extract_surface(0.0, observed_only=True))
    finally:
        v.close()


def test_volume_after_the_other_users_of_the_pinned_block_gives_a_fresh_contexts_bits():
    """the pattern of tests/test_gpu_pinned_block.py: filter, registration, clustering, NDT, then fusion on ONE context; the same fusion
    alone on a fresh one.  The volume's two words are a region of their own (tc_internal.h: PinnedBlock::tsdf_out)."""
    from threecrate_amd import synth
    surface = synth.tum_shaped_cloud(width=100, height=80, seed=3)
    tgt = np.ascontiguousarray(surface[:2000])
    src = np.ascontiguousarray(synth.apply_isometry(synth.yaw_isometry((0.02, -0.015, 0.01), 0.03), surface[2000:4000]))
    c = tc.GpuContext(0)
    try:
        assert c.voxel_grid_filter(tgt, 0.1).shape[0] > 1
        assert c.icp_detailed(src, tgt, None, 20, None, 0.0).iterations == 20
        c.extract_euclidean_clusters_labels(tgt, 0.08, 5, 2000)
        c.ndt_registration(src, tgt, None, resolution=1.0, max_iterations=3, min_points_per_voxel=2)
        together = _fusion(c)
        c.segment_plane(tgt, 0.01, 64, seed=1)
        again = _fusion(c)
    finally:
        c.close()
    fresh = tc.GpuContext(0)
    try:
        alone = _fusion(fresh)
    finally:
        fresh.close()
    assert together[0].min() > 0 and len(together[4]) > 0
    for k, (x, y, z) in enumerate(zip(alone, together, again)):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)) and np.array_equal(x.view(np.uint8), z.view(np.uint8)), f"output {k}"


def test_profile_rows_and_launch_counts():
    L = _lib.load()
    vol, frames = CASES["65x4x5 three frames max_weight 3"]
    c = tc.GpuContext(0)
    try:
        v = make(c, vol)
        c.profile_enable(True)
        c.profile_reset()
        n = C.c_size_t(0)
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, None, None, 0, C.byref(n)) == _lib.TC_OK and n.value == 0
        xyz = np.zeros((16, 3), F)
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, None, 16, C.byref(n)) == _lib.TC_OK and n.value == 0
        p = c.profile_read()
        assert p["tsdf_count"][0] == 2 and "tsdf_fill" not in p and "tsdf_integrate" not in p          # an empty result: no fill launch
        for k, (depth, rgb, intr, m) in enumerate(frames):
            v.integrate(depth, intrinsics(intr), world_to_camera=m, color=rgb, count=(k == 1))
            assert c.profile_read()["tsdf_integrate"][0] == k + 1
        want = len(T.extract(_after(vol, frames))[0])
        xyz, rgb = np.zeros((want, 3), F), np.zeros((want, 3), np.uint8)
        assert L.tc_tsdf_extract_surface(v._h, 0.0, 0, xyz.ctypes.data, rgb.ctypes.data, want, C.byref(n)) == _lib.TC_OK and n.value == want > 0
        p = c.profile_read()
        assert (p["tsdf_integrate"][0], p["tsdf_count"][0], p["tsdf_fill"][0]) == (3, 3, 1)             # one extraction: one count, one fill
        v.extract_surface()                                                                            # the facade: the count call, then the points
        p = c.profile_read()
        assert (p["tsdf_count"][0], p["tsdf_fill"][0]) == (5, 2)
        v.close()
    finally:
        c.close()


def _after(vol, frames):
    vol = vol.copy()
    for depth, rgb, intr, m in frames:
        T.integrate(vol, depth, intr, m, rgb)
    return vol
