"""tc_colorize on the device against tests/color_checker.py: every case of tests/color_cases.py on both roads (numpy in: the host entry
point; torch device tensors in: the _device one).  Colours, source indices and counts are EQUAL to the checker's: no tolerance, nothing
left out of a comparison."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, api
from tests import color_cases as CC
from tests import color_checker as K

pytestmark = pytest.mark.gpu
F = np.float32
MODES = {0: "nearest", 1: "bilinear"}


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """the checker's answer to every case, computed once and shared"""
    return {name: K.colorize(case["xyz"], case["sources"], **case["cfg"]) for name, case in CC.CASES.items()}


def _to(a, road):
    return a if road == "numpy" or a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _sources(case, road):
    return [tuple(_to(x, road) if i in (0, 3) else x for i, x in enumerate(src)) for src in case["sources"]]


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def run(ctx, case, road, **kw):
    c = case["cfg"]
    out = ctx.colorize(_to(case["xyz"], road), _sources(case, road), default_color=c["default_color"], interpolation=MODES[c["interpolation"]],
                       min_depth=c["min_depth"], depth_tolerance=c["depth_tolerance"], **kw)
    return tuple(_host(a) for a in out) if isinstance(out, tuple) else _host(out)


@pytest.mark.parametrize("road", ["numpy", "torch"])
@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_every_case_equals_the_checker(ctx, expected, name, road):
    rgb, index, count = run(ctx, CC.CASES[name], road, return_index=True)
    want_rgb, want_index, want_count = expected[name]
    assert rgb.dtype == np.uint8 and index.dtype == np.int32 and rgb.shape == want_rgb.shape
    assert np.array_equal(index, want_index), np.nonzero(index != want_index)[0][:10]
    assert np.array_equal(rgb, want_rgb), np.nonzero((rgb != want_rgb).any(axis=1))[0][:10]
    assert count == want_count


@pytest.mark.parametrize("road", ["numpy", "torch"])
@pytest.mark.parametrize("n", CC.BLOCK_SIZES)
def test_every_subset_of_the_outputs(ctx, expected, n, road):
    case = CC.CASES[f"blocks_{n}"]
    want = dict(zip(("return_color", "return_index", "count"), expected[f"blocks_{n}"]))
    for subset in itertools.product((False, True), repeat=3):
        kw = dict(zip(("return_color", "return_index", "count"), subset))
        if not any(subset):
            with pytest.raises(tc.InvalidData, match="all NULL"):
                run(ctx, case, road, **kw)
            continue
        got = run(ctx, case, road, **kw)
        got = got if isinstance(got, tuple) else (got,)
        for key, value in zip([k for k in kw if kw[k]], got):
            assert np.array_equal(value, want[key]) if key != "count" else value == want[key], (kw, key)
    if road == "torch":
        torch.cuda.synchronize()


def test_two_calls_give_equal_bits_and_two_contexts_agree(ctx, expected):
    other = tc.GpuContext(0)
    try:
        for name in ("edges_7x5_bilinear", "sources_max", f"blocks_{CC.SLICES * 256 + 1}"):
            for road in ("numpy", "torch"):
                a, b = run(ctx, CC.CASES[name], road, return_index=True), run(ctx, CC.CASES[name], road, return_index=True)
                c = run(other, CC.CASES[name], road, return_index=True)
                for x, y, z, w in zip(a, b, c, expected[name]):
                    assert np.array_equal(x, y) and np.array_equal(x, z) and np.array_equal(x, w)
    finally:
        other.close()


def test_a_call_after_the_other_users_of_the_pinned_block_equals_a_fresh_context(ctx, expected):
    """voxel filter (the count word), plane segmentation (the union), a voxel map (the region in front of colorization's)"""
    pts = np.random.default_rng(3).random((3000, 3), dtype=F)
    ctx.voxel_grid_filter(pts, 0.1)
    ctx.segment_plane(pts, 0.05, 64, seed=1)
    m = ctx.voxel_map(0.1)
    m.insert(pts)
    assert len(m) > 0
    m.close()
    name = f"blocks_{CC.SLICES * 256 + 1}"
    fresh = tc.GpuContext(0)
    try:
        for road in ("numpy", "torch"):
            a, b = run(ctx, CC.CASES[name], road, return_index=True), run(fresh, CC.CASES[name], road, return_index=True)
            for x, y, w in zip(a, b, expected[name]):
                assert np.array_equal(x, y) and np.array_equal(x, w)
    finally:
        fresh.close()
    assert ctx.voxel_grid_filter(pts, 0.1).shape[1] == 3        # and the others still work after it


def test_launch_rows(ctx):
    """every call launches exactly one of the two instantiations: row `colorize` without a count, row `colorize_counted` with one"""
    case = CC.CASES["blocks_513"]
    rows = lambda: {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("colorize")}
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        for road in ("numpy", "torch"):
            run(ctx, case, road, count=False)
            run(ctx, case, road, count=False, return_index=True)
        assert rows() in ({"colorize": 4}, {"colorize": 4, "colorize_counted": 0})
        for road in ("numpy", "torch"):
            run(ctx, case, road, count=True)
        assert rows() == {"colorize": 4, "colorize_counted": 2}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


def test_the_checks_come_in_the_headers_order(ctx):
    L = _lib.load_companion("threecrate_hip_color.h")
    img = np.zeros((1, 1, 3), np.uint8)
    xyz, rgb, count = np.zeros((1, 3), F), np.full((1, 3), 7, np.uint8), C.c_size_t(7)

    def source(rgb_ptr=img.ctypes.data, fx=1.0, m0=1.0, w=1, h=1):
        m = CC.IDENTITY.copy()
        m[0] = m0
        return _lib.ColorSourceC(rgb_ptr, None, _lib.CameraIntrinsicsC(fx, 1, 0, 0, w, h), (C.c_float * 12)(*m))

    def config(mode=1, min_depth=1e-4, tol=0.05):
        return _lib.ColorizeConfigC((C.c_uint8 * 3)(128, 128, 128), mode, min_depth, tol)

    def call(sources, cfg, n=1, xyz_ptr=xyz.ctypes.data, n_sources=None, out=True, fn=L.tc_colorize):
        table = (_lib.ColorSourceC * max(1, len(sources)))(*sources)
        return fn(ctx._h, xyz_ptr, n, table, len(sources) if n_sources is None else n_sources, None if cfg is None else C.byref(cfg),
                  rgb.ctypes.data if out else None, None, C.byref(count) if out else None)

    I, U = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED
    message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
    ok, bad_cfg = source(), config(mode=2, min_depth=float("nan"))
    for fn in (L.tc_colorize, L.tc_colorize_device):
        # 1 before everything: 65 sources, one without an image, and a bad configuration
        assert call([ok] * 64 + [source(rgb_ptr=None)], bad_cfg, fn=fn) == I and "source 64: rgb is NULL" in message()
        assert call([ok] * 65, bad_cfg, xyz_ptr=None, fn=fn) == I
        assert call([ok] * 65, None, fn=fn) == I
        assert call([ok], config(), out=False, fn=fn) == I
        # 2 before 4: no sources and a bad configuration -> the reference's message
        assert call([], bad_cfg, n_sources=0, fn=fn) == I and "sources slice must not be empty" in message()
        # 3 before 4, 5 and 6
        assert call([source(fx=float("inf"))] * 65, bad_cfg, fn=fn) == U
        # 4 before 5 and 6
        assert call([source(w=0)], config(mode=2, tol=-1.0), fn=fn) == I
        # 5 before 6: a bad tolerance and a source that would be TC_UNSUPPORTED
        for cfg in (config(min_depth=float("inf")), config(tol=float("nan")), config(tol=-1.0)):
            assert call([source(w=65537)], cfg, fn=fn) == I
        # 6 in index order: the first bad source answers
        assert call([ok, source(w=65537), source(m0=float("nan"))], config(), fn=fn) == U
        assert call([ok, source(m0=float("nan")), source(w=65537)], config(), fn=fn) == I
        assert call([source(h=0)], config(), fn=fn) == I and call([source(fx=float("nan"))], config(), fn=fn) == I
        assert call([source(w=65536, h=1)], config(), n=0, fn=fn) == _lib.TC_OK        # the limit itself passes; n == 0 touches no image
        # 6 before 7
        assert call([source(w=65537)], config(), n=2 ** 32 - 16, fn=fn) == U
        assert call([ok], config(), n=2 ** 32 - 16, fn=fn) == U
    assert rgb.tolist() == [[7, 7, 7]] and count.value == 0                            # written by the n == 0 call alone
    with pytest.raises(tc.InvalidData, match="sources slice must not be empty"):
        ctx.colorize(xyz, [])
    with pytest.raises(tc.Unsupported, match="64"):
        ctx.colorize(xyz, [(img, (1, 1, 0, 0), CC.IDENTITY)] * 65)
    with pytest.raises(tc.InvalidData, match="source 1: an intrinsic or matrix entry is not finite"):
        ctx.colorize(xyz, [(img, (1, 1, 0, 0), CC.IDENTITY), (img, (np.nan, 1, 0, 0), CC.IDENTITY)])
    # n == 0: TC_OK with a count of 0 on both roads
    assert ctx.colorize(np.zeros((0, 3), F), [(img, (1, 1, 0, 0), CC.IDENTITY)])[1] == 0
    empty = ctx.colorize(torch.zeros((0, 3), device="cuda:0"), [(torch.zeros((1, 1, 3), dtype=torch.uint8, device="cuda:0"), (1, 1, 0, 0), CC.IDENTITY)])
    assert empty[1] == 0 and tuple(empty[0].shape) == (0, 3)


def test_compat_colorize_point_cloud_equals_the_context_call(ctx):
    case = CC.CASES["edges_7x5_bilinear"]
    img, k, _ = case["sources"][0]
    pose = np.eye(4)
    pose[:3, 3] = (0.25, -0.5, 0.0)
    cloud = threecrate.PointCloud(case["xyz"])
    got = threecrate.colorize_point_cloud(cloud, img.tobytes(), 7, 5, *k, pose)
    want = api.default_context().colorize(case["xyz"], [(img, k, pose.astype(F))], count=False)
    checker = K.colorize(case["xyz"], [(img, k, pose.astype(F)[:3].reshape(12))])[0]
    assert isinstance(got, threecrate.ColoredPointCloud) and len(got) == len(case["xyz"]) and repr(got) == f"ColoredPointCloud({len(got)} points)"
    assert np.array_equal(got.colors(), want) and np.array_equal(want, checker) and np.array_equal(got.positions(), case["xyz"])
    assert 0 < (got.colors() != 128).any(axis=1).sum() < len(got)
    # the reference's unit tests through the wheel's function
    red = np.tile(np.uint8([255, 0, 0]), 16).tobytes()
    one = threecrate.colorize_point_cloud(threecrate.PointCloud(np.array([[0, 0, 1], [0, 0, -1], [1000, 0, 1]], F)), red, 4, 4, 2.0, 2.0, 1.5, 1.5, np.eye(4))
    assert one.colors().tolist() == [[255, 0, 0], [128, 128, 128], [128, 128, 128]]
