"""The host twins of the registration entry points (csrc/registration.hip) and of the other surfaces that stage a caller's arrays.

1. A failed tc_kiss_icp / tc_gicp / tc_multiscale_icp_point_to_point leaves the caller's correspondence array alone and puts the
   caller's pointer back into the result; a successful one writes what the _device twin writes (KISS-ICP: n_source_down words).
   tc_icp_detailed / tc_icp_point_to_plane_detailed: a failed call leaves the context as a fresh one.
2. Every host twin validates before it stages: with its first-checked invalid argument and a NULL cloud it returns what its
   _device twin returns, status and message, and never touches the pointer.

300-point clouds; every call is a raw entry point."""
import ctypes as C
import functools

import numpy as np
import pytest

import threecrate_amd as tc
from threecrate_amd import _lib, synth

pytestmark = pytest.mark.gpu
F = np.float32
N = 300
MARK = 0xDEADBEEF
INVALID, ALGORITHM, UNSUPPORTED = 1, 2, 4
IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], F)
I7 = IDENTITY.ctypes.data


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    return _lib.load()


@functools.lru_cache(None)
def pair(far=False):
    """an ordinary pair, or the same with the source 100 units away from the target"""
    src, tgt, _ = synth.registration_pair(N, seed=2)
    if far:
        src = np.ascontiguousarray(src + np.array([100, 0, 0], F))
    return src, tgt


@functools.lru_cache(None)
def normals_of_target():
    c = tc.GpuContext(0)
    nrm = np.ascontiguousarray(c.estimate_normals(pair()[1], 8)[:, 3:], F)
    c.close()
    return nrm


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
    torch.cuda.synchronize()
    return t


def _msg(L, ctx):
    return L.tc_last_error_message(ctx._h).decode()


def _result(corr_ptr=None):
    r = _lib.IcpResultC()
    r.corr_target = corr_ptr
    return r


def _fields(r):
    return (np.array(r.transformation, F).view(np.uint32).tolist(), np.array([r.mse], F).view(np.uint32)[0], r.iterations, r.converged,
            r.n_correspondences)


# ---- the three variants whose host twin lends the _device road a device array ------------------------------------------------
# name -> call(L, h, source pointer, target pointer, max distance, result) -> (status, words written on success)
def _kiss(L, h, s, t, dist, r, device=False):
    # identity start: sigma = 3 voxel_size (kiss_icp.rs:82-95), far below 100; `dist` has no say
    cfg, nd = _lib.KissIcpConfigC(0.1, 1.0e6, 0.0, 5), C.c_size_t(0)
    rc = (L.tc_kiss_icp_device if device else L.tc_kiss_icp)(h, s, N, t, N, I7, C.byref(cfg), C.byref(r), C.byref(nd))
    return rc, nd.value


def _gicp(L, h, s, t, dist, r, device=False):
    cfg = _lib.GicpConfigC(5, dist, 1e-6, 20)
    return (L.tc_gicp_device if device else L.tc_gicp)(h, s, N, t, N, I7, C.byref(cfg), C.byref(r)), N


def _multiscale(level_dist):
    def call(L, h, s, t, dist, r, device=False):
        assert not device
        lv = (_lib.ScaleLevelC * 1)()
        lv[0].voxel_size, lv[0].max_iterations, lv[0].max_correspondence_distance = 0.05, 1, dist if level_dist else -1.0
        cfg = _lib.MultiScaleConfigC(lv, 1, 5, dist, 1e-6)
        return L.tc_multiscale_icp_point_to_point(h, s, N, t, N, I7, C.byref(cfg), C.byref(r)), N
    return call


# multiscale fails in its level (before the device array exists) or, the level without a cut-off, in the final refinement (with it)
LENDERS = {"kiss": _kiss, "gicp": _gicp, "multiscale_level": _multiscale(True), "multiscale_final": _multiscale(False)}
FAILURE = {"kiss": "Insufficient correspondences found", "multiscale_level": "Insufficient correspondences found",
           "multiscale_final": "Insufficient correspondences found",
           "gicp": "GICP: insufficient correspondences (need >= 6) or ill-conditioned Gauss-Newton system"}


@pytest.mark.parametrize("name", list(LENDERS))
def test_failed_call_leaves_the_callers_correspondences_alone(ctx, L, name):
    src, tgt = pair(far=True)
    corr = np.full(N, MARK, np.uint32)
    r = _result(corr.ctypes.data)
    rc, _ = LENDERS[name](L, ctx._h, src.ctypes.data, tgt.ctypes.data, 1e-3, r)
    assert rc == ALGORITHM and _msg(L, ctx) == FAILURE[name]
    assert r.corr_target == corr.ctypes.data
    assert np.all(corr == MARK)


@pytest.mark.parametrize("name", ["kiss", "gicp"])
def test_successful_call_writes_what_the_device_twin_writes(ctx, L, name):
    src, tgt = pair()
    corr = np.full(N, MARK, np.uint32)
    r = _result(corr.ctypes.data)
    rc, count = LENDERS[name](L, ctx._h, src.ctypes.data, tgt.ctypes.data, 1.0, r)
    assert rc == 0, _msg(L, ctx)
    assert r.corr_target == corr.ctypes.data
    d_src, d_tgt, d_corr = _dev(src), _dev(tgt), _dev(np.full(N, MARK, np.uint32))
    rd = _result(d_corr.data_ptr())
    rcd, count_d = LENDERS[name](L, ctx._h, d_src.data_ptr(), d_tgt.data_ptr(), 1.0, rd, device=True)
    assert rcd == 0 and count_d == count and _fields(rd) == _fields(r)
    twin = d_corr.cpu().numpy().view(np.uint32)
    assert 0 < count <= N and (name != "kiss" or count < N)         # (KISS-ICP: the voxel filter merged some points)
    assert np.array_equal(corr[:count], twin[:count]) and np.all(corr[:count] != MARK)
    assert np.all(corr[count:] == MARK)


def test_successful_multiscale_call_writes_every_word(ctx, L):
    """no _device twin: every source has its word (a target index, or 0xFFFFFFFF = none), as many pairs as the result counts"""
    src, tgt = pair()
    corr = np.full(N, MARK, np.uint32)
    r = _result(corr.ctypes.data)
    rc, _ = LENDERS["multiscale_level"](L, ctx._h, src.ctypes.data, tgt.ctypes.data, 1.0, r)
    assert rc == 0, _msg(L, ctx)
    assert r.corr_target == corr.ctypes.data
    paired = corr != 0xFFFFFFFF
    assert np.all(corr[paired] < N) and int(paired.sum()) == r.n_correspondences > 0


# ---- the two twins of the overlapped upload: a failure leaves nothing behind on the context ----------------------------------
def _detailed(L, h, src, tgt, dist, r):
    return L.tc_icp_detailed(h, src.ctypes.data, N, tgt.ctypes.data, N, I7, 10, dist, 1e-6, C.byref(r))


def _p2plane(L, h, src, tgt, dist, r):
    nrm = normals_of_target()
    return L.tc_icp_point_to_plane_detailed(h, src.ctypes.data, N, tgt.ctypes.data, N, nrm.ctypes.data, N, 3, I7, 10, dist, 1e-6, C.byref(r))


@pytest.mark.parametrize("call,message", [(_detailed, "Insufficient correspondences found"),
                                          (_p2plane, "Insufficient correspondences for point-to-plane ICP (need >= 6) or ill-conditioned system")],
                         ids=["icp_detailed", "icp_point_to_plane_detailed"])
def test_call_after_a_failed_one_gives_a_fresh_contexts_bits(ctx, L, call, message):
    far_src, tgt = pair(far=True)
    scratch = np.full(N, MARK, np.uint32)
    rc = call(L, ctx._h, far_src, tgt, 1e-3, _result(scratch.ctypes.data))
    assert rc == ALGORITHM and _msg(L, ctx) == message
    src, _ = pair()
    got, want = [], []
    fresh = tc.GpuContext(0)
    for c, out in ((ctx, got), (fresh, want)):
        corr = np.full(N, MARK, np.uint32)
        r = _result(corr.ctypes.data)
        assert call(L, c._h, src, tgt, 1.0, r) == 0, _msg(L, c)
        out.extend([_fields(r), corr.tolist()])
    fresh.close()
    assert got == want


# ---- validation precedes staging ------------------------------------------------------------------------------------------------
def _icp(n_source=N, max_iters=10):
    return lambda L, h, fn: fn(h, None, n_source, None, N, I7, max_iters, 1.0, 1e-6, C.byref(_result()))


def _plane(n_source=N, n_normals=N, stride=3, max_iters=10):
    return lambda L, h, fn: fn(h, None, n_source, None, N, None, n_normals, stride, I7, max_iters, 1.0, 1e-6, C.byref(_result()))


def _kiss_cfg(n_source=N, voxel=0.1, iters=5):
    return lambda L, h, fn: fn(h, None, n_source, None, N, I7, C.byref(_lib.KissIcpConfigC(voxel, 1.0e6, 0.0, iters)), C.byref(_result()),
                               C.byref(C.c_size_t(0)))


def _gicp_cfg(n_source=N, iters=5, k=20):
    return lambda L, h, fn: fn(h, None, n_source, None, N, I7, C.byref(_lib.GicpConfigC(iters, 1.0, 1e-6, k)), C.byref(_result()))


def _index_query(L, h, fn):
    index = C.c_void_p()
    assert L.tc_search_index_create(h, pair()[1].ctypes.data, N, 8, C.byref(index)) == 0
    try:
        return fn(index, None, N, 4096, -1.0, None, None, None)
    finally:
        L.tc_search_index_destroy(index)


EMPTY = "Source or target point cloud is empty"
# (host export, what to call it with, status, message): the first checks of the present source, in its order
VALIDATION = [
    ("tc_icp_detailed", _icp(n_source=0), INVALID, EMPTY),
    ("tc_icp_detailed", _icp(max_iters=0), INVALID, "Max iterations must be positive"),
    ("tc_icp_point_to_plane_detailed", _plane(n_source=0), INVALID, EMPTY),
    ("tc_icp_point_to_plane_detailed", _plane(n_normals=N - 1), INVALID, "target_normals length must equal the number of target points"),
    ("tc_icp_point_to_plane_detailed", _plane(max_iters=0), INVALID, "Max iterations must be positive"),
    ("tc_icp_point_to_plane_detailed", _plane(stride=2), INVALID, "normal_stride must be >= 3"),
    ("tc_kiss_icp", _kiss_cfg(n_source=0), INVALID, "KISS-ICP: source or target point cloud is empty"),
    ("tc_kiss_icp", _kiss_cfg(iters=0), INVALID, "KISS-ICP: max_iterations must be > 0"),
    ("tc_kiss_icp", _kiss_cfg(voxel=0.0), INVALID, "KISS-ICP: voxel_size must be > 0"),
    ("tc_gicp", _gicp_cfg(n_source=0), INVALID, "GICP: source or target point cloud is empty"),
    ("tc_gicp", _gicp_cfg(iters=0), INVALID, "GICP: max_iterations must be > 0"),
    ("tc_gicp", _gicp_cfg(k=N + 1), INVALID, "GICP: clouds must have at least k_correspondences points"),
    ("tc_knn", lambda L, h, fn: fn(h, None, N, None, N, 2049, None, None, None), UNSUPPORTED, "k > 2048 is not supported by the HIP k-NN export"),
    ("tc_radius_search", lambda L, h, fn: fn(h, None, N, None, N, 1.0, 2049, None, None, None), UNSUPPORTED,
     "k_max > 2048 is not supported by the HIP radius search"),
    ("tc_search_index_query", _index_query, UNSUPPORTED, "k > 2048 is not supported by the HIP neighbour search"),
    ("tc_voxel_grid_filter", lambda L, h, fn: fn(h, None, N, 0.0, None, C.byref(C.c_size_t(7))), INVALID, "voxel_size must be positive"),
    ("tc_extract_euclidean_clusters", lambda L, h, fn: fn(h, None, N, 0.1, 0, 10, None, None, None, C.byref(C.c_size_t(7))), INVALID,
     "min_cluster_size must be at least 1"),
    ("tc_extract_fpfh_features", lambda L, h, fn: fn(h, None, N, 0.0, 8, None), INVALID, "search_radius must be positive"),
    ("tc_extract_fpfh_features_with_normals", lambda L, h, fn: fn(h, None, N, 0.0, 8, None), INVALID, "search_radius must be positive"),
]


@pytest.mark.parametrize("export,call,status,message", VALIDATION, ids=[f"{v[0]}-{i}" for i, v in enumerate(VALIDATION)])
def test_validation_precedes_staging(ctx, L, export, call, status, message):
    for name in (export, export + "_device"):
        # the context keeps its last message: put another one there first
        cfg = _lib.NormalConfig(k_neighbors=2)
        assert L.tc_estimate_normals(ctx._h, None, N, C.byref(cfg), None) == INVALID and _msg(L, ctx) == "k_neighbors must be at least 3"
        rc = call(L, ctx._h, getattr(L, name))
        assert (rc, _msg(L, ctx)) == (status, message), name


@pytest.mark.parametrize("export", ["tc_voxel_grid_filter", "tc_voxel_grid_filter_device"])
def test_empty_cloud_is_an_empty_result_before_any_pointer_is_read(ctx, L, export):
    n_out = C.c_size_t(7)
    assert getattr(L, export)(ctx._h, None, 0, 0.0, None, C.byref(n_out)) == 0 and n_out.value == 0         # (n == 0 precedes the voxel check)
