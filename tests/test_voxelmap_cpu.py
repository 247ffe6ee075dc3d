"""The streaming voxel map without a GPU: the checker (tests/voxelmap_checker.py) against the reference's own unit tests, every mutant
of the checker told apart by a named input (tests/voxelmap_cases.py), the preconditions of the GPU inputs, the null-handle calls through
the companion library, and the Python and Rust bindings' shapes."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import abi_text as T
from tests import voxelmap_cases as K
from tests.voxelmap_checker import (KEY_LIMIT, LONG_RUN, MIN_CAPACITY, OutOfRange, VoxelMapChecker, run, same_bits, same_state, slots_after)

F = np.float32


# ---- the reference's unit tests (streaming.rs:757-818, :900-921), restated as literals ----
def _grid_cloud(n):
    return np.stack([np.arange(n, dtype=F) * F(0.1), np.zeros(n, F), np.zeros(n, F)], axis=1)


def test_reference_reduces_density():
    for chunk in (32, 16):
        out = run(1.0, K.cut(_grid_cloud(100), chunk)).extract()[0]
        assert 0 < len(out) <= 10


def test_reference_centroid_and_chunk_boundary():
    out = run(1.0, K.cut(np.array([[0.1, 0, 0], [0.3, 0, 0]], F), 10)).extract()[0]
    assert len(out) == 1 and abs(out[0, 0] - 0.2) < 1e-5
    out = run(1.0, K.cut(np.array([[0.1, 0, 0], [0.9, 0, 0]], F), 1)).extract()[0]
    assert len(out) == 1 and abs(out[0, 0] - 0.5) < 1e-5


def test_reference_invalid_voxel_size_is_the_librarys_check():
    """process_chunk refuses voxel_size <= 0 (:251-253); here tc_voxel_map_create does, without a context too"""
    L = _lib.load_companion("threecrate_hip_voxelmap.h")
    for vs in (-1.0, 0.0, float("nan")):
        cfg, h = _lib.VoxelMapConfigC(vs, 0), C.c_void_p(7)
        assert L.tc_voxel_map_create(None, C.byref(cfg), C.byref(h)) == _lib.TC_INVALID_DATA and h.value is None


# ---- mutants ----
def _differs(voxel_size, chunks, **mutant):
    return not same_state(run(voxel_size, chunks).extract(), run(voxel_size, chunks, **mutant).extract())


@pytest.mark.parametrize("vs", [0.1, 0.3, 0.7])
def test_mutant_division_for_product(vs):
    pts = K.product_vs_division(vs)
    assert len(pts) >= 4
    real, mut = VoxelMapChecker(vs), VoxelMapChecker(vs, divide=True)
    assert (real.keys_of(pts)[0][:, 0] != mut.keys_of(pts)[0][:, 0]).all()
    assert _differs(vs, [pts], divide=True)


def test_mutant_truncation_for_floor():
    assert _differs(1.0, [K.negatives()], truncate=True)
    assert _differs(0.5, [K.faces()], truncate=True)


def test_mutant_nan_key():
    for nan_key in (-1, 1):
        assert _differs(1.0, [K.nan_points()], nan_key=nan_key)
    cent, keys, counts, sums = run(1.0, [K.nan_points()]).extract()
    assert np.isnan(sums).any() and (keys[np.isnan(sums)] == 0).all() and counts.sum() == len(K.nan_points())


def test_mutant_descending_fold_and_the_order_sensitive_input():
    pts = K.order_sensitive()
    assert len(pts) == 300 and len(run(1.0, [pts])) == 1
    asc, desc = run(1.0, [pts]).extract()[3], run(1.0, [pts], descending=True).extract()[3]
    assert (asc.view(np.uint64) != desc.view(np.uint64)).all()                  # every axis' sum differs in its bits
    assert _differs(1.0, [pts], descending=True)


def test_mutant_per_chunk_sums():
    pts = K.order_sensitive()
    assert _differs(1.0, K.cut(pts, 7), per_chunk=True)
    assert not _differs(1.0, [pts], per_chunk=True)                             # one chunk: the same fold


@pytest.mark.parametrize("count", [3, 7, 49])
def test_mutant_reciprocal_for_division(count):
    pts = K.reciprocal_case(count)
    assert len(pts) == count and len(run(1.0, [pts])) == 1
    real, mut = run(1.0, [pts]).extract(), run(1.0, [pts], reciprocal=True).extract()
    assert same_bits(real[3], mut[3]) and not same_bits(real[0], mut[0])


def test_mutant_unsigned_order():
    assert _differs(1.0, [K.negatives()], unsigned_order=True)
    keys = run(1.0, [K.stream()]).extract()[1]
    assert (keys < 0).any() and [tuple(k) for k in keys] == sorted(tuple(k) for k in keys.tolist())


def test_mutant_range_limits():
    ok = K.range_points()
    assert len(run(1.0, [ok])) == 9
    for mutant in (dict(limit_hi=KEY_LIMIT - 1), dict(limit_lo=-KEY_LIMIT + 1)):
        with pytest.raises(OutOfRange):
            run(1.0, [ok], **mutant)
    base = np.tile(F([[0.5, 0.5, 0.5]]), (9, 1))
    for bad in K.out_of_range_points():
        for axis in range(3):
            pts = base.copy()
            pts[4, axis] = bad
            c = run(1.0, [base])
            before = c.extract()
            with pytest.raises(OutOfRange):
                c.insert(pts)
            assert same_state(before, c.extract()) and c.points == 9
    for bad, mutant in ((F(KEY_LIMIT), dict(limit_hi=KEY_LIMIT + 1)), (F(-KEY_LIMIT - 1), dict(limit_lo=-KEY_LIMIT - 1))):
        pts = base.copy()
        pts[4, 0] = bad
        assert len(run(1.0, [pts], **mutant)) == 2


# ---- preconditions of the GPU inputs ----
def test_chunking_does_not_change_the_state():
    pts = K.stream()
    whole = run(1.0, [pts])
    assert 850 <= len(whole) <= 900 and (pts < 0).any()
    for chunks in (K.cut(pts, 7), K.cut(pts, 257), K.random_cut(pts)):
        assert same_state(whole.extract(), run(1.0, chunks).extract())


def test_line_clouds_and_long_runs_have_the_runs_they_claim():
    for r in (1, 255, 256, 257, 2049):
        for m in (1, 9):
            c = run(1.0, [K.line_cloud(r, m)])
            assert len(c) == r and (c.extract()[2] == m).all()
    c = run(1.0, [K.long_runs(K.LONG_LENGTHS, short=40)])
    assert sorted(c.extract()[2].tolist()) == [3] * 40 + [LONG_RUN - 1, LONG_RUN, LONG_RUN + 1]
    assert K.WAVE_LENGTHS == (192, 193, 256, 257) and min(K.WAVE_LENGTHS) > LONG_RUN
    for w in K.WAVE_LENGTHS:
        assert run(1.0, [K.long_runs((w,))]).extract()[2].tolist() == [w]
    c = run(1.0, [K.long_runs(K.LONG_LENGTHS + K.WAVE_LENGTHS, short=300)])
    assert sorted(c.extract()[2].tolist()) == [3] * 300 + [LONG_RUN - 1, LONG_RUN, LONG_RUN + 1, 192, 193, 256, 257]


def test_growth_steps_cross_each_doubling_where_they_claim():
    c, slots, seen = VoxelMapChecker(1.0), MIN_CAPACITY, []
    for pts, r, want in K.growth_steps():
        v = len(c)
        c.insert(pts)
        assert len(c) == v + r                                  # every voxel of the chunk is new
        slots = slots_after(slots, v, r)
        assert slots == want
        seen.append((2 * (v + r), slots))
    assert seen[:6] == [(254, 256), (256, 256), (258, 512), (510, 512), (512, 512), (514, 1024)] and seen[6][1] == 8 * 1024


# ---- null handles and contexts through the companion: a status, nothing written, no crash ----
def test_null_handle_and_null_context_calls():
    L = _lib.load_companion("threecrate_hip_voxelmap.h")
    xyz = np.full((4, 3), 7.0, F)
    out = np.full(12, 7, np.int32)
    n = C.c_size_t(7)
    h = C.c_void_p(7)
    cfg = _lib.VoxelMapConfigC(1.0, 0)
    assert L.tc_voxel_map_create(None, C.byref(cfg), C.byref(h)) == _lib.TC_INVALID_DATA and h.value is None
    assert L.tc_voxel_map_create(None, None, C.byref(h)) == _lib.TC_INVALID_DATA
    assert L.tc_voxel_map_create(None, C.byref(cfg), None) == _lib.TC_INVALID_DATA
    big = _lib.VoxelMapConfigC(1.0, (1 << 28) + 1)
    assert L.tc_voxel_map_create(None, C.byref(big), C.byref(h)) == _lib.TC_UNSUPPORTED
    assert L.tc_voxel_map_destroy(None) is None
    assert L.tc_voxel_map_reset(None) == _lib.TC_INVALID_DATA
    assert L.tc_voxel_map_size(None) == 0 and L.tc_voxel_map_points(None) == 0
    for fn in (L.tc_voxel_map_insert, L.tc_voxel_map_insert_device):
        assert fn(None, xyz.ctypes.data, 4) == _lib.TC_INVALID_DATA and fn(None, xyz.ctypes.data, 0) == _lib.TC_INVALID_DATA
    for fn in (L.tc_voxel_map_extract, L.tc_voxel_map_extract_device):
        assert fn(None, out.ctypes.data, None, None, None, 4, C.byref(n)) == _lib.TC_INVALID_DATA
    assert n.value == 7 and (out == 7).all() and (xyz == 7.0).all()


# ---- bindings ----
def test_compat_class_has_the_wheels_signature_and_messages():
    import threecrate_amd.compat as threecrate
    assert "RealtimeVoxelFilter" in threecrate.__all__
    sig = inspect.signature(threecrate.RealtimeVoxelFilter)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [("voxel_size", inspect.Parameter.empty), ("max_queue_depth", 1024),
                                                                      ("chunk_size", 256), ("flush_timeout_ms", 10)]
    for args, msg in (((0.0,), "voxel_size must be positive"), ((-1.0,), "voxel_size must be positive"), ((1.0, 1024, 0), "chunk_size must be ≥ 1"),
                      ((1.0, 0), "max_queue_depth must be ≥ 1"), ((0.0, 0, 0), "voxel_size must be positive"), ((1.0, 0, 0), "chunk_size must be ≥ 1")):
        with pytest.raises(ValueError) as e:
            threecrate.RealtimeVoxelFilter(*args)
        assert str(e.value) == msg
    rt = threecrate.RealtimeVoxelFilter(0.5, flush_timeout_ms=None)
    m = rt.metrics()
    assert (m.items_queued, m.items_processed, m.items_dropped, m.estimated_queue_depth) == (0, 0, 0, 0)
    for bad in (np.zeros(2, F), np.zeros((1, 3), F), [0.0, 0.0, 0.0], np.zeros(3, np.int32)):
        with pytest.raises(ValueError):
            rt.send(bad)
    with pytest.raises(ValueError):
        rt.send_batch(np.zeros((2, 2), F))
    cloud = rt.finish()                                         # an empty stream: no device is touched
    assert isinstance(cloud, threecrate.PointCloud) and len(cloud) == 0
    for call in (lambda: rt.send(np.zeros(3, F)), lambda: rt.send_batch(np.zeros((1, 3), F)), lambda: rt.try_send(np.zeros(3, F)), rt.metrics, rt.finish):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == "pipeline already finished"
    assert "nothing is dropped" in threecrate.RealtimeVoxelFilter.try_send.__doc__


def test_python_api_has_the_methods():
    import threecrate_amd as tc
    from threecrate_amd import api
    assert list(inspect.signature(api.GpuContext.voxel_map).parameters) == ["self", "voxel_size", "initial_capacity"]
    for name in ("insert", "__len__", "points_inserted", "reset", "extract", "close"):
        assert hasattr(api.VoxelMap, name), name
    assert list(inspect.signature(api.VoxelMap.extract).parameters)[:4] == ["self", "keys", "counts", "sums"]
    assert tc is not None


def test_rust_facade_has_the_references_names():
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    assert re.search(r"^pub mod ffi_voxelmap;", lib_rs, re.M)
    assert re.search(r"pub struct StreamingVoxelFilterConfig\s*\{\s*pub voxel_size: f32,?\s*\}", lib_rs)
    assert re.search(r"pub struct StreamingVoxelFilter\b", lib_rs)
    body = lib_rs[re.search(r"^impl(<'a>)? StreamingVoxelFilter", lib_rs, re.M).start():]
    for fn in ("pub fn new(", "pub fn voxel_count(", "pub fn process_chunk(", "pub fn finalize("):
        assert fn in body, fn
    assert "voxel_size must be positive" in body and "InvalidData" in body
