"""The streaming voxel map on the device against the checker (tests/voxelmap_checker.py), bit for bit: keys and counts exact, sums and
centroids by their bits (a NaN equals a NaN), through the host road (numpy) and the device road (torch tensors).  The inputs are the
named ones of tests/voxelmap_cases.py, whose claims tests/test_voxelmap_cpu.py proves on the checker."""
import ctypes as C

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import _lib, api
from tests import voxelmap_cases as K
from tests.voxelmap_checker import KEY_LIMIT, LONG_RUN, MIN_CAPACITY, VoxelMapChecker, run, same_bits, same_state

pytestmark = pytest.mark.gpu
F = np.float32
ROADS = ["numpy", "torch"]


def _arg(pts, road):
    return pts if road == "numpy" else torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")


def _state(m):
    cent, keys, counts, sums = m.extract(keys=True, counts=True, sums=True)
    return cent, keys, counts, sums


def _check(m, ref, what=""):
    got, want = _state(m), ref.extract()
    assert len(m) == len(ref) and m.points_inserted == ref.points, what
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), what            # keys, counts
    assert same_bits(got[3], want[3]), what                                                         # sums
    assert same_bits(got[0], want[0]), what                                                         # centroids
    return got


def _both(ctx, voxel_size, chunks, road, capacity=0):
    m, ref = ctx.voxel_map(voxel_size, capacity), VoxelMapChecker(voxel_size)
    for ch in chunks:
        m.insert(_arg(ch, road))
        ref.insert(ch)
    return m, ref


# ---- block edges ----
@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("m_per", [1, 9])
@pytest.mark.parametrize("runs", [1, 255, 256, 257, 2049])
def test_block_edges(ctx, runs, m_per, road):
    m, ref = _both(ctx, 1.0, [K.line_cloud(runs, m_per)], road, MIN_CAPACITY)
    _check(m, ref)
    m.close()


# ---- long runs ----
def _rows(ctx):
    """launches of the map's kernels since the last reset (a reset keeps the rows it has seen, at zero)"""
    return {k: v[0] for k, v in ctx.profile_read().items() if k.startswith("voxel_map") and v[0]}


@pytest.mark.parametrize("road", ROADS)
def test_long_runs_alone_mixed_and_into_an_existing_voxel(ctx, road):
    ctx.profile_enable(True)
    try:
        # (the last: five long runs in one chunk, a wave each)
        for lengths, long_expected in (((LONG_RUN - 1,), 0), ((LONG_RUN,), 0), ((LONG_RUN + 1,), 1), (K.LONG_LENGTHS, 1)) + \
                tuple(((w,), 1) for w in K.WAVE_LENGTHS) + ((K.LONG_LENGTHS + K.WAVE_LENGTHS, 1),):
            for short in (0, 300):
                ctx.profile_reset()
                pts = K.long_runs(lengths, short=short)
                m, ref = _both(ctx, 1.0, [pts], road)
                _check(m, ref, (lengths, short))
                rows = _rows(ctx)
                assert rows.get("voxel_map_insert") == 1 and rows.get("voxel_map_insert_long", 0) == long_expected, (lengths, short, rows)
                assert "voxel_map_rehash" not in rows
                # the same voxels again: every run starts from the sums its slot holds
                again = K.long_runs(lengths, short=short, seed=1)
                m.insert(_arg(again, road))
                ref.insert(again)
                _check(m, ref, (lengths, short, "again"))
                m.close()
    finally:
        ctx.profile_enable(False)


# ---- chunk invariance ----
@pytest.fixture(scope="module")
def stream_state():
    return run(1.0, [K.stream()]).extract()


@pytest.mark.parametrize("road", ROADS)
@pytest.mark.parametrize("cut", ["one", 7, 256, 257, "random"])
def test_chunk_invariance(ctx, stream_state, cut, road):
    pts = K.stream()
    chunks = [pts] if cut == "one" else K.random_cut(pts) if cut == "random" else K.cut(pts, cut)
    m = ctx.voxel_map(1.0, MIN_CAPACITY)
    for ch in chunks:
        m.insert(_arg(ch, road))
    assert same_state(_state(m), stream_state) and m.points_inserted == len(pts)
    m.close()


@pytest.mark.parametrize("road", ROADS)
def test_chunks_of_one_point(ctx, road):
    pts = K.stream()[:300]
    m, ref = _both(ctx, 1.0, K.cut(pts, 1), road)
    whole = run(1.0, [pts])
    assert same_state(_check(m, ref), whole.extract())
    m.close()


@pytest.mark.parametrize("road", ROADS)
def test_order_sensitive_input_is_folded_in_stream_order(ctx, road):
    pts = K.order_sensitive()
    want = run(1.0, [pts]).extract()
    for chunks in ([pts], K.cut(pts, 1), K.cut(pts, 7), K.cut(pts, 256), K.cut(pts, 257), K.random_cut(pts, seed=9)):
        m, ref = _both(ctx, 1.0, chunks, road)
        assert same_state(_check(m, ref), want)
        m.close()


# ---- growth ----
@pytest.mark.parametrize("road", ROADS)
def test_growth_at_every_doubling_and_reset(ctx, road):
    ctx.profile_enable(True)
    try:
        m, ref, slots = ctx.voxel_map(1.0, 1), VoxelMapChecker(1.0), MIN_CAPACITY       # 1 slot asked for: the floor
        for round_ in range(2):
            for pts, r, want in K.growth_steps():
                ctx.profile_reset()
                m.insert(_arg(pts, road))
                ref.insert(pts)
                _check(m, ref, (round_, r, want))
                grew = want > slots and round_ == 0                                     # the second round finds the table large enough
                assert ("voxel_map_rehash" in _rows(ctx)) == grew, (round_, r, want, _rows(ctx))
                slots = max(slots, want)
            first = _state(m) if round_ == 0 else first
            if round_ == 0:
                m.reset()
                ref.reset()
                assert len(m) == 0 and m.points_inserted == 0 and _state(m)[0].shape == (0, 3)
        assert same_state(_state(m), first)
        m.close()
    finally:
        ctx.profile_enable(False)


# ---- keys ----
@pytest.mark.parametrize("road", ROADS)
def test_keys_faces_products_negatives_nans_and_the_range_ends(ctx, road):
    cases = [(0.5, K.faces()), (1.0, K.negatives()), (1.0, K.nan_points()), (1.0, K.range_points())]
    cases += [(vs, K.product_vs_division(vs)) for vs in (0.1, 0.3, 0.7)] + [(1.0, K.reciprocal_case(c)) for c in (3, 7, 49)]
    for vs, pts in cases:
        m, ref = _both(ctx, vs, [pts], road)
        _check(m, ref, vs)
        m.close()
    got = ctx.voxel_map(1.0)
    got.insert(_arg(K.range_points(), road))
    keys = got.extract(keys=True)[1]
    assert keys.min() == -KEY_LIMIT and keys.max() == KEY_LIMIT - 1
    got.close()


@pytest.mark.parametrize("road", ROADS)
def test_a_point_out_of_range_refuses_the_chunk_and_leaves_the_map(ctx, road):
    m, ref = _both(ctx, 1.0, [K.line_cloud(257, 9)], road, MIN_CAPACITY)
    before = _check(m, ref)
    base = K.line_cloud(300, 3, seed=4)
    for bad in K.out_of_range_points():
        for axis in range(3):
            pts = base.copy()
            pts[len(pts) // 2, axis] = bad
            with pytest.raises(tc.Unsupported) as e:
                m.insert(_arg(pts, road))
            assert "2^20" in str(e.value)
            assert len(m) == len(ref) and m.points_inserted == ref.points
    assert same_state(_state(m), before)
    m.insert(_arg(base, road))                      # the map still takes a valid chunk
    ref.insert(base)
    _check(m, ref)
    m.close()


# ---- extraction rules ----
def test_extraction_rules_through_the_raw_entry_points(ctx):
    L = _lib.load_companion("threecrate_hip_voxelmap.h")
    m, ref = _both(ctx, 1.0, [K.stream()[:2000]], "numpy")
    want = ref.extract()
    v = len(ref)
    n = C.c_size_t(0)
    assert L.tc_voxel_map_extract(m._h, None, None, None, None, 0, C.byref(n)) == _lib.TC_OK and n.value == v      # the count call
    for fn, dev in ((L.tc_voxel_map_extract, None), (L.tc_voxel_map_extract_device, "cuda:0")):
        for cap in (v - 1, v, v + 1):
            for mask in range(1, 16):               # every subset of outputs but the empty one
                if dev is None:
                    out = [np.full((v + 1, 3), -7, np.int32), np.full(v + 1, 7, np.uint32), np.full((v + 1, 3), -7.0), np.full((v + 1, 3), -7.0, F)]
                else:
                    out = [torch.full((v + 1, 3), -7, dtype=torch.int32, device=dev), torch.full((v + 1,), 7, dtype=torch.int32, device=dev),
                           torch.full((v + 1, 3), -7.0, dtype=torch.float64, device=dev), torch.full((v + 1, 3), -7.0, dtype=torch.float32, device=dev)]
                    torch.cuda.synchronize()
                ptr = [api._ptr(a) if mask >> k & 1 else None for k, a in enumerate(out)]
                n = C.c_size_t(0)
                rc = fn(m._h, ptr[0], ptr[1], ptr[2], ptr[3], cap, C.byref(n))
                host = [a if dev is None else a.cpu().numpy() for a in out]
                host[1] = host[1].view(np.uint32)
                assert n.value == v
                if cap < v:
                    assert rc == _lib.TC_INVALID_DATA
                    assert (host[0] == -7).all() and (host[1] == 7).all() and (host[2] == -7).all() and (host[3] == -7).all()
                    continue
                assert rc == _lib.TC_OK
                for k, ref_a in enumerate((want[1], want[2], want[3], want[0])):
                    if mask >> k & 1:
                        assert same_bits(host[k][:v], ref_a), (cap, mask, k)
                        assert (host[k][v:] == (7 if k == 1 else -7)).all()
                    else:
                        assert (host[k] == (7 if k == 1 else -7)).all()
    more = K.stream()[2000:3000]                    # extraction does not change the map: inserting goes on
    m.insert(more)
    ref.insert(more)
    _check(m, ref)
    cent = m.extract()
    assert isinstance(cent, np.ndarray) and same_bits(cent, ref.extract()[0])
    dev = m.extract(keys=True, device="cuda:0")
    assert same_bits(dev[0].cpu().numpy(), ref.extract()[0]) and np.array_equal(dev[1].cpu().numpy(), ref.extract()[1])
    m.close()


# ---- handles ----
def test_two_maps_on_one_context_do_not_meet(ctx):
    a, ra = _both(ctx, 1.0, [], "numpy", MIN_CAPACITY)
    b, rb = _both(ctx, 0.5, [], "torch")
    for i, ch in enumerate(K.cut(K.stream(), 500)):
        (a if i % 2 == 0 else b).insert(_arg(ch, "numpy" if i % 2 == 0 else "torch"))
        (ra if i % 2 == 0 else rb).insert(ch)
    _check(a, ra)
    _check(b, rb)
    a.close()
    _check(b, rb)
    b.close()


def test_a_map_used_after_the_other_users_of_the_pinned_block(ctx):
    from threecrate_amd import synth
    pts = K.stream()
    src, tgt, _ = synth.registration_pair(2000, seed=3)

    def steps(c):
        out = [np.asarray(c.voxel_grid_filter(tgt, 0.1))]
        m = c.voxel_map(1.0, MIN_CAPACITY)
        m.insert(pts[:3000])
        r = c.icp_detailed(src, tgt, None, 10, None, 0.0)
        out += [np.asarray(r.transformation), np.asarray(c.estimate_normals(tgt, 10))]
        m.insert(pts[3000:])
        out += list(_state(m))
        m.close()
        return out
    fresh = tc.GpuContext(0)
    try:
        alone = steps(fresh)
    finally:
        fresh.close()
    together = steps(ctx)
    assert len(alone) == len(together) and all(same_bits(a, b) for a, b in zip(alone, together))
    assert same_state(together[3:], run(1.0, [pts]).extract())


def test_a_context_closes_the_handles_made_on_it_before_itself():
    """a handle points into its context: closing the context first destroys its live children, so a late close() or __del__ of one is quiet"""
    c = tc.GpuContext(0)
    m, vol = c.voxel_map(1.0, MIN_CAPACITY), c.tsdf_volume(0.01, 0.03, (8, 8, 8))
    dropped = c.voxel_map(1.0, MIN_CAPACITY)
    m.insert(K.line_cloud(300, 2))
    del dropped                                     # a child that is gone is not remembered
    assert len(m) == 300 and len(c._children) == 2
    c.close()
    assert m._h is None and vol._h is None
    m.close()
    vol.close()


# ---- launch rows ----
def test_launch_rows_name_the_kernels_that_ran(ctx):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        m = ctx.voxel_map(1.0, MIN_CAPACITY)
        m.insert(K.line_cloud(100, 2))
        assert _rows(ctx) == {"voxel_map_sort": 1, "voxel_map_insert": 1}
        m.insert(K.line_cloud(100, 2, seed=1))      # the same 100 voxels, but 2 (V + R) = 400 > 256: the table doubles
        assert _rows(ctx) == {"voxel_map_sort": 2, "voxel_map_insert": 2, "voxel_map_rehash": 1}
        m.insert(K.long_runs((LONG_RUN + 1, 2 * LONG_RUN + 5)))
        assert _rows(ctx) == {"voxel_map_sort": 3, "voxel_map_insert": 3, "voxel_map_rehash": 1, "voxel_map_insert_long": 1}
        assert len(m) == 100 + 1 and _rows(ctx).get("voxel_map_extract") is None    # (the long voxel (0, 0, 0) was there already) the count needs no extraction
        m.extract()
        assert _rows(ctx)["voxel_map_extract"] == 1
        m.close()
    finally:
        ctx.profile_enable(False)


# ---- errors, in the header's order, through every road ----
def test_errors(ctx):
    L = _lib.load_companion("threecrate_hip_voxelmap.h")
    for vs in (0.0, -1.0, float("nan")):
        with pytest.raises(tc.InvalidData) as e:
            ctx.voxel_map(vs)
        assert str(e.value) == "voxel_size must be positive"
    with pytest.raises(tc.Unsupported):
        ctx.voxel_map(1.0, (1 << 28) + 1)
    h = C.c_void_p()
    bad = _lib.VoxelMapConfigC(0.0, (1 << 28) + 1)                  # voxel_size is checked before the capacity
    assert L.tc_voxel_map_create(ctx._h, C.byref(bad), C.byref(h)) == _lib.TC_INVALID_DATA and h.value is None
    assert L.tc_voxel_map_create(ctx._h, None, C.byref(h)) == _lib.TC_INVALID_DATA
    m = ctx.voxel_map(1.0)
    xyz = np.full((4, 3), 0.5, F)
    for fn in (L.tc_voxel_map_insert, L.tc_voxel_map_insert_device):
        assert fn(m._h, None, 0) == _lib.TC_OK                          # n == 0 comes before the NULL check
        assert fn(m._h, None, 4) == _lib.TC_INVALID_DATA
        assert fn(m._h, xyz.ctypes.data, 0xFFFFFFF0) == _lib.TC_UNSUPPORTED      # the count comes before any read
    assert len(m) == 0 and m.points_inserted == 0
    m.insert(np.zeros((0, 3), F))
    m.insert(torch.zeros((0, 3), device="cuda:0"))
    assert len(m) == 0
    n = C.c_size_t(7)
    for fn in (L.tc_voxel_map_extract, L.tc_voxel_map_extract_device):
        assert fn(m._h, None, None, None, None, 0, None) == _lib.TC_INVALID_DATA
        assert fn(m._h, None, None, None, xyz.ctypes.data, 0, C.byref(n)) == _lib.TC_OK and n.value == 0      # nothing to write
    m.insert(xyz)
    for fn in (L.tc_voxel_map_extract, L.tc_voxel_map_extract_device):
        assert fn(m._h, None, None, None, xyz.ctypes.data, 0, C.byref(n)) == _lib.TC_INVALID_DATA and n.value == 1
    assert (xyz == 0.5).all()
    m.close()
    m.close()                                                           # closing twice is quiet


# ---- compat ----
def test_compat_realtime_voxel_filter_has_the_maps_bits(ctx):
    import threecrate_amd.compat as threecrate
    pts = K.stream()
    rt = threecrate.RealtimeVoxelFilter(voxel_size=1.0, max_queue_depth=512)
    rt._BATCH = 1000                                                    # several inserts, some of them partial
    for p in pts[:50]:
        rt.send(p)
    assert rt.try_send(pts[50].astype(np.float64)) is True
    assert rt.send_batch(pts[51:]) == len(pts) - 51
    mt = rt.metrics()
    assert mt.items_queued == len(pts) and mt.items_dropped == 0 and mt.items_processed + mt.estimated_queue_depth == len(pts)
    cloud = rt.finish()
    m, ref = _both(ctx, 1.0, [pts], "numpy")
    assert isinstance(cloud, threecrate.PointCloud) and same_bits(cloud.to_numpy(), m.extract()) and same_bits(cloud.to_numpy(), ref.extract()[0])
    m.close()
    bad = threecrate.RealtimeVoxelFilter(1.0)
    bad.send_batch(np.full((3, 3), 3e9, F))                             # buffered; the insert fails at the flush
    with pytest.raises(RuntimeError):
        bad.finish()
