"""Statistical and radius outlier removal on the MI355X against tests/outlier_checker.py: mean distances to the bit at every
register-list boundary and on the hard clouds, threshold and outputs consistent with each other and with the reference's kept set,
exact set equality for the threshold and radius variants, errors through every road, run-to-run bit equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib
from tests import outlier_checker as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _bits(a):
    return np.ascontiguousarray(_host(a), np.float32).view(np.uint32)


def assert_same_floats(got, ref):
    got, ref = np.asarray(_host(got), np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.nonzero(got.view(np.uint32)[~nan] != ref.view(np.uint32)[~nan])[0]
    assert len(bad) == 0, (len(bad), got[~nan][bad[:5]], ref[~nan][bad[:5]])


# ---- clouds (made once; the checker's means are cached per cloud and k) ----
@functools.lru_cache(None)
def cloud(name):
    rng = np.random.default_rng(17)
    if name == "uniform":
        return rng.random((3001, 3), dtype=np.float32)
    if name == "lattice":
        return OC.lattice(12)                                   # 1728 points, spacing 0.25: exact ties at the (k + 1)-th place
    if name == "far":                                           # far outliers at 30 extents; 3 005 points, below the builder's 4 096: the
        #                                                         grid's box is exact (the clamped ones: tests/filter_cases.py)
        p = rng.random((3000, 3), dtype=np.float32)
        far = np.array([[30, 30, 30], [-30, 0.5, 0.5], [0.5, 31, -29], [30.5, 30, 30], [0.2, 0.2, -30]], np.float32)
        return np.concatenate([p[:1500], far, p[1500:]])
    if name == "dup6":                                          # one point 6 times: at k = 4 its k + 1 nearest are all twins
        p = rng.random((700, 3), dtype=np.float32)
        p[[3, 90, 91, 300, 555, 699]] = p[3]
        return p
    if name == "dup2":
        p = rng.random((700, 3), dtype=np.float32)
        p[400] = p[20]
        return p
    if name == "five":
        return rng.random((5, 3), dtype=np.float32)
    if name == "one":
        return np.array([[0.25, -1.0, 3.0]], np.float32)
    if name == "nonfinite":
        p = rng.random((900, 3), dtype=np.float32)
        p[7, 0] = np.nan
        p[450, 2] = np.inf
        p[899, 1] = -np.inf
        return p
    raise KeyError(name)


@functools.lru_cache(None)
def ref_mean(name, k):
    return OC.mean_distances(cloud(name), k)


@functools.lru_cache(None)
def sor_case(n, k):
    p = OC.sor_cloud(n)
    return p, OC.mean_distances(p, k)


# ---- 1, 2: mean distances to the bit ----
@pytest.mark.parametrize("k", [1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 300])
def test_mean_distance_bit_equal_at_every_list_size(ctx, k):
    r = ctx.statistical_outlier_removal_detailed(cloud("uniform"), k, 1.0)
    assert_same_floats(r.mean_distance, ref_mean("uniform", k))


@pytest.mark.parametrize("name,k", [("lattice", 6), ("lattice", 8), ("lattice", 26), ("lattice", 140), ("far", 8), ("far", 40), ("far", 200),
                                    ("dup6", 4), ("dup2", 4), ("five", 8), ("five", 200), ("one", 1), ("one", 5), ("nonfinite", 8),
                                    ("nonfinite", 150)])
def test_mean_distance_bit_equal_on_hard_clouds(ctx, name, k):
    p, ref = cloud(name), ref_mean(name, k)
    r = ctx.statistical_outlier_removal_detailed(p, k, 1.0)
    assert_same_floats(r.mean_distance, ref)
    d = ctx.statistical_outlier_removal_detailed(_dev(p), k, 1.0)               # the device road
    assert_same_floats(d.mean_distance, ref)
    assert np.array_equal(_host(d.index), r.index) and np.array_equal(_bits(d.points), _bits(r.points))
    assert d.threshold == r.threshold or (np.isnan(d.threshold) and np.isnan(r.threshold))
    if name == "dup6":
        assert np.all(ref[[3, 90, 91, 300, 555, 699]] == 0.0)
    if name == "one":
        assert r.index.tolist() == [0] and r.threshold == 0.0                   # mean 0 <= threshold 0
    if name == "nonfinite":
        assert np.isnan(_host(r.mean_distance)[[7, 450, 899]]).all() and not set(r.index.tolist()) & {7, 450, 899}


# ---- 3: threshold and outputs ----
def _check_outputs(p, r, keep):
    idx = _host(r.index).astype(np.int64) & 0xFFFFFFFF
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, keep)
    assert len(_host(r.points)) == len(idx)
    assert np.array_equal(_bits(r.points), p[idx].view(np.uint32))


@pytest.mark.parametrize("n,k", OC.SOR_CASES)
def test_threshold_and_outputs_are_consistent_and_kept_set_equals_the_reference(ctx, n, k):
    p, ref = sor_case(n, k)
    for mult in OC.SOR_MULTIPLIERS:
        for arr in (p, _dev(p)):
            r = ctx.statistical_outlier_removal_detailed(arr, k, mult)
            assert_same_floats(r.mean_distance, ref)
            t_ref, t_f64 = OC.thresholds(ref, mult)
            thr = np.float32(r.threshold)
            print(f"n={n} k={k} mult={mult}: threshold_used={thr!r} t_f64={t_f64!r} t_ref={t_ref!r} kept={len(_host(r.index))}")
            assert abs(int(thr.view(np.uint32)) - int(t_f64.view(np.uint32))) <= 1
            _check_outputs(p, r, OC.sor_keep(ref, thr))
            # tests/test_outliers_cpu.py shows that no mean lies between the two thresholds on these inputs: every point is compared
            assert np.array_equal(_host(r.index).astype(np.int64), OC.sor_keep(ref, t_ref))


def test_return_shapes(ctx):
    p = cloud("far")
    out = ctx.statistical_outlier_removal(p, 8, 1.0)
    out2, idx = ctx.statistical_outlier_removal(p, 8, 1.0, return_index=True)
    out3, idx3, mean = ctx.statistical_outlier_removal(p, 8, 1.0, True, True)
    assert out.dtype == np.float32 and out.shape == (len(idx), 3) and idx.dtype == np.uint32 and mean.shape == (len(p),)
    assert np.array_equal(out, out2) and np.array_equal(out, out3) and np.array_equal(idx, idx3) and np.array_equal(out, p[idx])
    assert len(idx) < len(p) and not set(idx.tolist()) & set(range(1500, 1505))          # the far points go
    assert np.array_equal(tc.gpu_remove_statistical_outliers(ctx, p, 8, 1.0), out)
    assert np.array_equal(tc.statistical_outlier_removal(p, 8, 1.0, ctx=ctx), out)
    assert np.array_equal(threecrate.remove_statistical_outliers(threecrate.PointCloud(p), 8, 1.0).to_numpy(), out)
    dev = ctx.statistical_outlier_removal(_dev(p), 8, 1.0)
    assert hasattr(dev, "device") and np.array_equal(_host(dev), out)
    e = ctx.statistical_outlier_removal(np.zeros((0, 3), np.float32), 8, 1.0, True, True)
    assert e[0].shape == (0, 3) and e[1].shape == (0,) and e[2].shape == (0,)


# ---- 4: the threshold variant ----
@pytest.mark.parametrize("name,k", [("uniform", 8), ("lattice", 6), ("far", 20), ("nonfinite", 8)])
def test_with_threshold_set_equality_on_and_below_a_mean(ctx, name, k):
    p, ref = cloud(name), ref_mean(name, k)
    fin = np.nonzero(~np.isnan(ref))[0]
    i = fin[np.argsort(ref[fin], kind="stable")[len(fin) // 2]]               # a point in the middle of the distribution
    on, below = ref[i], np.nextafter(ref[i], np.float32(0))
    for arr in (p, _dev(p)):
        out, idx, mean = ctx.statistical_outlier_removal_with_threshold(arr, k, on, True, True)
        assert_same_floats(mean, ref)
        _check_outputs(p, tc.OutlierResult(out, idx), OC.sor_keep(ref, on))
        assert i in _host(idx)
        out, idx = ctx.statistical_outlier_removal_with_threshold(arr, k, below, return_index=True)
        _check_outputs(p, tc.OutlierResult(out, idx), OC.sor_keep(ref, below))
        assert i not in _host(idx)
    assert np.array_equal(tc.statistical_outlier_removal_with_threshold(p, k, on, ctx=ctx), p[OC.sor_keep(ref, on)])


# ---- 5: the radius filter ----
def _radius_case(ctx, p, radius, min_neighbors):
    keep = OC.radius_keep(p, radius, min_neighbors)
    for arr in (p, _dev(p)):
        out, idx = ctx.radius_outlier_removal(arr, radius, min_neighbors, return_index=True)
        _check_outputs(p, tc.OutlierResult(out, idx), keep)
    return keep


@pytest.mark.parametrize("radius", [0.25, 0.5])
def test_radius_on_the_lattice_at_the_count_and_either_side(ctx, radius):
    p = cloud("lattice")
    counts = OC.radius_counts(p, radius) - 1
    full = int(counts.max())                                    # an interior point: 6 at 0.25 (d2 == r2 exactly), 32 at 0.5
    assert full == (6 if radius == 0.25 else 32)
    sizes = [len(_radius_case(ctx, p, radius, m)) for m in (full - 1, full, full + 1)]
    assert sizes[0] > sizes[1] == (12 - 2 * round(radius / 0.25)) ** 3 and sizes[2] == 0           # the interior of the 12^3 lattice
    assert len(_radius_case(ctx, p, radius, 1)) == len(p)
    assert len(_radius_case(ctx, p, radius, len(p) + 1)) == 0
    assert len(_radius_case(ctx, p, radius, 2 ** 63)) == 0


@pytest.mark.parametrize("name,radius,mins", [("one", 1.0, [1]), ("far", 0.1, [1, 3, 6]), ("far", 1.5, [1, 2, 2999]), ("nonfinite", 0.12, [1, 4]),
                                              ("nonfinite", 1e19, [1, 896, 897]),
                                              ("nonfinite", 1.8e19, [896]),          # r * r = 3.24e38 is finite: the indexed walk, one cell
                                              ("dup6", 1e-30, [1, 5, 6]), ("dup2", 1e-30, [1, 2]), ("uniform", 0.07, [2, 5])])
def test_radius_set_equality(ctx, name, radius, mins):
    p = cloud(name)
    for m in mins:
        keep = _radius_case(ctx, p, radius, m)
        if name == "one":
            assert len(keep) == 0
        if name == "dup6" and m <= 5:
            assert keep.tolist() == [3, 90, 91, 300, 555, 699]


@pytest.mark.parametrize("name", ["nonfinite", "far"])
def test_radius_infinite_and_nan(ctx, name):
    p = cloud(name)
    nfin = int(np.all(np.isfinite(p), axis=1).sum())
    for radius in (np.inf, 3e19):                               # r * r overflows as well
        assert len(_radius_case(ctx, p, radius, nfin - 1)) == nfin
        assert len(_radius_case(ctx, p, radius, nfin)) == 0
    assert len(_radius_case(ctx, cloud("one"), np.inf, 1)) == 0
    assert len(_radius_case(ctx, p, np.nan, 1)) == 0
    assert np.array_equal(tc.gpu_radius_outlier_removal(ctx, p, 0.1, 2), p[OC.radius_keep(p, 0.1, 2)])
    assert np.array_equal(tc.radius_outlier_removal(p, 0.1, 2, ctx=ctx), p[OC.radius_keep(p, 0.1, 2)])
    assert np.array_equal(threecrate.remove_radius_outliers(threecrate.PointCloud(p), 0.1, 2).to_numpy(), p[OC.radius_keep(p, 0.1, 2)])


def test_nan_parameters_keep_nothing(ctx):
    p = cloud("five")
    r = ctx.statistical_outlier_removal_detailed(p, 2, np.nan)
    assert len(r.index) == 0 and np.isnan(r.threshold)
    assert_same_floats(r.mean_distance, ref_mean("five", 2))
    out, idx, mean = ctx.statistical_outlier_removal_with_threshold(p, 2, np.nan, True, True)
    assert len(idx) == 0 and out.shape == (0, 3)
    assert_same_floats(mean, ref_mean("five", 2))


# ---- 6: errors and limits, the same through every road ----
SOR_ERRORS = [((0, 1.0), tc.InvalidData, "k_neighbors must be greater than 0"),
              ((0, -1.0), tc.InvalidData, "k_neighbors must be greater than 0"),           # the reference's order
              ((5, 0.0), tc.InvalidData, "std_dev_multiplier must be positive"),
              ((5, -1.0), tc.InvalidData, "std_dev_multiplier must be positive"),
              ((2048, 1.0), tc.Unsupported, "statistical_outlier_removal: k_neighbors > 2047 is not supported by the HIP backend")]
THR_ERRORS = [((0, 1.0), tc.InvalidData, "k_neighbors must be greater than 0"),
              ((5, 0.0), tc.InvalidData, "threshold must be positive"),
              ((5, -2.0), tc.InvalidData, "threshold must be positive"),
              ((2048, 1.0), tc.Unsupported, "statistical_outlier_removal: k_neighbors > 2047 is not supported by the HIP backend")]
RAD_ERRORS = [((0.0, 1), tc.InvalidData, "radius must be positive"),
              ((-1.0, 0), tc.InvalidData, "radius must be positive"),                       # the reference's order
              ((1.0, 0), tc.InvalidData, "min_neighbors must be greater than 0")]


def _raises(fn, exc, msg):
    with pytest.raises(exc) as e:
        fn()
    assert str(e.value) == msg


def test_errors_through_every_road(ctx):
    p = cloud("five")
    empty = np.zeros((0, 3), np.float32)
    for arr in (p, _dev(p)):                                    # host and _device entry points
        for args, exc, msg in SOR_ERRORS:
            _raises(lambda: ctx.statistical_outlier_removal(arr, *args), exc, msg)
        for args, exc, msg in THR_ERRORS:
            _raises(lambda: ctx.statistical_outlier_removal_with_threshold(arr, *args), exc, msg)
        for args, exc, msg in RAD_ERRORS:
            _raises(lambda: ctx.radius_outlier_removal(arr, *args), exc, msg)
    L, n_out = ctx._L, C.c_size_t(9)                            # the empty cloud returns OK before any other check
    for args, _, _ in SOR_ERRORS:
        assert ctx.statistical_outlier_removal(empty, *args).shape == (0, 3)
        assert L.tc_statistical_outlier_removal_device(ctx._h, None, 0, *args, None, None, None, C.byref(n_out), None) == 0 and n_out.value == 0
    for args, _, _ in THR_ERRORS:
        assert ctx.statistical_outlier_removal_with_threshold(empty, *args).shape == (0, 3)
        assert L.tc_statistical_outlier_removal_with_threshold_device(ctx._h, None, 0, *args, None, None, None, C.byref(n_out)) == 0
    for args, _, _ in RAD_ERRORS:
        assert ctx.radius_outlier_removal(empty, *args).shape == (0, 3)
        assert L.tc_radius_outlier_removal_device(ctx._h, None, 0, *args, None, None, C.byref(n_out)) == 0 and n_out.value == 0
    for args, exc, msg in SOR_ERRORS:                           # module functions, facade, compat
        _raises(lambda: tc.statistical_outlier_removal(p, *args, ctx=ctx), exc, msg)
        _raises(lambda: tc.gpu_remove_statistical_outliers(ctx, p, *args), exc, msg)
        _raises(lambda: threecrate.remove_statistical_outliers(threecrate.PointCloud(p), *args), RuntimeError, msg)
    for args, exc, msg in THR_ERRORS:
        _raises(lambda: tc.statistical_outlier_removal_with_threshold(p, *args, ctx=ctx), exc, msg)
    for args, exc, msg in RAD_ERRORS:
        _raises(lambda: tc.radius_outlier_removal(p, *args, ctx=ctx), exc, msg)
        _raises(lambda: tc.gpu_radius_outlier_removal(ctx, p, *args), exc, msg)
        _raises(lambda: threecrate.remove_radius_outliers(threecrate.PointCloud(p), *args), RuntimeError, msg)
    assert len(threecrate.remove_statistical_outliers(threecrate.PointCloud(empty), 0, -1.0)) == 0
    assert len(threecrate.remove_radius_outliers(threecrate.PointCloud(empty), -1.0, 0)) == 0


def test_point_count_limit(ctx):
    """n >= 2^32 - 16 is refused before anything is read"""
    L = ctx._L
    n_out, thr, big = C.c_size_t(0), C.c_float(0), 2 ** 32 - 16
    p = cloud("five")
    for fn in (L.tc_statistical_outlier_removal, L.tc_statistical_outlier_removal_device):
        assert fn(ctx._h, p.ctypes.data, big, 4, 1.0, None, None, None, C.byref(n_out), C.byref(thr)) == _lib.TC_UNSUPPORTED
    for fn in (L.tc_statistical_outlier_removal_with_threshold, L.tc_statistical_outlier_removal_with_threshold_device):
        assert fn(ctx._h, p.ctypes.data, big, 4, 1.0, None, None, None, C.byref(n_out)) == _lib.TC_UNSUPPORTED
    for fn in (L.tc_radius_outlier_removal, L.tc_radius_outlier_removal_device):
        assert fn(ctx._h, p.ctypes.data, big, 1.0, 1, None, None, C.byref(n_out)) == _lib.TC_UNSUPPORTED
    assert L.tc_last_error_message(ctx._h) == b"more than 2^32 points"


# ---- 7: run to run ----
def test_two_calls_are_bit_identical(ctx):
    p, _ = sor_case(20000, 8)
    for arr in (p, _dev(p)):
        a = ctx.statistical_outlier_removal_detailed(arr, 8, 1.5)
        b = ctx.statistical_outlier_removal_detailed(arr, 8, 1.5)
        assert np.array_equal(_bits(a.mean_distance), _bits(b.mean_distance)) and a.threshold == b.threshold
        assert np.array_equal(_host(a.index), _host(b.index)) and np.array_equal(_bits(a.points), _bits(b.points))
        ra, rb = (ctx.radius_outlier_removal(arr, 0.05, 3, return_index=True) for _ in range(2))
        assert np.array_equal(_host(ra[1]), _host(rb[1])) and np.array_equal(_bits(ra[0]), _bits(rb[0]))


def test_n_out_and_null_outputs_at_the_entry_points(ctx):
    """n_out itself against the checker's count, in over-allocated buffers whose rows past n_out stay as they were; each output
    may be NULL."""
    L, p = ctx._L, cloud("far")
    n, k, mult, radius, min_nb = len(p), 8, 1.0, 0.1, 3
    ref = ref_mean("far", k)
    pad = 7
    for road in ("host", "device"):
        def buf(shape, dtype, fill):
            a = np.full(shape, fill, dtype)
            return _dev(a) if road == "device" else a
        x = _dev(p) if road == "device" else p
        ptr = lambda a: None if a is None else (a.data_ptr() if road == "device" else a.ctypes.data)
        sor = L.tc_statistical_outlier_removal_device if road == "device" else L.tc_statistical_outlier_removal
        rad = L.tc_radius_outlier_removal_device if road == "device" else L.tc_radius_outlier_removal
        if road == "device":
            import torch
            ready = torch.cuda.synchronize          # the buffers are filled on torch's stream, the library reads them on its own
        else:
            ready = lambda: None
        for which in ("all", "xyz only", "index only", "none"):
            out = buf((n + pad, 3), np.float32, -7.0) if which in ("all", "xyz only") else None
            idx = buf(n + pad, np.int32, -7) if which in ("all", "index only") else None
            mean = buf(n + pad, np.float32, -7.0) if which == "all" else None
            n_out, thr = C.c_size_t(0), C.c_float(0)
            ready()
            assert sor(ctx._h, ptr(x), n, k, mult, ptr(out), ptr(idx), ptr(mean), C.byref(n_out), C.byref(thr)) == 0
            keep = OC.sor_keep(ref, np.float32(thr.value))
            assert n_out.value == len(keep) < n
            if out is not None:
                o = _host(out)
                assert np.array_equal(o[:len(keep)].view(np.uint32), p[keep].view(np.uint32)) and np.all(o[len(keep):] == -7.0)
            if idx is not None:
                i = _host(idx)
                assert np.array_equal(i[:len(keep)], keep) and np.all(i[len(keep):] == -7)
            if mean is not None:
                assert_same_floats(_host(mean)[:n], ref)
                assert np.all(_host(mean)[n:] == -7.0)
            out = buf((n + pad, 3), np.float32, -7.0) if which in ("all", "xyz only") else None
            idx = buf(n + pad, np.int32, -7) if which in ("all", "index only") else None
            ready()
            assert rad(ctx._h, ptr(x), n, radius, min_nb, ptr(out), ptr(idx), C.byref(n_out)) == 0
            keep = OC.radius_keep(p, radius, min_nb)
            assert n_out.value == len(keep) < n
            if out is not None:
                o = _host(out)
                assert np.array_equal(o[:len(keep)].view(np.uint32), p[keep].view(np.uint32)) and np.all(o[len(keep):] == -7.0)
            if idx is not None:
                i = _host(idx)
                assert np.array_equal(i[:len(keep)], keep) and np.all(i[len(keep):] == -7)
