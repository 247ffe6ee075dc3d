"""Outlier removal filters without a GPU: the checker (tests/outlier_checker.py) against the reference's own examples and unit tests
(filtering.rs:155-165, :237-247, :397-534), the names and the null-context behaviour of its surface (include/threecrate_hip_filters.h)
and the precondition of the GPU test's comparison with the reference's f32 threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import outlier_checker as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sor(points, k, mult):
    mean = OC.mean_distances(points, k)
    t_ref, _ = OC.thresholds(mean, mult)
    return OC.sor_keep(mean, t_ref), mean


# ---- the reference's doc examples and unit tests ----
def test_radius_doc_example():
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [10, 10, 10]], np.float32)
    assert OC.radius_keep(pts, 0.5, 2).tolist() == [0, 1, 2]


def test_statistical_doc_example():
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [10, 10, 10]], np.float32)
    keep, mean = _sor(pts, 3, 1.0)
    assert keep.tolist() == [0, 1, 2]
    # point 0: (1 + 1 + sqrt(300)) / 3 in sequential f32
    want = (np.float32(1) + np.float32(1) + np.sqrt(np.float32(300))) / np.float32(3)
    assert mean[0] == want


def test_statistical_single_point():
    keep, mean = _sor(np.zeros((1, 3), np.float32), 1, 1.0)
    assert keep.tolist() == [0] and mean.tolist() == [0.0]


def _grid(side):
    return np.array([[np.float32(i) * np.float32(0.1), np.float32(j) * np.float32(0.1), np.float32(k) * np.float32(0.1)]
                     for i in range(side) for j in range(side) for k in range(side)], np.float32)


def test_statistical_with_outliers():
    pts = np.concatenate([_grid(10), np.array([[10, 10, 10], [-10, -10, -10], [5, 5, 5]], np.float32)])
    keep, _ = _sor(pts, 5, 1.0)
    assert 0 < len(keep) < len(pts)
    assert 1000 not in keep and 1001 not in keep


def test_statistical_no_outliers():
    pts = _grid(5)
    keep, _ = _sor(pts, 5, 1.0)
    assert len(keep) > len(pts) * 8 // 10


def test_statistical_with_threshold():
    pts = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [10, 10, 10]], np.float32)
    assert OC.sor_keep(OC.mean_distances(pts, 3), 0.5).tolist() == [0, 1, 2, 3]


def test_checker_conventions():
    """duplicates drop out of the mean (d2 == 0), fewer points than k + 1 use what there is, inert points are NaN"""
    pts = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    assert OC.mean_distances(pts, 2).tolist() == [0.0, 0.0, 0.0, 1.0]          # the two nearest of a triple are its twins
    assert OC.mean_distances(pts, 8).tolist() == [1.0, 1.0, 1.0, 1.0]
    pts = np.array([[0, 0, 0], [np.nan, 0, 0], [2, 0, 0], [0, np.inf, 0]], np.float32)
    m = OC.mean_distances(pts, 3)
    assert m[0] == 2.0 and m[2] == 2.0 and np.isnan(m[1]) and np.isnan(m[3])
    assert OC.radius_keep(pts, 2.0, 1).tolist() == [0, 2] and OC.radius_keep(pts, np.inf, 1).tolist() == [0, 2]
    assert OC.radius_keep(pts, np.inf, 2).tolist() == [] and OC.radius_keep(pts, np.nan, 1).tolist() == []


# ---- what is this feature's own of the surface (tests/test_abi_surfaces.py holds header, table, Rust file and library together) ----
def test_rust_facade_has_the_reference_names():
    lib_rs = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ("statistical_outlier_removal", "statistical_outlier_removal_with_threshold", "radius_outlier_removal",
               "gpu_remove_statistical_outliers", "gpu_radius_outlier_removal"):
        assert re.search(r"pub fn " + fn + r"\(", lib_rs), fn


def test_every_filter_export_returns_a_status_and_writes_nothing_without_a_context():
    L = _lib.load()
    n_out, thr = C.c_size_t(7), C.c_float(0)
    pts = np.zeros((4, 3), np.float32)
    sor = (None, pts.ctypes.data, 4, 2, 1.0, None, None, None, C.byref(n_out))
    assert L.tc_statistical_outlier_removal(*sor, C.byref(thr)) == _lib.TC_INVALID_DATA
    assert L.tc_statistical_outlier_removal_device(*sor, C.byref(thr)) == _lib.TC_INVALID_DATA
    assert L.tc_statistical_outlier_removal_with_threshold(*sor) == _lib.TC_INVALID_DATA
    assert L.tc_statistical_outlier_removal_with_threshold_device(*sor) == _lib.TC_INVALID_DATA
    rad = (None, pts.ctypes.data, 4, 1.0, 2, None, None, C.byref(n_out))
    assert L.tc_radius_outlier_removal(*rad) == _lib.TC_INVALID_DATA
    assert L.tc_radius_outlier_removal_device(*rad) == _lib.TC_INVALID_DATA
    assert n_out.value == 7          # nothing is written without a context


def test_python_surface():
    import threecrate_amd as tc
    import threecrate_amd.compat as threecrate
    for name in ("statistical_outlier_removal", "statistical_outlier_removal_with_threshold", "radius_outlier_removal"):
        assert callable(getattr(tc.GpuContext, name)) and callable(getattr(tc, name))
    assert callable(tc.gpu_remove_statistical_outliers) and callable(tc.gpu_radius_outlier_removal)
    assert "remove_statistical_outliers" in threecrate.__all__ and "remove_radius_outliers" in threecrate.__all__
    import inspect
    sig = inspect.signature(threecrate.remove_statistical_outliers)
    assert sig.parameters["k_neighbors"].default == 20 and sig.parameters["std_ratio"].default == 2.0      # threecrate.pyi:288-294


# ---- precondition of test_gpu_outliers.py::test_kept_set_equals_the_reference ----
@pytest.mark.parametrize("n,k", OC.SOR_CASES)
def test_no_mean_distance_lies_between_the_two_thresholds(n, k):
    """The backend sums the global statistics in f64, the reference in sequential f32.  On these inputs the two thresholds differ
    in the 6th-7th digit and no point's mean distance lies between them: the kept sets are the same, so the GPU test may demand
    set equality with the reference's threshold and leave no point out of the comparison."""
    mean = OC.mean_distances(OC.sor_cloud(n), k)
    for mult in OC.SOR_MULTIPLIERS:
        t_ref, t_f64 = OC.thresholds(mean, mult)
        lo, hi = min(t_ref, t_f64), max(t_ref, t_f64)
        print(f"n={n} k={k} mult={mult}: t_ref={t_ref!r} t_f64={t_f64!r} removed={int((mean > t_ref).sum())}")
        assert abs(float(t_ref) - float(t_f64)) <= 1e-5 * float(t_f64)
        assert int(((mean > lo) & (mean <= hi)).sum()) == 0
        removed = int((mean > t_ref).sum())
        assert 0.003 * n <= removed <= 0.03 * n, removed
