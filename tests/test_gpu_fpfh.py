"""FPFH descriptors on the MI355X: the reference's unit tests restated (features.rs:825-988), parity with the checker
(tests/fpfh_checker.py: every bin within 1e-5 on unambiguous points, an L1 bound on the others), edge cases, errors, the device
entry points and run-to-run bit equality."""
import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import synth
from tests import fpfh_checker as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = tc.GpuContext(0)
    yield c
    c.close()


def _np(pos, nrm):
    return np.ascontiguousarray(np.concatenate([pos, nrm], 1), np.float32)


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _parity(ctx, pos, nrm, radius, k, rows=None, min_strict=None):
    got = ctx.extract_fpfh_features_with_normals(_np(pos, nrm), radius, k)
    ref = F.fpfh(pos, nrm, radius, k, rows)
    if rows is not None:
        got = got[rows]
    return got, ref, F.compare(got, ref, min_strict=min_strict)


def plane_cloud(n):
    """make_plane_cloud (features.rs:807-825)"""
    side = int(np.ceil(np.sqrt(n)))
    step = np.float32(1.0) / np.float32(side)
    ij = [(i, j) for i in range(side) for j in range(side)][:n]
    pos = np.array([[np.float32(i) * step, np.float32(j) * step, 0.0] for i, j in ij], np.float32)
    return pos, np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))


# ---- the reference's unit tests (features.rs:825-988) ----
def test_fpfh_empty_cloud(ctx):
    assert ctx.extract_fpfh_features_with_normals(np.zeros((0, 6), np.float32)).shape == (0, 33)


def test_fpfh_descriptor_dimension(ctx):
    out = ctx.extract_fpfh_features_with_normals(_np(*plane_cloud(25)), 0.5, 5)
    assert out.shape == (25, 33) and out.dtype == np.float32


def test_fpfh_descriptor_non_negative(ctx):
    assert (ctx.extract_fpfh_features_with_normals(_np(*plane_cloud(25)), 0.5, 5) >= 0).all()


def test_fpfh_sub_histograms_normalised(ctx):
    out = ctx.extract_fpfh_features_with_normals(_np(*plane_cloud(36)), 0.5, 8)
    for part in range(3):
        s = out[:, part * 11:(part + 1) * 11].sum(1)
        assert np.all(np.abs(s - 1.0) < 1e-4) or np.all((np.abs(s - 1.0) < 1e-4) | (s == 0)), s


def test_fpfh_identical_clouds_same_descriptors(ctx):
    c = _np(*plane_cloud(25))
    assert np.array_equal(ctx.extract_fpfh_features_with_normals(c, 0.5, 5), ctx.extract_fpfh_features_with_normals(c, 0.5, 5))


def _ref_sphere():
    pts = []
    pi = np.float32(np.pi)
    for i in range(5):
        for j in range(5):
            th = pi * np.float32(i) / np.float32(4)
            ph = np.float32(2) * pi * np.float32(j) / np.float32(5)
            pts.append([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
    p = np.array(pts, np.float32)
    return p, p.copy()


def test_fpfh_plane_vs_sphere_differ(ctx):
    pd = ctx.extract_fpfh_features_with_normals(_np(*plane_cloud(25)), 0.5, 5)
    sp, sn = _ref_sphere()
    sd = ctx.extract_fpfh_features_with_normals(_np(sp, sn), 0.5, 5)
    assert (np.abs(pd[:, None, :] - sd[None, :, :]).sum(2) > 0.1).any()
    _parity(ctx, sp, sn, 0.5, 5)


def test_fpfh_from_xyz(ctx):
    g = np.array([[i * 0.1, j * 0.1, 0.0] for i in range(5) for j in range(5)], np.float32)
    out = ctx.extract_fpfh_features(g, 0.1, 10)
    assert out.shape == (25, 33)


def test_fpfh_invalid_radius(ctx):
    with pytest.raises(tc.InvalidData, match="search_radius must be positive"):
        ctx.extract_fpfh_features_with_normals(_np(*plane_cloud(9)), -1.0, 5)


def test_fpfh_single_point_all_zero(ctx):
    out = ctx.extract_fpfh_features_with_normals(np.array([[0, 0, 0, 0, 0, 1]], np.float32), 1.0, 1)
    assert out.shape == (1, 33) and (out == 0).all()


# ---- parity with the checker ----
def test_uniform_cloud_with_fallback_points(ctx):
    rng = np.random.default_rng(11)
    pos = rng.random((20000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(20000, 3)))
    got, ref, _ = _parity(ctx, pos, nrm, 0.055, 10, min_strict=0.99)
    assert (ref["nlist"] == 10).sum() > 1000 and (ref["nlist"] > 10).sum() > 1000       # both branches, many points each


def test_kitti_shaped_sweep(ctx):
    pos = np.ascontiguousarray(synth.kitti_shaped_cloud(azimuth_steps=600), np.float32)
    nrm = ctx.estimate_normals(pos, 10)[:, 3:].copy()
    rows = np.random.default_rng(2).choice(len(pos), 4000, replace=False)
    _parity(ctx, pos, nrm, 0.5, 10, rows=rows, min_strict=0.99)


def test_sphere(ctx):
    rng = np.random.default_rng(12)
    v = _unit(rng.normal(size=(5000, 3)))
    _parity(ctx, v, v, 0.1, 10, min_strict=0.99)


def test_flipped_normal_plane_bins_0_and_10_exact(ctx):
    pos, nrm = plane_cloud(400)
    nrm[::3] = -nrm[::3]
    got, ref, frac = _parity(ctx, pos, nrm, 0.12, 5)
    assert frac == 1.0
    assert np.array_equal(got[:, 22] > 0, ref["desc"][:, 22] > 0) and np.array_equal(got[:, 32] > 0, ref["desc"][:, 32] > 0)
    assert (got[:, 22] > 0).any() or (got[:, 32] > 0).any()                 # theta = +-pi: the sign of a zero decides


def test_facing_walls_pin_the_dot_form(ctx):
    """bins 0 and 10 of theta on two walls facing each other: every term of w . n_t is a signed zero, so the sign of the sum
    depends on the dot product's form (a0*b0 + a1*b1 + a2*b2 here, nalgebra's); a leading +0 would move every row"""
    pos, nrm = F.two_walls()
    got, ref, frac = _parity(ctx, pos, nrm, 0.115, 3)
    assert frac == 1.0
    for b in (22, 32):
        assert np.array_equal(got[:, b] > 0, ref["desc"][:, b] > 0)
        assert np.abs(got[:, b] - ref["desc"][:, b]).max() <= 1e-6
    alt = F.fpfh(pos, nrm, 0.115, 3, lead_zero=True)["desc"]
    assert (np.abs(alt - got).max(1) > 1e-3).all()                      # far outside the 1e-5 parity tolerance


def test_duplicates_are_skipped_pairs(ctx):
    rng = np.random.default_rng(13)
    pos = rng.random((3000, 3)).astype(np.float32)
    pos[1000:1300] = pos[0:300]
    nrm = _unit(rng.normal(size=(3000, 3)))
    _parity(ctx, pos, nrm, 0.12, 5, min_strict=0.99)


def test_pairs_along_the_normal(ctx):
    z = np.arange(40, dtype=np.float32)[:, None] * np.float32(0.01)
    pos = np.concatenate([np.zeros((40, 2), np.float32), z], 1)
    pos = np.concatenate([pos, pos + np.array([[0.02, 0, 0]], np.float32)])
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (80, 1))
    got = ctx.extract_fpfh_features_with_normals(_np(pos, nrm), 0.05, 3)
    ref = F.fpfh(pos, nrm, 0.05, 3)
    assert np.abs(got - ref["desc"]).max() <= 1e-5


def test_nan_and_non_unit_normals(ctx):
    rng = np.random.default_rng(14)
    pos = rng.random((4000, 3)).astype(np.float32)
    nrm = rng.normal(size=(4000, 3)).astype(np.float32) * np.float32(2.5)
    nrm[::97] = np.nan
    got, ref, _ = _parity(ctx, pos, nrm, 0.08, 8, min_strict=0.99)
    assert np.isfinite(got).all()


def test_non_finite_points_are_inert(ctx):
    rng = np.random.default_rng(15)
    pos = rng.random((3000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(3000, 3)))
    bad = np.arange(0, 3000, 101)
    pos[bad, bad % 3] = np.where(bad % 2 == 0, np.nan, np.inf)
    got, ref, _ = _parity(ctx, pos, nrm, 0.08, 8, min_strict=0.99)
    assert (got[bad] == 0).all()


def test_nan_radius_every_point_falls_back(ctx):
    rng = np.random.default_rng(16)
    pos = rng.random((3000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(3000, 3)))
    got, ref, _ = _parity(ctx, pos, nrm, float("nan"), 7, min_strict=0.99)
    assert (ref["nlist"] == 7).all()


def test_k_zero_is_radius_only(ctx):
    rng = np.random.default_rng(17)
    pos = rng.random((3000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(3000, 3)))
    got, ref, _ = _parity(ctx, pos, nrm, 0.05, 0, min_strict=0.99)
    assert (ref["nlist"] == 0).any() and (got[ref["nlist"] == 0] == 0).all()


def test_n_not_above_k(ctx):
    rng = np.random.default_rng(18)
    for n in (2, 5, 11):
        pos = rng.random((n, 3)).astype(np.float32)
        nrm = _unit(rng.normal(size=(n, 3)))
        _parity(ctx, pos, nrm, 0.01, 11)


def test_large_k_fallback(ctx):
    rng = np.random.default_rng(19)
    pos = rng.random((4000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(4000, 3)))
    # 200 neighbours of 200 neighbours each: 40 000 pairs touch a point, so the theta edge band flags more of them
    _parity(ctx, pos, nrm, 0.05, 200, rows=np.arange(0, 4000, 10), min_strict=0.85)


# ---- errors ----
def test_errors(ctx):
    one = _np(*plane_cloud(4))
    assert ctx.extract_fpfh_features(np.zeros((0, 3), np.float32)).shape == (0, 33)
    for r in (0.0, -1.0):
        with pytest.raises(tc.InvalidData, match="search_radius must be positive"):
            ctx.extract_fpfh_features_with_normals(one, r, 5)
        with pytest.raises(RuntimeError, match="search_radius must be positive"):
            threecrate.extract_fpfh_features(threecrate.PointCloud(one[:, :3].copy()), r, 5)
    with pytest.raises(tc.Unsupported):
        ctx.extract_fpfh_features_with_normals(one, 0.1, 2048)
    with pytest.raises(tc.InvalidData, match="k_neighbors must be at least 3"):
        ctx.extract_fpfh_features(one[:, :3].copy(), -1.0, 2)                 # the normals' check comes first
    with pytest.raises(RuntimeError, match="k_neighbors must be at least 3"):
        threecrate.extract_fpfh_features(threecrate.PointCloud(one[:, :3].copy()), 0.1, 2)


# ---- entry points ----
def test_host_and_device_entry_points_bit_identical(ctx):
    import torch
    rng = np.random.default_rng(20)
    pos = rng.random((30000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(30000, 3)))
    c6 = _np(pos, nrm)
    a = ctx.extract_fpfh_features_with_normals(c6, 0.03, 10)
    b = ctx.extract_fpfh_features_with_normals(c6, 0.03, 10)
    d = ctx.extract_fpfh_features_with_normals(torch.from_numpy(c6).to("cuda:0"), 0.03, 10)
    assert isinstance(d, torch.Tensor) and d.is_cuda
    assert np.array_equal(a, b) and np.array_equal(a, d.cpu().numpy())
    x = ctx.extract_fpfh_features(pos, 0.03, 10)
    y = ctx.extract_fpfh_features(torch.from_numpy(pos).to("cuda:0"), 0.03, 10)
    assert np.array_equal(x, y.cpu().numpy()) and np.array_equal(x, ctx.extract_fpfh_features(pos, 0.03, 10))
    # the xyz form is estimate_normals then the descriptors
    n6 = ctx.estimate_normals(pos, 10)
    assert np.array_equal(x, ctx.extract_fpfh_features_with_normals(n6, 0.03, 10))


def test_compat_defaults_equal_the_context_path(ctx):
    rng = np.random.default_rng(21)
    pos = rng.random((5000, 3)).astype(np.float32)
    got = threecrate.extract_fpfh_features(threecrate.PointCloud(pos))
    assert isinstance(got, np.ndarray) and got.shape == (5000, 33) and got.dtype == np.float32
    assert np.array_equal(got, tc.default_context().extract_fpfh_features(pos, 0.1, 10))
    assert np.array_equal(got, ctx.extract_fpfh_features(pos, 0.1, 10))


def test_one_million_points_sampled(ctx):
    pos = np.ascontiguousarray(synth.uniform_cloud(10**6), np.float32)
    rng = np.random.default_rng(22)
    nrm = _unit(rng.normal(size=(10**6, 3)))
    rows = rng.choice(10**6, 2000, replace=False)
    _parity(ctx, pos, nrm, 0.02, 10, rows=rows, min_strict=0.99)
