"""FPFH descriptors, device-free: the checker against a literal per-point restatement of features.rs:81-259, and the binding
surfaces (header, ctypes exports, Rust shim, compat module)."""
import inspect
import math
import os
import re

import numpy as np

from tests import fpfh_checker as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bin(v, lo, hi):
    t = (v - lo) / (hi - lo) * f32(11)
    if math.isnan(t) or t <= 0:            # Rust's `as usize` saturates: NaN and negative -> 0
        return 0
    return min(int(min(t, f32(11))), 10)


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _pair(ps, ns, pt, nt):
    with np.errstate(all="ignore"):
        delta = (pt[0] - ps[0], pt[1] - ps[1], pt[2] - ps[2])
        dist = np.sqrt(f32(0) + _dot(delta, delta))
        if dist < 1e-10:
            return None
        d = (delta[0] / dist, delta[1] / dist, delta[2] / dist)
        v = _cross(ns, d)
        vm = np.sqrt(f32(0) + _dot(v, v))
        if vm < 1e-10:
            return None
        v = (v[0] / vm, v[1] / vm, v[2] / vm)
        w = _cross(ns, v)
        return _dot(v, nt), _dot(ns, d), np.arctan2(_dot(w, nt), _dot(ns, nt))


def reference(pos, nrm, radius, k):
    """features.rs:131-259, one point at a time, brute-force f32 neighbour search"""
    pos = [tuple(f32(c) for c in p) for p in np.asarray(pos, np.float32)]
    nrm = [tuple(f32(c) for c in p) for p in np.asarray(nrm, np.float32)]
    n = len(pos)
    r2 = f32(radius) * f32(radius)
    with np.errstate(all="ignore"):
        d2 = [[_dot(*(2 * [(pos[j][0] - pos[i][0], pos[j][1] - pos[i][1], pos[j][2] - pos[i][2])])) for j in range(n)] for i in range(n)]
    nbrs = []
    for i in range(n):
        within = sorted([j for j in range(n) if d2[i][j] <= r2 and j != i], key=lambda j: (d2[i][j], j))
        if len(within) >= k:
            nbrs.append(within)
            continue
        near = sorted(range(n), key=lambda j: (d2[i][j], j))[: k + 1]
        nbrs.append([j for j in near if j != i][:k])
    spfh = []
    for i in range(n):
        h = [f32(0)] * 33
        count = 0
        for t in nbrs[i]:
            f = _pair(pos[i], nrm[i], pos[t], nrm[t])
            if f is None:
                continue
            a, p, th = f
            for off, b in ((0, _bin(a, f32(-1), f32(1))), (11, _bin(p, f32(-1), f32(1))), (22, _bin(th, -F.PI32, F.PI32))):
                h[off + b] = h[off + b] + f32(1)
            count += 1
        if count:
            scale = f32(1) / f32(count)
            h = [x * scale for x in h]
        spfh.append(h)
    out = np.zeros((n, 33), np.float32)
    for i in range(n):
        desc = list(spfh[i])
        if nbrs[i]:
            ws, acc = f32(0), [f32(0)] * 33
            for j in nbrs[i]:
                dl = (pos[j][0] - pos[i][0], pos[j][1] - pos[i][1], pos[j][2] - pos[i][2])
                dist = np.sqrt(f32(0) + _dot(dl, dl))
                if dist < 1e-10:
                    continue
                w = f32(1) / dist
                ws = ws + w
                acc = [acc[b] + w * spfh[j][b] for b in range(33)]
            if ws > 0:
                iw = f32(1) / ws
                desc = [desc[b] + iw * acc[b] for b in range(33)]
                for part in range(3):
                    s = f32(0)
                    for b in range(11 * part, 11 * part + 11):
                        s = s + desc[b]
                    if s > 0:
                        for b in range(11 * part, 11 * part + 11):
                            desc[b] = desc[b] / s
        out[i] = desc
    return out


def _same(pos, nrm, radius, k):
    ref = reference(pos, nrm, radius, k)
    got = F.fpfh(pos, nrm, radius, k)
    assert np.array_equal(got["desc"], ref), np.abs(got["desc"] - ref).max()     # same operations, same order: bit-equal
    return got


def _unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def test_checker_equals_reference_on_random_clouds_with_fallback():
    rng = np.random.default_rng(1)
    pos = rng.random((120, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(120, 3)))
    got = _same(pos, nrm, 0.25, 8)
    assert (got["nlist"] == 8).any() and (got["nlist"] > 8).any()       # both branches of find_neighbors
    _same(pos, nrm, 0.3, 10)
    _same(pos, nrm, 0.2, 0)


def test_checker_duplicates_nan_and_non_unit_normals():
    rng = np.random.default_rng(2)
    pos = rng.random((60, 3)).astype(np.float32)
    pos[10] = pos[11] = pos[12]                                          # duplicates: pairs skipped at dist < 1e-10
    nrm = rng.normal(size=(60, 3)).astype(np.float32) * 3.0              # non-unit normals
    nrm[5] = np.nan                                                      # NaN features -> bin 0
    got = _same(pos, nrm, 0.35, 5)
    assert got["desc"][5, 0] > 0 and np.isfinite(got["desc"]).all()


def test_checker_flipped_normal_plane_signed_zero_bins():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * f32(0.1)
    pos = np.concatenate([g, np.zeros((len(g), 1), np.float32)], 1)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (len(g), 1))
    nrm[::2] = -nrm[::2]                                                 # flipped neighbours: theta = atan2(+-0, -1) = +-pi
    got = _same(pos, nrm, 0.25, 4)
    theta = got["desc"][:, 22:]
    assert (theta[:, 0] > 0).any() or (theta[:, 10] > 0).any()


def test_dot_form_pin_on_facing_walls():
    """The pinned assumption: w . n_t = a0*b0 + a1*b1 + a2*b2, no leading +0.  Here every term of w . n_t is -0, so the sum is
    -0 and theta = atan2(-0, -1) = -pi (bin 0); summed from +0 it would be +0 and +pi (bin 10)."""
    pos, nrm = F.two_walls()
    ps, ns, pt, nt = pos[[0]], nrm[[0]], pos[[37]], nrm[[37]]
    _, _, _, th, _ = F.pair_features(ps, ns, pt, nt)
    assert float(th[0]) == -float(F.PI32) and np.signbit(th[0])
    assert F.pair_bins(ps, ns, pt, nt)[1][0, 2] == 22 + 0
    assert F.pair_bins(ps, ns, pt, nt, lead_zero=True)[1][0, 2] == 22 + 10
    assert _pair(ps[0], ns[0], pt[0], nt[0])[2] == -F.PI32            # the literal restatement agrees
    got = _same(pos, nrm, 0.115, 3)
    assert got["strict"].all()
    alt = F.fpfh(pos, nrm, 0.115, 3, lead_zero=True)["desc"]
    assert (np.abs(alt - got["desc"]).max(1) > 1e-3).all()             # every row tells the two forms apart (tolerance 1e-5)


def test_checker_pairs_along_the_normal_are_skipped():
    pos = np.array([[0, 0, 0], [0, 0, 0.1], [0, 0, 0.2], [0.05, 0, 0]], np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (4, 1))
    valid, _, _ = F.pair_bins(pos[[0, 0]], nrm[[0, 0]], pos[[1, 3]], nrm[[1, 3]])
    assert valid.tolist() == [False, True]
    _same(pos, nrm, 0.3, 2)


def test_checker_nan_radius_and_small_clouds():
    rng = np.random.default_rng(3)
    pos = rng.random((30, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(30, 3)))
    got = _same(pos, nrm, float("nan"), 4)                              # every point falls back
    assert (got["nlist"] == 4).all()
    _same(pos[:5], nrm[:5], 0.01, 10)                                    # n <= k: n - 1 neighbours each
    assert (F.fpfh(pos[:5], nrm[:5], 0.01, 10)["nlist"] == 4).all()


def test_checker_subset_rows_equal_full_run():
    rng = np.random.default_rng(4)
    pos = rng.random((3000, 3)).astype(np.float32)
    nrm = _unit(rng.normal(size=(3000, 3)))
    full = F.fpfh(pos, nrm, 0.06, 8)
    rows = rng.choice(3000, 200, replace=False)
    sub = F.fpfh(pos, nrm, 0.06, 8, rows)
    assert np.array_equal(sub["desc"], full["desc"][rows])
    assert np.array_equal(sub["strict"], full["strict"][rows])
    assert full["strict"].mean() > 0.9


def test_header_declares_the_fpfh_entry_points():
    hdr = open(os.path.join(ROOT, "include", "threecrate_hip.h")).read()
    assert "#define TC_FPFH_DIM 33" in hdr
    names = {"tc_extract_fpfh_features_with_normals", "tc_extract_fpfh_features_with_normals_device", "tc_extract_fpfh_features",
             "tc_extract_fpfh_features_device"}
    for nm in names:
        assert re.search(r"tc_status %s\(" % nm, hdr), nm
    from threecrate_amd import _lib
    assert names <= set(_lib.EXPORTS)


def test_rust_shim_has_the_fpfh_functions_and_config():
    src = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "lib.rs")).read()
    for fn in ["extract_fpfh_features_with_normals", "extract_fpfh_features"]:
        assert re.search(r"pub fn %s\s*\(" % fn, src), fn
    assert "pub const FPFH_DIM: usize = 33;" in src
    m = re.search(r"pub struct FpfhConfig\s*\{([^}]*)\}", src)
    assert m and [f.split(":")[0].replace("pub", "").strip() for f in m.group(1).split(",") if f.strip()] == ["search_radius", "k_neighbors"]
    assert "search_radius: 0.1, k_neighbors: 10" in src
    assert "Result<Vec<[f32; FPFH_DIM]>>" in src and "Result<Vec<Vec<f32>>>" in src
    ffi = open(os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src", "ffi.rs")).read()
    for nm in ["tc_extract_fpfh_features_with_normals", "tc_extract_fpfh_features_with_normals_device", "tc_extract_fpfh_features",
               "tc_extract_fpfh_features_device"]:
        assert "pub fn %s(" % nm in ffi, nm


def test_compat_has_extract_fpfh_features_with_the_wheels_signature():
    import threecrate_amd.compat as threecrate
    assert "extract_fpfh_features" in threecrate.__all__
    sig = inspect.signature(threecrate.extract_fpfh_features)
    assert [(p.name, p.default) for p in sig.parameters.values()] == [
        ("cloud", inspect.Parameter.empty), ("search_radius", 0.1), ("k_neighbors", 10)]
    import threecrate_amd.api as api
    for nm in ["extract_fpfh_features", "extract_fpfh_features_with_normals"]:
        assert callable(getattr(api, nm)) and callable(getattr(api.GpuContext, nm))
