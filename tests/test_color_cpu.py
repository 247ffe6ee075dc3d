"""Colorization without a GPU: the checker (tests/color_checker.py) on the reference's unit tests, the preconditions of every input of
tests/test_gpu_color.py, the calls that need no device, the compat surface, the Rust facade's names, and the mutant table -- every rule
of color_checker.RULES replaced in turn must be told apart by a named case of tests/color_cases.py, which the GPU file runs as well."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from threecrate_amd import _lib
import threecrate_amd.compat as threecrate
from tests import abi_text as T
from tests import color_cases as CC
from tests import color_checker as K

F = np.float32


def check(case, rules=()):
    return K.colorize(case["xyz"], case["sources"], rules=rules, **case["cfg"])


# ---- the checker on the reference's own unit tests ----
@pytest.mark.parametrize("name", [n for n in CC.CASES if n.startswith("reference_")])
def test_checker_passes_the_reference_unit_tests(name):
    case = CC.CASES[name]
    rgb, index, count = check(case)
    want_rgb, want_count = case["want"]
    assert rgb.tolist() == [want_rgb] and count == want_count and index.tolist() == [0 if want_count else -1]


def test_there_are_the_five_unit_tests_and_the_buffer_error():
    assert len([n for n in CC.CASES if n.startswith("reference_")]) == 5
    with pytest.raises(RuntimeError, match=r"RgbImageView: buffer too small — expected 48 bytes for 4×4 RGB image, got 10"):
        threecrate.colorize_point_cloud(threecrate.PointCloud(np.zeros((1, 3), F)), bytes(10), 4, 4, 2.0, 2.0, 1.5, 1.5, np.eye(4))


def test_roundf_is_half_away_and_leaves_large_values_alone():
    x = F([0.5, -0.5, 1.5, 2.5, -2.5, 0.49999997, -0.25, 2 ** 23 + 1, -(2 ** 23) - 1, 2 ** 24, np.inf, -np.inf])
    want = F([1, -1, 2, 3, -3, 0, -0.0, 2 ** 23 + 1, -(2 ** 23) - 1, 2 ** 24, np.inf, -np.inf])
    got = K.roundf(x)
    assert got.dtype == F and got.tobytes() == want.tobytes()
    assert np.isnan(K.roundf(F([np.nan])))[0]
    assert K.roundf(F([0.5, 2.5]), half_even=True).tolist() == [0, 2]


# ---- the preconditions of every GPU input ----
@pytest.mark.parametrize("name", [n for n, c in CC.CASES.items() if "uv" in c])
def test_every_constructed_pixel_coordinate_is_the_intended_float(name):
    case = CC.CASES[name]
    u, v = case["uv"]
    _, k, m = case["sources"][0][:3]
    cz, gu, gv = K.project(case["xyz"], k, m)
    assert np.all(cz == 1) and gu.dtype == F
    assert gu.tobytes() == np.asarray(u, F).tobytes() and gv.tobytes() == np.asarray(v, F).tobytes()


def test_edges_reach_what_they_are_for():
    assert sorted({tuple(c["sources"][0][0].shape[:2]) for n, c in CC.CASES.items() if n.startswith("edges_")}) == [(1, 1), (1, 5), (2, 2), (4, 4), (5, 1), (5, 7)]
    assert CC.CASES["edges_7x5_bilinear"]["sources"][0][0].strides[0] == 21         # the odd row stride
    for name, case in CC.CASES.items():
        if not name.startswith("edges_"):
            continue
        h, w = case["sources"][0][0].shape[:2]
        u, v = case["uv"]
        assert u.min() == -1.5 and u.max() == w + 0.5 and v.min() == -1.5 and v.max() == h + 0.5
        assert {-0.5, 0.5, w - 0.5}.issubset(set(u.tolist())) and len(set(np.diff(np.unique(u)).tolist())) == 1
        rgb, index, count = check(case)
        at = lambda uu, vv: index[(u == uu) & (v == vv)][0]
        assert at(-0.5, 0) == -1 and at(w - 0.5, 0) == -1 and at(-0.25, 0) == 0 and at(w - 0.75, h - 0.75) == 0     # -0.5 -> -1, w - 0.5 -> w: outside
        assert 0 < count < len(index)
    # the 1 x 1 image: bilinear never applies and gives what nearest gives
    a, b = check(CC.CASES["edges_1x1_bilinear"]), check(CC.CASES["edges_1x1_nearest"])
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2] > 0
    # left of 0 and at w - 1 the bilinear neighbourhood clips, falls back to nearest and still colours
    case = CC.CASES["edges_4x4_bilinear"]
    u, v = case["uv"]
    rgb, index, _ = check(case)
    img = case["sources"][0][0]
    for uu, px in ((-0.25, 0), (3.25, 3)):
        sel = (u == uu) & (v == 1.0)
        assert index[sel][0] == 0 and rgb[sel][0].tolist() == img[1, px].tolist()


def test_the_tie_inputs_are_what_the_search_finds():
    """HALF: the three-operation value is exactly k + 0.5.  FUSED: it is k + 0.5 while fma(b - a, t, a), exact in float64, lies below --
    they round to different bytes.  The search (a = 1, b < 20, three floats either side of the exact t) finds the table's a = 1 rows."""
    one = lambda a, b, t, fused: float(K.lerp(F([a]), F([b]), F([t]), fused)[0])
    for a, b, t in CC.TIES_HALF:
        val = one(a, b, t, False)
        assert val - np.floor(val) == 0.5 and K.roundf(F([val]))[0] == np.floor(val) + 1
    for a, b, t in CC.TIES_FUSED:
        val, fused = one(a, b, t, False), one(a, b, t, True)
        assert val - np.floor(val) == 0.5 and fused < val and K.roundf(F([val]))[0] == K.roundf(F([fused]))[0] + 1
    found = set()
    for b in range(2, 20):
        for k in range(1, b):
            t = F((k + 0.5 - 1) / (b - 1))
            cands = [t]
            for d in (F(0), F(1)):
                c = t
                for _ in range(3):
                    c = np.nextafter(c, d)
                    cands.append(c)
            for cand in cands:
                if 0 <= cand < 1 and K.roundf(F([one(1, b, cand, False)]))[0] != K.roundf(F([one(1, b, cand, True)]))[0]:
                    found.add((1, b, float(cand)))
    assert {row for row in CC.TIES_FUSED if row[0] == 1} <= found


def test_depth_gate_inputs_sit_where_they_should():
    case = CC.CASES["depth_gate_min_depth_bilinear"]
    z = case["xyz"][:, 2]
    assert z[0] < 1 == z[1] < z[2] and z[1] - z[0] == 2.0 ** -24 and z[2] - z[1] == 2.0 ** -23 and z[3] == -1
    assert check(case)[1].tolist() == [-1, 0, 0, -1]
    case = CC.CASES["depth_gate_tolerance_nearest"]
    d = case["sources"][0][3]
    gap = np.abs(F(1) - d)
    tol = F(case["cfg"]["depth_tolerance"])
    assert gap[0, 1] == tol == gap[0, 2] and gap[0, 3] > tol and gap[1, 0] > tol and gap[2, 2] < tol and gap[2, 3] < tol
    index = check(case)[1]
    #               row 0: 0, lo, hi, below      row 1: above, 1, -1, NaN     row 2: inf, -inf, inside, inside   row 3    (0.75, 0.75) (1.75, 0.75)
    assert index.tolist() == [-1, 0, 0, -1] + [-1, 0, -1, -1] + [-1, -1, 0, 0] + [0, 0, 0, 0] + [0, -1]
    assert check(CC.CASES["depth_gate_tolerance_bilinear"])[1].tolist() == index.tolist()


def test_sources_cases_are_what_they_say():
    for k in (2, 3, 4, 5):
        assert set(check(CC.CASES[f"sources_first_wins_{k}"])[1].tolist()) == {0}
        assert set(check(CC.CASES[f"sources_only_last_sees_{k}"])[1].tolist()) == {k - 1}
        rgb, index, count = check(CC.CASES[f"sources_nobody_sees_{k}"])
        assert count == 0 and set(index.tolist()) == {-1} and set(map(tuple, rgb.tolist())) == {CC.GREY}
    index = check(CC.CASES["sources_default_pixel_falls_through"])[1].reshape(4, 4)
    assert np.all(index[:, :2] == 1) and np.all(index[:, 2:] == 0)
    assert len(CC.CASES["sources_max"]["sources"]) == _lib.TC_COLOR_MAX_SOURCES == 64
    assert check(CC.CASES["sources_max"])[1].tolist() == np.repeat(np.arange(64), 16).tolist()


def test_bad_points_and_blocks():
    for name in ("bad_points_bilinear", "bad_points_nearest"):
        case = CC.CASES[name]
        n = len(case["xyz"])
        bad = ~np.isfinite(case["xyz"]).all(axis=1)
        assert np.nonzero(bad)[0].tolist() == [0, n // 2, n - 1]
        index = check(case)[1]
        assert np.all(index[bad] == -1) and np.all(index[~bad] == 0)
    case = CC.CASES["bad_points_matrix_overflow"]
    assert all(np.isfinite(np.asarray(s[2])).all() for s in case["sources"])
    with np.errstate(all="ignore"):
        assert np.isnan(K.project(case["xyz"], *case["sources"][0][1:3])[0]).all() and np.isinf(K.project(case["xyz"], *case["sources"][1][1:3])[1]).all()
    assert check(case)[1].tolist() == [2, 2, 2]
    assert CC.SLICES * 256 + 1 in CC.BLOCK_SIZES and CC.SLICES == 16
    assert re.search(r"constexpr int kColorSlices = 16;", open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "tc_internal.h")).read())
    for n in CC.BLOCK_SIZES:
        count = check(CC.CASES[f"blocks_{n}"])[2]
        assert (count == 1) if n == 1 else 0 < count < n


def test_no_case_is_large():
    assert max(len(c["xyz"]) for c in CC.CASES.values()) == CC.SLICES * 256 + 1


# ---- the calls that need no device ----
def _one_source():
    img = np.zeros((1, 1, 3), np.uint8)
    src = _lib.ColorSourceC(img.ctypes.data, None, _lib.CameraIntrinsicsC(1, 1, 0, 0, 1, 1), (C.c_float * 12)(*CC.IDENTITY))
    return img, src


def test_a_null_context_is_invalid_data_whatever_else_is_wrong_and_writes_nothing():
    """check 1 of the header comes first: without a context there is no later answer (TC_UNSUPPORTED for 65 sources, ...) and no output"""
    L = _lib.load_companion("threecrate_hip_color.h")
    cfg = _lib.ColorizeConfigC()
    L.tc_colorize_config_default(C.byref(cfg))
    L.tc_colorize_config_default(None)
    assert (list(cfg.default_color), cfg.interpolation, cfg.min_depth, cfg.depth_tolerance) == ([128, 128, 128], 1, F(1e-4), F(0.05))
    img, src = _one_source()
    xyz, rgb, index, count = np.zeros((1, 3), F), np.full((1, 3), 7, np.uint8), np.full(1, 7, np.int32), C.c_size_t(7)
    many = (_lib.ColorSourceC * 65)(*[src] * 65)
    bad = _lib.ColorizeConfigC((C.c_uint8 * 3)(1, 2, 3), 2, float("nan"), -1.0)
    for fn in (L.tc_colorize, L.tc_colorize_device):
        for args in ((xyz.ctypes.data, 1, C.pointer(src), 1, C.byref(cfg)), (None, 1, None, 0, None), (xyz.ctypes.data, 1, many, 65, C.byref(cfg)),
                     (xyz.ctypes.data, 1, C.pointer(src), 1, C.byref(bad)), (None, 0, C.pointer(src), 1, C.byref(cfg)),
                     (xyz.ctypes.data, 2 ** 32, C.pointer(src), 1, C.byref(cfg))):
            assert fn(None, *args, rgb.ctypes.data, index.ctypes.data, C.byref(count)) == _lib.TC_INVALID_DATA
        assert fn(None, xyz.ctypes.data, 1, C.pointer(src), 1, C.byref(cfg), None, None, None) == _lib.TC_INVALID_DATA
    assert rgb.tolist() == [[7, 7, 7]] and index.tolist() == [7] and count.value == 7


def test_the_header_states_the_checks_in_the_order_the_entry_points_make_them():
    """the order itself needs a context (tests/test_gpu_color.py runs it); here: the text of color_check() follows the header's list"""
    src = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "color.hip")).read()
    body = src[src.index("static tc_status color_check("):src.index('extern "C" {')]
    marks = ["if (!ctx)", "!xyz && n > 0", "!sources)", "!cfg)", "rgb is NULL", "all NULL", "n_sources == 0", "n_sources > TC_COLOR_MAX_SOURCES",
             "interpolation > TC_COLOR_BILINEAR", "isfinite(cfg->min_depth)", "is not finite", "is zero", "above 65536", "check_point_count", "n == 0"]
    at = [body.index(m) for m in marks]
    assert at == sorted(at)
    header = open(os.path.join(T.ROOT, "include", "threecrate_hip_color.h")).read()
    assert "A PIXEL OF THE DEFAULT COLOUR COLOURS NOTHING" in header and "Deviations from colorization.rs" in header


# ---- compat ----
def test_colored_point_cloud_has_the_wheels_checks_and_messages():
    p, c = np.zeros((4, 3)), np.arange(12, dtype=np.uint8).reshape(4, 3)
    cloud = threecrate.ColoredPointCloud.from_numpy(p, c)
    assert len(cloud) == 4 and not cloud.is_empty and repr(cloud) == "ColoredPointCloud(4 points)"
    assert cloud.positions().dtype == F and cloud.positions().shape == (4, 3) and cloud.colors().dtype == np.uint8 and np.array_equal(cloud.colors(), c)
    assert threecrate.ColoredPointCloud().is_empty and repr(threecrate.ColoredPointCloud()) == "ColoredPointCloud(0 points)"
    with pytest.raises(ValueError, match=r"colors must be a \(N, 3\) uint8 numpy array"):
        threecrate.ColoredPointCloud.from_numpy(p, c.astype(np.float32))
    with pytest.raises(ValueError, match=r"colors must have shape \(N, 3\), got \[4, 2\]"):
        threecrate.ColoredPointCloud.from_numpy(p, c[:, :2])
    with pytest.raises(ValueError, match=r"positions and colors must have the same length \(4 vs 3\)"):
        threecrate.ColoredPointCloud.from_numpy(p, c[:3])
    with pytest.raises(ValueError, match=r"must have shape \(N, 3\)"):
        threecrate.ColoredPointCloud.from_numpy(np.zeros((4, 2)), c)


def test_colorize_point_cloud_has_the_wheels_signature():
    assert list(inspect.signature(threecrate.colorize_point_cloud).parameters) == ["cloud", "image_data", "width", "height", "fx", "fy", "cx", "cy",
                                                                                   "world_to_camera"]
    assert {"ColoredPointCloud", "colorize_point_cloud"} <= set(threecrate.__all__)
    cloud = threecrate.PointCloud(np.zeros((1, 3), F))
    with pytest.raises(ValueError, match="4×4"):
        threecrate.colorize_point_cloud(cloud, bytes(48), 4, 4, 2.0, 2.0, 1.5, 1.5, np.eye(3))
    from threecrate_amd import api
    want = ["self", "xyz", "sources", "default_color", "interpolation", "min_depth", "depth_tolerance", "return_index", "count"]
    sig = inspect.signature(api.GpuContext.colorize)
    assert list(sig.parameters)[:len(want)] == want
    assert [sig.parameters[k].default for k in want[3:]] == [(128, 128, 128), "bilinear", 1e-4, 0.05, False, True]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want[3:])


# ---- the Rust facade ----
def test_the_rust_facade_has_the_references_names():
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    mod = lib_rs[lib_rs.index("pub mod colorization {"):]
    for decl in ("pub struct CameraIntrinsics", "pub struct RgbImageView<'a>", "pub fn new(data: &'a [u8], width: u32, height: u32) -> Result<Self>",
                 "pub enum InterpolationMode", "pub struct ColorizationConfig", "impl Default for ColorizationConfig", "pub struct ColorizationResult",
                 "pub fn colorize_point_cloud(", "pub fn colorize_from_images("):
        assert decl in mod, decl
    assert "default_color: [128, 128, 128]" in mod and "min_depth: 1e-4" in mod and "#[default]\n        Bilinear" in mod
    assert "RgbImageView: buffer too small — expected {} bytes for {}×{} RGB image, got {}" in mod
    assert "colorize_from_images: sources slice must not be empty" in mod


# ---- the mutants ----
INVISIBLE = {}      # rule -> why no case can show it.  Empty: every mutant below is told apart


@pytest.mark.parametrize("rule", sorted(K.RULES))
def test_every_mutant_is_told_apart_by_a_named_case(rule):
    assert (rule in CC.TELLS) != (rule in INVISIBLE)
    for name in CC.TELLS.get(rule, ()):
        case = CC.CASES[name]
        good, bad = check(case), check(case, rules={rule})
        same = good[0].tobytes() == bad[0].tobytes() and good[1].tobytes() == bad[1].tobytes() and good[2] == bad[2]
        assert not same, (rule, name)


def test_the_mutant_table_is_the_issues():
    assert sorted(K.RULES) == sorted(CC.TELLS) and len(K.RULES) == 12 and not INVISIBLE
    assert all(name in CC.CASES for names in CC.TELLS.values() for name in names)
