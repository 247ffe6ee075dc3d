"""Ground segmentation without a GPU: the checker (tests/ground_checker.py) on cases worked by hand, the case list of
tests/ground_cases.py proven clean (every status and every branch of the kernel reached, every parity case at a margin of 1e-6 or more),
the eigen routine of csrc/sym3_eigen.h as a stand-alone host program against numpy.linalg.eigh, the two exports that need no context,
the configuration checks as far as they come before the context, and the two arithmetic modes of the checker side by side."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import threecrate_amd as tc
from threecrate_amd import _lib, synth
from tests import ground_cases as GCASES
from tests import ground_checker as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-6


# ---- the checker, by hand ----
def _twelve():
    """12 points of one patch (one zone, one ring, one sector): ten on the plane z = -2 + 0.1 x, at x = 10 + i / 2, y = +-1; one 0.3 above
    it and one 2 above it.  Every sum is a short decimal: the plane and the labels can be written out"""
    pts = [[10.0 + 0.5 * i, 1.0 if i % 2 else -1.0, -2.0 + 0.1 * (10.0 + 0.5 * i)] for i in range(10)]
    pts += [[12.0, 0.0, -2.0 + 1.2 + 0.3], [12.0, 0.5, -2.0 + 1.2 + 2.0]]
    cfg = GC.default_config(0.75, zone_radii=[0.0, 40.0], num_rings=[1], num_sectors=[1], max_range=40.0, flatness_threshold=0.05)
    return np.array(pts, np.float32), cfg


def test_checker_on_a_twelve_point_patch_written_out():
    pts, cfg = _twelve()
    r = GC.segment(pts, cfg)
    # the lowest 12 (all: num_seed_points = 20 > 12) have mean z = (sum of -1 .. -0.55 step 0.05 = -7.75, + -0.5 + 1.2) / 12 = -0.5875; the
    # cutoff -0.0875 admits the ten plane points (z <= -0.55) and the point 0.3 above the plane (-0.5), not the one 2 above (1.2)
    # first plane: through eleven points; the second keeps the ten (the eleventh is 0.3 / sqrt(1.01) = 0.2985 off the ten's plane, and
    # more than 0.125 off the first plane, which it pulled up by little); the third sweep keeps the same ten: the early stop
    want = np.array([True] * 10 + [False, False])
    assert (r["labels"] == want).all()
    rec = r["patches"][0]
    assert (rec["count"], rec["n_inliers"], rec["status"]) == (12, 10, GC.GROUND)
    n = np.array([-0.1, 0.0, 1.0]) / np.sqrt(1.01)                  # the plane z = -2 + 0.1 x: normal (-0.1, 0, 1) / sqrt(1.01), d = 2 / sqrt(1.01)
    assert np.abs(rec["normal"] - n).max() < 1e-6 and abs(rec["d"] - 2.0 / np.sqrt(1.01)) < 1e-5
    assert abs(rec["mean_z"] - (-0.775)) < 1e-6 and rec["flatness"] < 1e-9
    assert r["iterations"][0] == 2 and r["early_stop"][0]
    assert abs(rec["normal"][2]) >= 0.707 and abs(rec["mean_z"] + 0.75) <= 1.0


def test_checker_statuses_on_the_twelve_points():
    pts, cfg = _twelve()
    status = lambda **over: GC.segment(pts, dict(cfg, **over))["patches"]["status"][0]
    assert status(min_points_per_patch=13) == GC.TOO_FEW_POINTS
    assert status(seed_selection_threshold=-10.0) == GC.TOO_FEW_SEEDS
    assert status(num_iterations=0) == GC.NO_ITERATION
    assert status(dist_threshold=1e-9, seed_selection_threshold=5.0) == GC.TOO_FEW_INLIERS
    assert status(uprightness_threshold=0.9999) == GC.NOT_UPRIGHT     # |n.z| = 1 / sqrt(1.01) = 0.995
    assert status(sensor_height=3.0) == GC.ELEVATION                   # |-0.775 + 3| > 1
    assert status(sensor_height=1.7) == GC.GROUND
    empty = GC.segment(np.zeros((0, 3), np.float32), cfg)
    assert len(empty["labels"]) == 0 and (empty["patches"]["status"] == GC.EMPTY).all() and len(empty["patches"]) == 1


def test_checker_bucketing_by_hand():
    cfg = GC.default_config(1.8)
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [1, -1e-3, 0], [2.0, 0, 0], [3, 0, 0], [79.9, 0, 0], [80, 0, 0], [81, 0, 0],
                    [np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]], np.float32)
    got = GC.bucket(pts, cfg)
    # zone 0: 2 rings of 1.35 m, 16 sectors of 22.5 degrees; zone 1 starts at patch 32 (4 rings of 32 sectors); zone 3 at 32 + 128 + 216
    assert got.tolist() == [0, 0, 4, 8, 12, 15, 16, 32, 376 + 3 * 32, 504, 504, 504, 504, 504]
    assert GC.patch_count(cfg) == 504


# ---- the case list is clean before any GPU sees it ----
@pytest.mark.parametrize("name", list(GCASES.CASES))
def test_every_parity_case_keeps_the_margin(name):
    e = GCASES.expected(name)
    print(f"{name}: margin {e['margin']:.3e} at {e['margin_at']}")
    assert e["margin"] >= MARGIN, (e["margin"], e["margin_at"])


def test_the_cases_reach_every_status_and_every_branch():
    seen, counts = set(), set()
    first_stop = all_run = False
    for name in GCASES.CASES:
        e, (_, cfg) = GCASES.expected(name), GCASES.case(name)
        fitted = e["patches"]["status"] >= GC.NOT_UPRIGHT
        seen |= set(int(s) for s in e["patches"]["status"])
        counts |= set(int(c) for c in e["patches"]["count"])
        first_stop |= bool((fitted & e["early_stop"] & (e["iterations"] == 1)).any())
        all_run |= bool((fitted & ~e["early_stop"] & (e["iterations"] == cfg["num_iterations"]) & (cfg["num_iterations"] >= 3)).any())
    assert seen == set(range(9)), seen
    assert first_stop and all_run
    K, W = GCASES.K_STAGE, GCASES.K_WAVE
    assert {9, 10, W - 1, W, W + 1, 255, 256, 257, K - 1, K, K + 1, 20000, 1, 2} <= counts
    assert (GCASES.expected("statuses")["patches"]["count"] == 15).any() and GCASES.case("statuses")[1]["num_seed_points"] == 20
    assert GC.patch_count(GCASES.case("max_patches")[1]) == 65536 == _lib.TC_GROUND_MAX_PATCHES and GC.patch_count(GCASES.too_many_patches()) == 65537
    assert (GCASES.expected("iterations_1")["iterations"].max(), GCASES.expected("iterations_0")["iterations"].max()) == (1, 0)
    # the kernel's thresholds are the ones the sizes were built around
    src = open(os.path.join(ROOT, "threecrate_amd", "csrc", "ground.hip")).read()
    assert f"kGroundStage = {K};" in src and f"kGroundWavePatch = {W};" in src


def test_the_reference_scenes_own_assertions():
    flat, scene = GCASES.expected("scene_flat"), GCASES.expected("scene")
    assert flat["labels"].mean() > 0.85
    pts = GCASES.case("scene")[0]
    g, ng = pts[scene["labels"]], pts[~scene["labels"]]
    assert len(g) > 0 and len(ng) > 0 and len(g) + len(ng) == len(pts)
    assert ng[:, 2].mean() > g[:, 2].mean() + 0.3
    k = GCASES.expected("kitti16")
    pts = GCASES.case("kitti16")[0]
    far = np.hypot(pts[:, 0], pts[:, 1]) > 19.0                      # the walls are 20 m out
    wall_patches = np.unique(k["patch_of"][far & (pts[:, 2] > -1.0)])
    assert len(wall_patches) and (k["patches"]["status"][wall_patches[k["patches"]["count"][wall_patches] >= 10]] == GC.NOT_UPRIGHT).all()
    assert (k["patches"]["status"] == GC.EMPTY).sum() > 100


def test_bucketing_edges_fall_where_they_were_built():
    pts, cfg = GCASES.case("bucket_edges")
    e = GCASES.expected("bucket_edges")
    r = np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64))
    out = e["patch_of"] == GC.patch_count(cfg)
    assert (out == ((r < 2.0) | (r > 25.0))).all()                   # zone_radii[0] > 0, max_range below the last radius
    assert out[(pts[:, 0] == 0) & (pts[:, 1] == 0)].all()
    theta = np.arctan2(pts[:, 1], pts[:, 0])
    last = (~out) & (theta < 0) & (theta > -0.02)
    assert last.any() and set(e["patch_of"][last] % 2) <= {1}         # the last sector of 4 or of 6: an odd number, also after the zone's base of 8
    assert not e["labels"][out].any()


def test_points_that_are_not_finite_change_nothing_else():
    pts, cfg = GCASES.case("data_edges")
    e = GCASES.expected("data_edges")
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() == 9 and not e["labels"][bad].any() and (e["patch_of"][bad] == 504).all()
    clean = GC.segment(pts[~bad], cfg)
    assert (clean["labels"] == e["labels"][~bad]).all() and clean["patches"].tobytes() == e["patches"].tobytes()


# ---- the eigen routine, as a host program ----
@pytest.fixture(scope="module")
def eigen_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("sym3")), "sym3_eigen_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "threecrate_amd", "csrc"),
                           os.path.join(ROOT, "tests", "abi", "sym3_eigen_host.cpp"), "-o", exe])
    return exe


def _case_matrices():
    """the covariance of every fitted patch's inliers, over all cases"""
    out = []
    for name in GCASES.CASES:
        pts, _ = GCASES.case(name)
        e = GCASES.expected(name)
        for pid in np.flatnonzero(e["patches"]["status"] == GC.GROUND):
            q = pts[(e["patch_of"] == pid) & e["labels"]].astype(np.float64)
            out.append(np.cov((q - q[0]).T, bias=True))
    return out


def test_eigen_routine_against_numpy(eigen_exe):
    rng = np.random.default_rng(0)
    mats = _case_matrices()
    n_case = len(mats)
    for _ in range(2000):
        a = rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-6, 6)
        mats.append((a + a.T) / 2)
    for _ in range(500):                                            # covariance-like: positive semi-definite, often nearly flat
        a = rng.normal(size=(3, 3)) * np.array([1.0, 1.0, 10.0 ** rng.uniform(-6, 0)])
        mats.append(a @ a.T)
    mats += [np.zeros((3, 3)), np.eye(3), np.diag([3.0, 1.0, 2.0]), np.diag([1.0, 1.0, 2.0]), np.ones((3, 3)), np.diag([0.0, 0.0, 5.0])]
    text = "\n".join(" ".join(repr(float(m[i, j])) for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))) for m in mats) + "\n"
    out = subprocess.run([eigen_exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(mats) and n_case > 300
    worst_w = worst_angle = 0.0
    for m, line in zip(mats, out):
        vals = line.split()
        sweeps, w, v = int(vals[0]), np.array(vals[1:4], np.float64), np.array(vals[4:], np.float64).reshape(3, 3)
        ew, ev = np.linalg.eigh(m)
        scale = max(np.abs(ew).max(), 1e-300)
        assert sweeps < 24 and (np.diff(w) >= 0).all()
        worst_w = max(worst_w, np.abs(w - ew).max() / scale)
        assert np.abs(w - ew).max() <= 1e-12 * scale, (m, w, ew)
        assert np.abs(np.linalg.norm(v, axis=1) - 1).max() < 1e-14
        assert np.abs(m @ v.T - v.T * w).max() <= 1e-13 * scale    # each returned pair is an eigenpair, whatever the gaps
        for k in range(3):
            gap = min(abs(ew[k] - ew[j]) for j in range(3) if j != k) / scale
            if gap > 1e-6:
                c = min(abs(float(v[k] @ ev[:, k])), 1.0)
                angle = np.arccos(c) if c < 0.999999 else np.sqrt(max(2.0 * (1.0 - c), 0.0))
                # 1 - cos is blind below 1e-8 in f64: the sine from the cross product instead
                angle = min(angle, np.linalg.norm(np.cross(v[k], ev[:, k])))
                worst_angle = max(worst_angle, angle)
                assert angle <= 1e-9, (m, k, angle)
    print(f"eigenvalues: worst relative difference {worst_w:.2e}; eigenvectors: worst angle {worst_angle:.2e}")


# ---- the exports that need no context ----
@pytest.fixture(scope="module")
def L():
    return _lib.load_companion("threecrate_hip_ground.h")


def test_config_default_and_patch_count(L):
    cfg = _lib.GroundConfigC()
    L.tc_ground_config_default(1.8, C.byref(cfg))
    L.tc_ground_config_default(1.8, None)
    ref = GC.default_config(1.8)
    assert cfg.n_zones == 4 and list(cfg.zone_radii)[:5] == [float(np.float32(v)) for v in ref["zone_radii"]] and list(cfg.zone_radii)[5:] == [0.0] * 4
    assert list(cfg.num_rings) == ref["num_rings"] + [0] * 4 and list(cfg.num_sectors) == ref["num_sectors"] + [0] * 4
    for name in ("sensor_height", "max_range", "seed_selection_threshold", "dist_threshold", "uprightness_threshold", "flatness_threshold", "elevation_threshold"):
        assert getattr(cfg, name) == float(np.float32(ref[name])), name
    assert (cfg.min_points_per_patch, cfg.num_seed_points, cfg.num_iterations) == (10, 20, 3)
    assert L.tc_ground_patch_count(C.byref(cfg)) == 504 == GC.patch_count(ref)
    assert L.tc_ground_patch_count(None) == 0
    for name in GCASES.CASES:
        c = GCASES.case(name)[1]
        assert L.tc_ground_patch_count(C.byref(tc.GpuContext.ground_config(**c))) == GC.patch_count(c), name
    assert L.tc_ground_patch_count(C.byref(tc.GpuContext.ground_config(**GCASES.too_many_patches()))) == 65537


def test_patch_count_is_zero_for_every_invalid_config(L):
    def count(**over):
        cfg = tc.GpuContext.ground_config(1.8)
        for k, v in over.items():
            if isinstance(v, tuple):
                getattr(cfg, k)[v[0]] = v[1]
            else:
                setattr(cfg, k, v)
        return L.tc_ground_patch_count(C.byref(cfg))
    assert count() == 504
    for bad in ({"n_zones": 0}, {"zone_radii": (2, 2.7)}, {"zone_radii": (1, float("nan"))}, {"dist_threshold": 0.0}, {"dist_threshold": float("nan")},
                {"num_seed_points": 0}, {"uprightness_threshold": 0.0}, {"uprightness_threshold": 1.5}, {"n_zones": 9}, {"num_rings": (3, 0)},
                {"num_sectors": (0, 0)}):
        assert count(**bad) == 0, bad
    assert count(n_zones=3) == 32 + 128 + 216 and count(uprightness_threshold=1.0) == 504


def test_a_null_context_comes_first(L):
    cfg = tc.GpuContext.ground_config(1.8)
    cfg.n_zones = 0
    labels, ng = np.full(4, 7, np.uint8), C.c_size_t(7)
    pts = np.zeros((4, 3), np.float32)
    for fn in (L.tc_segment_ground, L.tc_segment_ground_device):
        assert fn(None, pts.ctypes.data, 4, C.byref(cfg), labels.ctypes.data, None, None, None, C.byref(ng)) == _lib.TC_INVALID_DATA
    assert (labels == 7).all() and ng.value == 7


def test_python_config_lengths_answer_with_the_references_messages():
    with pytest.raises(tc.InvalidData, match="num_rings_per_zone must be non-empty"):
        tc.GpuContext.ground_config(1.8, zone_radii=[0.0], num_rings=[], num_sectors=[])
    with pytest.raises(tc.InvalidData, match=r"zone_radii.len\(\) must equal"):
        tc.GpuContext.ground_config(1.8, zone_radii=[0.0, 10.0], num_rings=[2, 2], num_sectors=[8, 8])
    with pytest.raises(tc.InvalidData, match=r"num_sectors_per_zone.len\(\) must equal"):
        tc.GpuContext.ground_config(1.8, zone_radii=[0.0, 10.0, 20.0], num_rings=[2, 2], num_sectors=[8])
    import threecrate_amd.compat as compat
    c = compat.PatchworkConfig()
    assert (c.sensor_height, c.zone_radii, c.num_rings_per_zone, c.num_sectors_per_zone) == (1.723, [0.0, 2.7, 12.3625, 22.025, 80.0], [2, 4, 4, 4], [16, 32, 54, 32])
    assert bytes(c._c()) == bytes(tc.GpuContext.ground_config(1.723))


# ---- what the deviation costs ----
@pytest.mark.parametrize("name", ["scene", "kitti16"])
def test_f32_sums_in_index_order_against_the_f64_contract(name):
    a, b = GCASES.expected(name), GCASES.expected(name, "f32")
    differ = float((a["labels"] != b["labels"]).mean())
    print(f"{name}: {100 * differ:.4f} % of the labels differ between the reference's f32 sums and the f64 contract")
    assert (a["patches"]["status"] == b["patches"]["status"]).all()
    assert differ <= 0.01
