"""The CPU twin of tests/test_gpu_poisson.py: the case table of tests/poisson_cases.py proved on the checker alone (no GPU).  It measures
what the device's budgets are derived from and asserts that the table's recorded numbers are those measurements; it shows that the f64
checker's sphere meshes are closed, of genus 0 and near the sphere; and it shows every mutant of the checker on a named case (or lists it
as invisible)."""
import numpy as np
import pytest

from tests import mc_checker as MC
from tests import poisson_cases as CS
from tests import poisson_checker as PC

F = np.float32
MEASURED_CASES = [n for n in CS.names() if n != "sphere_d6"]


def mesh_of(res):
    N, h = res["N"], float(res["h"])
    v, _, f = MC.marching_cubes(np.asarray(res["chi"], F), (N, N, N), (h, h, h), tuple(float(o) for o in res["origin"]), F(res["iso_value"]), normals=False,
                                weld=True, layout="x_fastest")
    return v, f


def test_the_table_has_every_family_and_every_case_passes_the_checks():
    families = {CS.case(n)["family"] for n in CS.names()}
    assert families == {"sphere", "sphere6", "faces", "small", "blocks", "dense_node", "duplicates", "plane_patch", "shifted"}
    assert set(CS.MEASURED) == set(MEASURED_CASES)
    for n in CS.names():
        c = CS.case(n)
        assert PC.check(c["points"], c["normals"], c["cfg"]) is None, n
        assert c["points"].dtype == F and c["normals"].dtype == F
    assert [len(CS.case(n)["points"]) for n in CS.names("blocks")] == [255, 256, 257, 513, 4097]
    assert [len(CS.case(n)["points"]) for n in CS.names("small")] == [10, 11]
    assert len(CS.depth8()["points"]) == 2000 and CS.depth8()["cfg"]["max_iterations"] == 3


def test_bad_inputs_are_what_the_checker_rejects():
    words = {"nan_coordinate": "not finite", "normal_0.0": "Invalid normal", "normal_0.85": "Invalid normal", "normal_1.15": "Invalid normal",
             "identical_points": "no extent", "nine_points": "too small", "depth_1": "depth", "depth_9": "depth", "scale_0.5": "scale"}
    for name, (p, q, cfg, ok) in CS.bad_inputs().items():
        got = PC.check(p, q, cfg)
        assert (got is None) == ok, (name, got)
        if not ok:
            assert words[name] in got, (name, got)
    assert PC.check(np.zeros((0, 3), F), np.zeros((0, 3), F), PC.config()) == "Point cloud is empty"


@pytest.mark.parametrize("name", MEASURED_CASES)
def test_the_recorded_budgets_are_the_checkers_own_distances(name):
    ex, f64 = CS.expected(name, "exact"), CS.expected(name, "f64")
    chi_d = PC.rel_max(ex["chi"], f64["chi"])
    iso_d = abs(float(ex["iso_value"]) - f64["iso_value"]) / np.abs(f64["chi"]).max()
    rec = CS.MEASURED[name]
    print(name, "chi", chi_d, "iso", iso_d, "iterations", ex["iterations"], "rel", ex["rel_residual"])
    assert ex["iterations"] == rec[2] and chi_d == pytest.approx(rec[0], rel=0.05) and iso_d == pytest.approx(rec[1], rel=0.05, abs=1e-12)
    assert 0 < ex["iterations"] < CS.case(name)["cfg"]["max_iterations"] and ex["occupied_nodes"] > 0


def test_at_most_a_tenth_of_the_cases_stop_near_the_tolerance():
    near = [n for n in MEASURED_CASES if near_tolerance(n)]
    print("near the tolerance:", near)
    assert len(near) <= len(MEASURED_CASES) // 10


def near_tolerance(name):
    """the exact checker's residual at the stop lies within 10 % of the tolerance: the device may stop one iteration apart"""
    tol = CS.case(name)["cfg"]["tolerance"]
    return abs(CS.expected(name)["rel_residual"] - tol) <= 0.1 * tol


def test_faces_land_where_intended():
    for n in CS.names("faces"):
        c, e = CS.case(n), CS.expected(n)
        N = e["N"]
        assert float(e["h"]) == 1.0 and (e["origin"] == 0).all()
        p = c["points"]
        assert (e["cell"] <= N - 2).all() and (e["cell"] >= 0).all()
        top = (p == N - 1)
        assert top.any() and (e["frac"][top] == 1.0).all() and (e["cell"][top] == N - 2).all()           # the clamp with f = 1
        on_node = (p == np.floor(p)).all(1)
        assert on_node.sum() >= N ** 3 - (N - 2) ** 3
        assert ((e["w"][on_node] == 1.0).sum(1) == 1).all() and ((e["w"][on_node] == 0.0).sum(1) == 7).all()
        on_face = ((p == np.floor(p)).sum(1) == 1)
        assert on_face.any() and ((e["w"][on_face] == 0.25).sum(1) == 4).all()
        corners = ((p == 0) | (p == N - 1)).all(1)
        assert corners.sum() >= 8


LONG_RUN = 256          # the library's kPoissonLongRun: a node with more records is folded by a wave


def longest_run(name):
    return int(np.bincount(CS.expected(name)["node"].reshape(-1)).max())


def test_dense_node_has_a_long_run_and_duplicates_repeat():
    assert longest_run("dense_node") > 4096                     # thousands of records on one node
    for n in MEASURED_CASES:                                    # and no other case reaches the wave-per-run road
        assert (longest_run(n) > LONG_RUN) == (CS.case(n)["family"] == "dense_node"), n
    d = CS.case("duplicates")["points"]
    assert len(d) == 2400 and len(np.unique(d, axis=0)) == 300


def test_plane_patch_density_is_the_recorded_median_and_trims():
    e = CS.expected("plane_patch")
    pos = e["W"][e["W"] > 0]
    assert float(F(np.median(pos))) == CS.PLANE_MIN_DENSITY == CS.case("plane_patch")["cfg"]["min_density"]
    valid = e["W"] >= F(CS.PLANE_MIN_DENSITY)
    assert 0 < valid.sum() < e["occupied_nodes"]


@pytest.mark.parametrize("depth", [3, 4, 5])
def test_the_f64_sphere_mesh_is_closed_genus_0_and_near_the_sphere(depth):
    worst = 0.0
    for pw in (0, 2):
        res = CS.expected(f"sphere_d{depth}_pw{pw}", "f64")
        v, f = mesh_of(res)
        assert len(v) and PC.is_closed(f) and PC.euler(v, f) == 2
        assert PC.signed_volume(v, f) < 0                        # the header's step 8: right-hand normals against the input normals
        worst = max(worst, float(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - CS.RADIUS).max()))
    print("depth", depth, "radial", worst)
    assert worst == pytest.approx(CS.RADIAL[depth], rel=0.02)


# mutant -> (case, the compared quantity it moves)
SHOWN = {"weights_assoc": ("sphere_d3_pw0", "W"), "div_sign": ("sphere_d3_pw0", "b"), "one_sided": ("faces_d3", "b"), "neumann": ("faces_d3", "chi"),
         "iso_grid_mean": ("sphere_d3_pw0", "iso_value"), "no_screen": ("sphere_d3_pw2", "chi")}
# no_upper_clamp: a point with g = N - 1 gets cell N - 1 with f = 0 instead of cell N - 2 with f = 1: the same node takes the same weight
# (1 against 1 - 0), so no value moves; what the clamp guards is the index N of the upper corner, which is outside the grid
# reverse_order: the sums are f64 and rounded to f32 once; the last bits of an f64 sum of a few thousand terms do not reach the f32 result on
# any case of the table, dense_node's 6 000-record node included.  The device's order is pinned by its own two-calls-are-equal test only
INVISIBLE = {"no_upper_clamp": "faces_d3", "reverse_order": "dense_node"}


def test_every_mutant_is_shown_or_listed():
    assert set(SHOWN) | set(INVISIBLE) == set(PC.MUTANTS) and not set(SHOWN) & set(INVISIBLE)


@pytest.mark.parametrize("mutant", sorted(SHOWN))
def test_a_mutant_moves_a_compared_quantity(mutant):
    name, what = SHOWN[mutant]
    c, good = CS.case(name), CS.expected(name)
    bad = PC.run(c["points"], c["normals"], c["cfg"], "exact", rules=(mutant,))
    if what in ("W", "b"):                                      # compared bit for bit
        assert not np.array_equal(bad[what], good[what]), mutant
    elif what == "chi":                                         # compared within 4 x the recorded distance
        assert PC.rel_max(bad["chi"], CS.expected(name, "f64")["chi"]) > 4 * CS.MEASURED[name][0], mutant
    else:
        f64 = CS.expected(name, "f64")
        assert abs(float(bad["iso_value"]) - f64["iso_value"]) / np.abs(f64["chi"]).max() > 4 * CS.MEASURED[name][1], mutant


@pytest.mark.parametrize("mutant", sorted(INVISIBLE))
def test_an_invisible_mutant_moves_nothing(mutant):
    name = INVISIBLE[mutant]
    c, good = CS.case(name), CS.expected(name)
    bad = PC.run(c["points"], c["normals"], c["cfg"], "exact", rules=(mutant,))
    assert np.array_equal(bad["W"], good["W"]) and np.array_equal(bad["b"], good["b"]) and np.array_equal(bad["chi"], good["chi"])
