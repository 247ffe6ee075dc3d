"""The numpy restatement of the alpha-shape contract (tests/alpha_checker.py) pinned by cases that can be computed by hand, and the Python
surface of the feature (signatures, defaults, __all__, what is Unsupported).  No GPU."""
import inspect

import numpy as np
import pytest

from tests import alpha_cases as AC
from tests import alpha_checker as K

F = np.float32
TRI = AC.CASES["three_points"][0]           # (0,0,0) (1,0,0) (0.5,1,0): sides 1, sqrt(1.25), sqrt(1.25); area 0.5; R^2 = 1.25^2 / (16 * 0.25)


def test_three_points_give_one_candidate_with_every_edge_single():
    r = K.alpha_shape(TRI, 2.0)
    assert r["faces"].tolist() == [[0, 1, 2]] and (r["candidates"], r["boundary_candidates"], r["n_faces"], r["capped"]) == (1, 1, 1, 0)
    assert K.boundary_flags(np.array([[0, 1, 2]])).tolist() == [True]
    guards, R2, area, per, quality = K.triple_terms(TRI[0:1], TRI[1:2], TRI[2:3])
    assert guards[0] and area[0] == F(0.5) and R2[0] == F(1.25 * 1.25 / 4.0)
    # alpha 1.2 still sees both neighbours of point 0 (1 and sqrt(1.25) = 1.118) but R^2 = 0.39 <= 1.44; alpha^2 below R^2 needs alpha < 0.625,
    # where point 0 has no neighbour left: no candidate at all
    assert K.alpha_shape(TRI, 1.2)["n_faces"] == 1
    with pytest.raises(K.AlphaError, match="No candidate triangles generated") as e:
        K.alpha_shape(TRI, 0.9)
    assert e.value.kind == "Algorithm"
    # the face filter on its own: a wide flat triangle whose circumradius exceeds alpha while its points are neighbours
    flat = np.array([[0, 0, 0], [1, 0, 0], [0.5, 0.1, 0]], F)         # R = 1.3 > alpha = 1.05 >= the sides
    with pytest.raises(K.AlphaError, match="No triangles survived alpha filtering"):
        K.alpha_shape(flat, 1.05)


def test_a_regular_tetrahedron_has_every_edge_on_two_candidates():
    tet, alpha, _ = AC.CASES["tetrahedron"]
    full = K.alpha_shape(tet, alpha, K.FULL)
    assert full["faces"].tolist() == [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]] and full["boundary_candidates"] == 0 and full["candidates"] == 4
    with pytest.raises(K.AlphaError, match="No triangles survived alpha filtering"):
        K.alpha_shape(tet, alpha, K.BOUNDARY)


def test_collinear_and_duplicated_points_fall_to_the_guards():
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    with pytest.raises(K.AlphaError, match="No candidate"):
        K.alpha_shape(line, 5.0)
    dup = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]], F)       # (0, 1, *) have a^2 = 0 < 1e-20
    r = K.alpha_shape(dup, 5.0, K.FULL)
    assert r["faces"].tolist() == [[0, 2, 3], [1, 2, 3]]
    assert len(K.neighbours(dup, 0, 5.0)) == 3                             # the duplicate is a neighbour


def test_a_sliver_either_side_of_the_quality_bound():
    # an isosceles sliver of base 1 and height h: quality = 4 (h / 2) / per^2, per = 1 + 2 sqrt(0.25 + h^2); 0.01 is crossed near h = 0.02
    def quality(h):
        p = np.array([[0, 0, 0], [1, 0, 0], [0.5, h, 0]], F)
        return K.triple_terms(p[0:1], p[1:2], p[2:3])[4][0], p
    (q_lo, p_lo), (q_hi, p_hi) = quality(0.0199), quality(0.0203)
    assert q_lo <= F(0.01) < q_hi
    with pytest.raises(K.AlphaError, match="No candidate"):
        K.alpha_shape(p_lo, 50.0)
    assert K.candidates(p_hi, 50.0)[0].tolist() == [[0, 1, 2]]


def test_the_result_depends_on_the_order_of_the_points():
    a, b = AC.expected("grid_1.3", "full"), AC.expected("grid_permuted_1.3", "full")
    assert a["candidates"] != b["candidates"]                              # j and k need not be neighbours: the lowest index decides
    assert AC.expected("grid_1.3", "boundary")["n_faces"] != a["n_faces"]  # the two modes differ on the grid
    for r in (a, b):
        f = r["faces"].astype(np.int64)
        assert (f[:, 0] < f[:, 1]).all() and (f[:, 1] < f[:, 2]).all()
        key = (f[:, 0] << 40) | (f[:, 1] << 20) | f[:, 2]
        assert (np.diff(key) > 0).all()                                    # lexicographic order


def test_the_caps_of_the_cases_do_what_their_names_say():
    points, alpha, cap = AC.CASES["sphere300_cap200"]
    tri = K.candidates(points, alpha, 1e-8, cap)[0]
    whole = K.candidates(points, alpha, 1e-8, 0)[0]
    assert len(tri) == 200 and np.array_equal(tri, whole[:200])
    assert whole[199, 0] == whole[200, 0]                                  # the cut falls inside one point's pairs
    big = AC.expected("sphere700_reference_cap", "boundary")
    assert (big["candidates"], big["capped"]) == (K.REFERENCE_CAP, 1) and big["n_faces"] > 0
    for name in ("sphere300_0.25", "sphere300_0.35", "sphere300_0.5", "grid_1.3", "grid_1.6"):
        assert AC.expected(name, "boundary")["n_faces"] > 0 and AC.expected(name, "full")["n_faces"] > 0
    assert AC.expected("sphere300_uncapped", "full")["faces"].tobytes() == AC.expected("sphere300_cap_above", "full")["faces"].tobytes()


def test_the_cluster_cases_reach_the_lengths_they_are_sized_for():
    longest = lambda name: max(int((K.neighbours(AC.CASES[name][0], i, AC.CASES[name][1]) > i).sum()) for i in range(len(AC.CASES[name][0])))
    assert 64 < longest("cluster_longer_than_a_wave") <= AC.STAGE
    p = AC.CASES["cluster_across_the_stage"][0]
    lengths = {int((K.neighbours(p, i, 1.0) > i).sum()) for i in range(len(p))}
    assert {AC.STAGE - 1, AC.STAGE, AC.STAGE + 1, 2 * AC.STAGE + 1} <= lengths
    p = AC.CASES["cluster_among_isolated_points"][0]
    pairs = sum(int((K.neighbours(p, i, 1.0) > i).sum()) for i in range(len(p)))
    assert pairs // len(p) < AC.PACK_BELOW and longest("cluster_among_isolated_points") > AC.STAGE
    assert longest("sphere300_0.25") < AC.PACK_BELOW                       # the sparse sphere packs four points into a wave as well


def test_invalid_arguments_in_the_headers_order():
    for args, word in (((TRI[:0], 1.0), "empty"), ((TRI[:2], 1.0), "at least 3"), ((TRI, 1.0, 2), "mode"), ((TRI, 0.0), "alpha"),
                       ((TRI, float("nan")), "alpha"), ((TRI, float("inf")), "alpha"), ((TRI, 1.0, 0, -1.0), "min_triangle_area")):
        with pytest.raises(K.AlphaError, match=word) as e:
            K.alpha_shape(*args)
        assert e.value.kind == "InvalidData"


def test_the_python_surface():
    import threecrate_amd as tc
    import threecrate_amd.compat as threecrate
    from threecrate_amd import _lib
    sig = inspect.signature(tc.GpuContext.alpha_shape)
    assert list(sig.parameters)[:7] == ["self", "points", "alpha", "mode", "min_triangle_area", "max_triangles", "return_stats"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["mode"], d["min_triangle_area"], d["max_triangles"], d["return_stats"]) == ("boundary", 1e-8, 50000, False)
    assert {"alpha_shape_reconstruct", "estimate_optimal_alpha"} <= set(threecrate.__all__)
    assert list(inspect.signature(threecrate.alpha_shape_reconstruct).parameters) == ["cloud", "alpha"]
    assert inspect.signature(threecrate.alpha_shape_reconstruct).parameters["alpha"].default == 1.0          # threecrate.pyi
    assert list(inspect.signature(threecrate.estimate_optimal_alpha).parameters) == ["cloud", "k"]
    assert _lib.ALPHA_EXPORTS == ["tc_alpha_config_default", "tc_alpha_shape", "tc_alpha_shape_device"]
    assert (_lib.TC_ALPHA_BOUNDARY_ONLY, _lib.TC_ALPHA_FULL, _lib.TC_ALPHA_REFERENCE_CAP) == (K.BOUNDARY, K.FULL, K.REFERENCE_CAP)
    # what is out of scope is refused before any device is touched
    ctx = tc.GpuContext.__new__(tc.GpuContext)
    with pytest.raises(tc.Unsupported, match="fast_mode"):
        tc.GpuContext.alpha_shape(ctx, TRI, 1.0, fast_mode=True)
    with pytest.raises(tc.Unsupported, match="adaptive"):
        tc.GpuContext.alpha_shape(ctx, TRI, 1.0, mode="adaptive")
    with pytest.raises(RuntimeError, match="Point cloud is empty"):
        threecrate.alpha_shape_reconstruct(threecrate.PointCloud(), 1.0)
    with pytest.raises(RuntimeError, match="Point cloud is empty"):
        threecrate.estimate_optimal_alpha(threecrate.PointCloud(), 5)
    assert threecrate.estimate_optimal_alpha(threecrate.PointCloud.from_numpy(TRI), 3) == 1.0               # no sample has three other points


def test_estimate_optimal_alpha_sampling_against_brute_force():
    """the checker's sampling arithmetic (sample, step, the k-th other distance, the median) against a plain numpy version"""
    for n, k in ((30, 3), (499, 5), (700, 8), (5300, 4), (6, 5), (6, 6)):
        p = AC.sphere(n, 12)
        sample = min(max(n // 10, 50), 500)
        step = max(n // sample, 1)
        picked = list(range(0, n, step))
        assert len(picked) == -(-n // step)
        kth = []
        for i in picked:
            d = np.sqrt(K.norm_sq(p[i] - p))
            others = sorted(float(x) for j, x in enumerate(d) if j != i)
            if len(others) >= k:
                kth.append(F(others[k - 1]))
        want = F(1.0) if not kth else F(sorted(kth)[len(kth) // 2] * F(1.8))
        assert K.estimate_optimal_alpha(p, k) == want, (n, k)
        # the (k + 1)-list that holds the sample itself: its entry k is the k-th other distance
        if n - 1 >= k:
            i = picked[len(picked) // 2]
            both = np.sort(np.sqrt(K.norm_sq(p[i] - p)))
            assert both[0] == 0 and both[k] == F(sorted(float(x) for j, x in enumerate(np.sqrt(K.norm_sq(p[i] - p))) if j != i)[k - 1])
