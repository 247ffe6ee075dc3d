"""The quadric-error simplification contract without a GPU: the invariants of tests/qem_checker.py on every case of tests/qem_cases.py, the
cost key against f64::total_cmp, a mutant table (the checker with one rule changed differs from the real one on a named case), the quality of
the rounds against the reference's one-queue algorithm, and the Python surface."""
import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, synth
from tests import qem_cases as SC
from tests import qem_checker as K

F = np.float32
RUNS = [(name, i) for name, c in sorted(SC.CASES.items()) for i in range(len(c["runs"]))]


def signature(out):
    return tuple((out[k].shape, out[k].tobytes()) for k in ("vertices", "faces", "map")) + (out["rounds"],)


@pytest.fixture(scope="module")
def expected():
    return {name: [K.simplify(c["vertices"], c["faces"], cfg) for cfg in c["runs"]] for name, c in SC.CASES.items()}


def test_the_status_values_are_the_librarys():
    assert (K.OK, K.INVALID_DATA, K.UNSUPPORTED) == (_lib.TC_OK, _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED)


@pytest.mark.parametrize("name,i", RUNS)
def test_invariants_of_every_run(expected, name, i):
    case, cfg, out = SC.CASES[name], SC.CASES[name]["runs"][i], expected[name][i]
    v, f, vmap = out["vertices"], out["faces"].astype(np.int64), out["map"]
    n = len(case["vertices"])
    assert v.dtype == F and out["faces"].dtype == np.uint32 and vmap.dtype == np.uint32 and vmap.shape == (n,)
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(v))                                       # indices in range
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])).all()               # no repeated index
    assert len(np.unique(f)) == len(v)                                                              # only referenced vertices
    # the map is consistent with the faces: an input face whose three images differ and are all alive is an output face's triple
    live = vmap[vmap != K.NO_VERTEX]
    assert sorted(set(live.tolist())) == list(range(len(v)))
    roots = np.nonzero(vmap != K.NO_VERTEX)[0]
    first = roots[np.unique(vmap[roots], return_index=True)[1]]     # the smallest input index per output vertex: the survivor
    assert (np.diff(first) > 0).all()                               # output vertices in ascending input index
    if out["rounds"] == 0:
        assert v.tobytes() == case["vertices"][first].tobytes()     # without a round an output vertex is its input vertex, bit for bit
    images = vmap[case["faces"].astype(np.int64)]
    ok = (images != K.NO_VERTEX).all(axis=1) & (images[:, 0] != images[:, 1]) & (images[:, 1] != images[:, 2]) & (images[:, 2] != images[:, 0])
    assert np.array_equal(images[ok], out["faces"])                 # exactly the surviving faces, in input order, with their orientation
    # the budget
    assert out["selected_none"] or len(f) <= max(out["target"], 0) or out["alive0"] <= out["target"]
    if out["rounds"] and not out["selected_none"]:
        assert len(f) > out["target"] - out["last_multiplicity"]
    assert out["rounds"] == len(out["per_round"]) and all(taken >= 1 for _, _, taken in out["per_round"])


def test_ratio_zero_returns_the_input():
    for name, case in SC.CASES.items():
        out = K.simplify(case["vertices"], case["faces"], K.config(0.0))
        assert out["copy"] and out["rounds"] == 0 and out["vertices"].tobytes() == case["vertices"].tobytes()
        assert out["faces"].tobytes() == case["faces"].tobytes() and np.array_equal(out["map"], np.arange(len(case["vertices"])))


def test_the_cost_key_is_total_cmp():
    tiny = np.float64(5e-324)
    values = np.array([-np.inf, -1e300, -1.5, -1.0, -2.5e-308, -tiny, -0.0, 0.0, tiny, 2.5e-308, 1.0, 1.5, 1e300, np.inf], np.float64)
    keys = K.cost_key(values)
    assert keys.dtype == np.uint64 and (np.diff(keys.astype(object)) > 0).all()              # strictly ascending: -0.0 below +0.0
    rng = np.random.default_rng(7)
    mixed = np.concatenate([values, rng.standard_normal(50) * 1e-3, -values[::-1]])
    mk = K.cost_key(mixed).astype(object)
    for a in range(len(mixed)):
        for b in range(len(mixed)):
            assert K.total_cmp(mixed[a], mixed[b]) == (mk[a] > mk[b]) - (mk[a] < mk[b]), (mixed[a], mixed[b])
    assert int(K.cost_key(np.array([np.nan]))[0]) > int(keys[-1]) and int(keys.max()) < 2 ** 64 - 1     # the filler key is no cost's


# ---- the proofs: a case contains what it is there for ----
def test_cases_hold_what_they_are_there_for(expected):
    assert [len(SC.CASES["icosphere_3"][k]) for k in ("vertices", "faces")] == [642, 1280]
    assert [out["rounds"] for out in expected["tetrahedron"]][:1] == [1] and [out["rounds"] for out in expected["octahedron"]][:1] == [2]
    flat = expected["flat_grid_boundary"][0]
    assert flat["midpoints"] == flat["rounds"] > 0 and flat["min_cost"] == 0.0                     # every det is exactly 0, every cost ties
    assert all(taken == 1 for out in expected["fan_12"][:2] for _, _, taken in out["per_round"]) and expected["fan_12"][1]["rounds"] == 12
    assert expected["fan_12"][2]["rounds"] == 0 and expected["fan_12"][2]["selected_none"]         # every vertex of an open fan is boundary
    assert all(out["longest_ring"] == SC.CONE_FACES > SC.LONG_RING for out in expected[f"cone_{SC.CONE_FACES}"])
    book = expected["book"][0]
    assert book["last_multiplicity"] == 3 and book["per_round"] == [(3, 1, 1)] and len(book["faces"]) == 0 and book["target"] == 1
    odd = expected["octahedron_odd"][0]
    assert (odd["alive0"] - odd["target"]) % 2 == 1 and len(odd["faces"]) == odd["target"] - 1
    two = expected["two_components"][0]
    assert (two["map"][[0, 5, 10]] == K.NO_VERTEX).all() and two["per_round"][0][2] == 2
    untidy = expected["untidy"]
    assert untidy[0]["alive0"] == 9 and len(SC.CASES["untidy"]["faces"]) == 12 and untidy[1]["rounds"] == 0 and len(untidy[1]["faces"]) == 9
    limited, free = expected["stretched_max_edge"]
    assert limited["selected_none"] and len(limited["faces"]) > limited["target"] == free["target"] >= len(free["faces"])
    assert limited["per_round"] != free["per_round"]                                               # the limit ends the run: no candidate is left
    assert expected["offset_1e4"][0]["min_cost"] < 0.0
    field = expected["field_128"][0]
    assert len(SC.CASES["field_128"]["vertices"]) == 128 * 128 and field["rounds"] >= 12 and field["per_round"][0][1] > 256
    ico = expected["icosphere_3"]
    assert [len(out["faces"]) for out in ico] == [1152, 640, 128, 0] and ico[0]["per_round"][0][1] > ico[0]["per_round"][0][2]     # the prefix cut


def test_limits_fail_in_the_order_of_the_checks():
    for name, v, f, cfg, status, text in SC.LIMITS:
        with pytest.raises(K.CheckFailed, match=text.replace(".", r"\.")) as e:
            K.simplify(v, f, cfg)
        assert e.value.status == status, name


# ---- mutants: one rule changed, and the named case shows it ----
MUTANTS = {
    "boundary_le2": ("tetrahedron", "an edge with two incidences made boundary as well"),
    "tie_descending": ("flat_grid_open", "equal costs ranked by descending (lo, hi)"),
    "cut_all": ("icosphere_3", "every selected edge taken, whatever the budget"),
    "fallback_endpoint": ("flat_grid_boundary", "the fallback position is lo's, not the midpoint"),
    "survivor_hi": ("octahedron", "the larger index survives"),
    "degenerate_quadric": ("untidy", "a face that repeats an index adds the quadric of z = 0, as in the reference"),
    "target_f64": ("icosphere_3", "the target computed in f64: 1151, not 1152, at ratio 0.1"),
}
# a mutant no case can show, and why
INVISIBLE = {
    "det_zero_unchecked": "the test det == 0 left out: the three quotients by a zero det are infinite or NaN, so the test for finite "
                          "results takes the midpoint anyway.  (A det that is not finite does not occur below the f64 range.)",
    "boundary_once": "boundary vertices found in the first round only: with preserve_boundary a boundary vertex neither moves nor merges, so "
                     "a boundary edge stays one, and on these meshes a collapse leaves the edges it merges with two sides: no new one appears",
    "fold_reversed": "a vertex's quadric folded in descending face index: the bits of the quadrics differ (the test below), by parts in "
                     "1e16 to 1e14, which neither moves an f32 position across a rounding boundary nor swaps two ranks on these cases",
}


def test_the_fold_order_shows_in_the_bits_of_the_quadrics():
    for name in (f"cone_{SC.CONE_FACES}", "field_128"):
        v, f = SC.CASES[name]["vertices"], SC.CASES[name]["faces"].astype(np.int64)
        quads = K.plane_quadrics(K.planes(v, f))
        up, down = K.vertex_quadrics(len(v), f, quads)[0], K.vertex_quadrics(len(v), f, quads, "fold_reversed")[0]
        assert (up != down).any() and np.allclose(up, down, rtol=1e-9, atol=1e-12), name


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_shows_on_its_named_case(expected, mutant):
    name, _ = MUTANTS[mutant]
    case = SC.CASES[name]
    shown = [signature(K.simplify(case["vertices"], case["faces"], cfg, mutant)) != signature(want) for cfg, want in zip(case["runs"], expected[name])]
    assert any(shown), (mutant, name)


@pytest.mark.parametrize("mutant", sorted(INVISIBLE))
def test_invisible_mutants_are_invisible_everywhere(expected, mutant):
    for name, case in SC.CASES.items():
        for cfg, want in zip(case["runs"], expected[name]):
            assert signature(K.simplify(case["vertices"], case["faces"], cfg, mutant)) == signature(want), (mutant, name)


# ---- quality against the reference's algorithm ----
@pytest.mark.parametrize("ratio", [0.5, 0.9])
@pytest.mark.parametrize("shape", sorted(SC.QUALITY))
def test_rounds_are_as_good_as_the_one_queue_algorithm(shape, ratio):
    v, f = SC.QUALITY[shape]
    cfg = K.config(ratio)
    ours = K.simplify(v, f, cfg)
    lv, lf = K.literal(v, f, cfg)
    assert abs(len(ours["faces"]) - len(lf)) <= 2 and ours["midpoints"] == 0            # the same target; det away from 0
    a, b = K.surface_error(v, ours["vertices"], ours["faces"]), K.surface_error(v, lv, lf)
    print(f"{shape} ratio {ratio}: checker {a:.6g} literal {b:.6g} ratio {a / b:.3f} (measured {SC.QUALITY_MEASURED[(shape, ratio)]})")
    assert a <= SC.QUALITY_K * b, (shape, ratio, a, b, a / b)
    assert SC.QUALITY_K == max(SC.QUALITY_MEASURED.values()) + 0.25


def test_surface_error_is_exact_on_known_distances():
    tri_v, tri_f = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.asarray([[0, 1, 2]], np.uint32)
    box = np.asarray([[-3, -3, -3], [3, 3, 3]], np.float64)          # every point below lies inside: one diagonal
    diag = np.sqrt(108.0)
    for p, d in (([0.25, 0.25, 0.5], 0.5), ([-1, -1, 0], np.sqrt(2.0)), ([0.5, -2, 0], 2.0), ([1, 1, 0], np.sqrt(0.5)), ([0.2, 0.2, 0], 0.0)):
        pts = np.concatenate([box, [p]])
        want = (K.surface_error(box, tri_v, tri_f) * 2 * diag + d) / 3 / diag
        assert abs(K.surface_error(pts, tri_v, tri_f) - want) < 1e-12, p


def test_the_literal_road_meets_the_references_own_assertions():
    """quadric_error.rs:476-...: zero reduction returns the mesh, an empty mesh and a bad ratio are errors"""
    v, f = SC.tetrahedron()
    zv, zf = K.literal(v, f, K.config(0.0))
    assert zv.tobytes() == v.tobytes() and zf.tobytes() == f.tobytes()
    with pytest.raises(K.CheckFailed, match="Mesh is empty"):
        K.literal(v[:0], f[:0], K.config(0.5))
    with pytest.raises(K.CheckFailed, match="Reduction ratio"):
        K.literal(v, f, K.config(1.5))
    lv, lf = K.literal(*SC.QUALITY["icosphere_3"], K.config(0.5))
    assert len(lf) == 640 and lf.max() < len(lv)


# ---- the Python surface ----
def test_python_surface():
    assert "QuadricErrorSimplifier" in threecrate.__all__ and not hasattr(threecrate, "simplify_mesh")
    assert "QuadricErrorSimplifier" in threecrate.ClusteringSimplifier.__doc__ and "simplify_mesh" in threecrate.ClusteringSimplifier.__doc__
    s = threecrate.QuadricErrorSimplifier()
    assert (s.max_edge_length, s.preserve_boundary) == (None, True) and F(s.feature_angle_threshold).view(np.uint32) == 0x3F490FDB
    assert "IGNORED" in threecrate.QuadricErrorSimplifier.__doc__
    t = threecrate.QuadricErrorSimplifier(0.5, False, 1.0)
    assert (t.max_edge_length, t.preserve_boundary, t.feature_angle_threshold) == (0.5, False, 1.0)
    assert hasattr(tc.GpuContext, "simplify_mesh_quadric")
    assert _lib.QEM_EXPORTS == ["tc_qem_config_default", "tc_simplify_quadric", "tc_simplify_quadric_device"]
    assert [f[0] for f in _lib.QemConfigC._fields_] == ["reduction_ratio", "preserve_boundary", "max_edge_length"]


def test_synthetic_meshes_are_what_they_say():
    for level in (0, 1, 3):
        v, f = synth.icosphere(level)
        assert len(v) == 10 * 4 ** level + 2 and len(f) == 20 * 4 ** level and v.dtype == F and f.dtype == np.uint32
        assert np.abs(np.sqrt((v.astype(np.float64) ** 2).sum(axis=1)) - 1.0).max() < 1e-6
        edges = np.sort(np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1)
        assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()                          # closed
        n = K.planes(v, f.astype(np.int64))[:, :3]
        assert ((n * v[f[:, 0]]).sum(axis=1) > 0).all()                                              # outward
    v, f = synth.bumpy_grid_mesh(32, 32, amplitude=0.1, waves=2.0)
    assert len(v) == 1024 and len(f) == 2 * 31 * 31 and v[:, :2].min() == 0.0 and v[:, :2].max() == 1.0 and np.ptp(v[:, 2]) > 0.15
    assert np.array_equal(f, synth.grid_mesh(32, 32)[1])
