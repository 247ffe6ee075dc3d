"""The mesh simplification contract without a GPU: tests/simplify_checker.py against its literal restatement of clustering.rs on every case
of tests/simplify_cases.py, the reference's own assertions, the proof per family that a case holds what it is there for, and a mutant table:
the checker with one rule changed differs from the real one on a named case."""
import numpy as np
import pytest

import threecrate_amd as tc
import threecrate_amd.compat as threecrate
from threecrate_amd import _lib, synth
from tests import simplify_cases as SC
from tests import simplify_checker as K

F = np.float32
KEYS = ("vertices", "faces", "normals", "colors")


def checker(case, params, mutant=None):
    return K.simplify(case["vertices"], case["faces"], normals=case["normals"], colors=case["colors"], mutant=mutant, **params)


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes())


def signature(out):
    return tuple(None if out[k] is None else (out[k].shape, out[k].tobytes()) for k in KEYS + ("map",))


@pytest.fixture(scope="module")
def expected():
    return {name: [checker(c, p) for p in c["runs"]] for name, c in SC.CASES.items()}


def test_the_status_values_are_the_librarys():
    assert (K.OK, K.INVALID_DATA, K.UNSUPPORTED) == (_lib.TC_OK, _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED)
    assert K.DEFAULT_ANGLE == tc.GpuContext.SIMPLIFY_DEFAULT_FEATURE_ANGLE and F(K.DEFAULT_ANGLE).view(np.uint32) == 0x3F490FDB
    assert K.cosf(SC.PI) == F(-1.0) and K.cosf(0.0) == F(1.0) and K.cosf(SC.HALF_PI) < 0 < K.cosf(SC.BELOW_HALF_PI)


@pytest.mark.parametrize("name", sorted(n for n, c in SC.CASES.items() if c["literal"]))
def test_the_checker_equals_the_literal_restatement(expected, name):
    """up to the permutation of output vertices that step 6 fixes: the literal road's clusters sorted by cell key"""
    case = SC.CASES[name]
    for params, want in zip(case["runs"], expected[name]):
        lit = K.literal_in_contract_order(case["vertices"], case["faces"], normals=case["normals"], colors=case["colors"], **params)
        for key in KEYS:
            assert same(want[key], lit[key]), (params, key)
        # the member order of every cluster is the reference's own (ascending vertex index): no summation-order bound is needed
        assert all(list(members) == sorted(members) for _, members in lit["clusters"])
        assert sorted(len(m) for _, m in lit["clusters"]) == sorted(want["sizes"].tolist())


def test_the_insertion_order_is_a_permutation_of_the_contract_order(expected):
    case, params = SC.CASES["classes_open_box"], SC.CASES["classes_open_box"]["runs"][0]
    first = K.literal(case["vertices"], case["faces"], normals=case["normals"], colors=case["colors"], **params)
    want = expected["classes_open_box"][0]
    assert [k for k, _ in first["clusters"]] != sorted(k for k, _ in first["clusters"])           # the HashMap's order is not the contract's
    order = np.lexsort(first["vertices"].T[::-1])
    assert same(first["vertices"][order], want["vertices"][np.lexsort(want["vertices"].T[::-1])])
    assert len(first["faces"]) == len(want["faces"])


# ---- the reference's assertions (clustering.rs:996-1247) ----
def test_the_references_assertions(expected):
    for name in ("reference_plane_6", "reference_plane_11", "reference_curved_8"):
        for params, out in zip(SC.CASES[name]["runs"], expected[name]):
            if params["ratio"] == 0.5:
                assert 0 < len(out["faces"]) < len(SC.CASES[name]["faces"]), (name, params)
    assert len(SC.CASES["reference_plane_6"]["faces"]) == 50 and len(SC.CASES["reference_plane_11"]["faces"]) == 200
    for out in expected["reference_triangle"]:
        assert len(out["vertices"]) > 0
    for out in expected["reference_tetrahedron"]:
        assert len(out["vertices"]) <= 4
    for params, out in zip(SC.CASES["reference_sharp_edge"]["runs"], expected["reference_sharp_edge"]):
        assert out["feature"].any() == (params["threshold"] == K.DEFAULT_ANGLE)
        if params["ratio"] == 0.3:
            assert len(out["faces"]) > 0 and len(out["vertices"]) > 0
    (out,) = expected["reference_plane_5_attributes"]
    assert len(out["normals"]) == len(out["colors"]) == len(out["vertices"]) > 0 and (out["normals"][:, 2] > 0.9).all()
    assert (out["colors"] == [128, 64, 200]).all()
    zero = K.simplify(*SC.TRIANGLE, 0.0)
    assert len(zero["vertices"]) == 3 and len(zero["faces"]) == 1 and zero["copy"]


def test_boundary_vertices_only_merge_with_boundary_vertices(expected):
    """test_boundary_preservation_uniform restated exactly: with preserve_boundary no cluster mixes the classes"""
    for name in ("reference_plane_6", "classes_open_box", "blocks_513"):
        case = SC.CASES[name]
        for params, out in zip(case["runs"], expected[name]):
            if not params["preserve_boundary"]:
                continue
            on_boundary = out["boundary"]
            assert on_boundary.any() and not on_boundary.all()
            for c in np.unique(out["cluster_of"][on_boundary]):
                assert on_boundary[out["cluster_of"] == c].all(), (name, params, c)


# ---- the proofs: a case contains what it is there for ----
def test_blocks_straddle_a_block_and_hold_an_unreferenced_vertex(expected):
    assert [len(SC.CASES[f"blocks_{n}"]["vertices"]) for n in SC.BLOCKS] == list(SC.BLOCKS) == [255, 256, 257, 513]
    assert [len(SC.CASES[f"blocks_faces_{m}"]["faces"]) for m in (255, 256, 257)] == [255, 256, 257]
    c = SC.CASES["blocks_257"]
    assert 256 not in c["faces"] and (expected["blocks_257"][0]["map"][256] == K.NO_VERTEX)
    inside = expected["blocks_unreferenced_inside"]
    n = len(SC.CASES["blocks_unreferenced_inside"]["vertices"])
    assert n - 1 not in SC.CASES["blocks_unreferenced_inside"]["faces"]
    assert any(out["map"][n - 1] != K.NO_VERTEX and out["sizes"][out["cluster_of"][n - 1]] > 1 for out in inside)


def test_cluster_sizes_are_exactly_what_their_names_say(expected):
    assert {1, 2, SC.LONG_CLUSTER - 1, SC.LONG_CLUSTER, SC.LONG_CLUSTER + 1, 192, 193, 256, 257} <= set(SC.CLUSTER_SIZES) and max(SC.CLUSTER_SIZES) > 4000
    for s in SC.CLUSTER_SIZES:
        for out in expected[f"cluster_sizes_{s}"]:
            assert sorted(out["sizes"].tolist()) == sorted([s, 1, 1]) and out["used"].all()
            assert len(out["faces"]) == 1 and out["repeated"] == s - 1 and out["degenerate"] == 0
            assert out["faces"].tolist() == [[0, 2, 1]]            # face 0 survives with its own orientation: apexes, B = cell (1, 0), C = cell (0, 1)
    for out in expected["cluster_sizes_five_long"]:
        assert sorted(out["sizes"].tolist()) == sorted(SC.five_long_clusters()[2].tolist()) and len(out["sizes"]) == 45
        assert sorted(s for s in out["sizes"].tolist() if s > SC.LONG_CLUSTER) == [129, 192, 193, 256, 257] and (out["sizes"] <= SC.LONG_CLUSTER).sum() == 40
    # the order of the fold shows in the bits of the large apexes: the members reversed give another sum
    big = SC.CASES["cluster_sizes_4097"]["vertices"][:4097].astype(np.float64)
    assert not np.array_equal(np.add.accumulate(big, axis=0)[-1], np.add.accumulate(big[::-1], axis=0)[-1])
    grid = expected["cluster_sizes_ratio_1_grid"]
    assert all(out["sizes"].max() > 500 for out in grid) and all(len(out["sizes"]) <= 12 for out in grid)
    (empty,) = expected["cluster_sizes_zero_faces"]
    assert len(empty["faces"]) == 0 and len(empty["vertices"]) == 0 and (empty["map"] == K.NO_VERTEX).all() and empty["degenerate"] == 1


def test_classes_reach_every_class_and_both_sides_of_every_dot(expected):
    box, open_box = SC.CASES["classes_box"], SC.CASES["classes_open_box"]
    seen = {}
    for name, case in (("box", box), ("open_box", open_box)):
        for params, out in zip(case["runs"], expected[f"classes_{name}"]):
            seen[(name, params["preserve_boundary"], params["threshold"])] = out
    # the closed box has no boundary; across a box edge the dot is exactly 0, inside a side exactly 1
    for pb in (0, 1):
        assert not seen[("box", pb, K.DEFAULT_ANGLE)]["boundary"].any()
        edges = seen[("box", pb, K.DEFAULT_ANGLE)]["feature"]
        assert 0 < edges.sum() < len(edges)
        assert np.array_equal(seen[("box", pb, SC.BELOW_HALF_PI)]["feature"], edges)              # cos just above 0: 0 < cos
        assert not seen[("box", pb, SC.HALF_PI)]["feature"].any()                                 # cosf(pi / 2) < 0: 0 < cos fails
        assert np.array_equal(seen[("box", pb, 0.0)]["feature"], edges)                           # cos = 1: dot 1 < 1 fails at equality, dot 0 < 1
        assert seen[("box", pb, 1e-3)]["feature"].sum() == edges.sum()
        assert not seen[("box", pb, SC.PI)]["feature"].any()
    out = seen[("open_box", 1, K.DEFAULT_ANGLE)]
    assert (out["classes"] > 0).all() and out["boundary"].sum() == 16                             # interior, boundary and feature vertices
    assert (seen[("open_box", 0, K.DEFAULT_ANGLE)]["classes"][1] == 0) and seen[("open_box", 0, K.DEFAULT_ANGLE)]["boundary"].sum() == 16
    # some cell holds clusters of more than one class
    cells = {}
    for params, out in zip(open_box["runs"], expected["classes_open_box"]):
        if params["ratio"] == 0.9 and params["preserve_boundary"] == 1 and params["threshold"] == K.DEFAULT_ANGLE:
            assert len(out["cluster_classes"]) > len(set(out["cluster_classes"].tolist()))
            cells = set(out["cluster_classes"].tolist())
    assert cells == {0, 1, 2}
    pair = expected["faces_open_pair"]
    assert not pair[0]["feature"].any() and pair[1]["feature"].sum() == 3                         # dot exactly -1: -1 < cosf(pi) = -1 fails, -1 < cosf(3.0)


def test_faces_drop_repeats_and_degenerates_and_keep_the_first(expected):
    once, twice = SC.CASES["faces_twice"], expected["faces_twice"]
    m = len(once["faces"]) // 2
    for params, out in zip(once["runs"], twice):
        single = K.simplify(once["vertices"], once["faces"][:m], **params)
        assert out["repeated"] >= m - out["degenerate"] // 2 - single["repeated"] and out["repeated"] > 0
    for out_a, out_b in zip(expected["faces_twice_interleaved_reversed"], expected["faces_reversed_first"]):
        assert len(out_a["faces"]) == len(out_b["faces"]) > 0
        assert not same(out_a["faces"], out_b["faces"])                                            # the first copy's orientation survives: they differ
    for out in expected["faces_repeated_index"]:
        assert out["degenerate"] >= 4


def test_degenerate_boxes_have_the_dimension_they_claim(expected):
    dims = {"degenerate_box_point": 0, "degenerate_box_line": 1, "degenerate_box_plane": 2, "degenerate_box_extent_below": 2,
            "degenerate_box_extent_equal": 2, "degenerate_box_extent_above": 3, "degenerate_box_line_target": 1}
    for name, dim in dims.items():
        assert all(out["dim"] == dim for out in expected[name]), name
    assert all(out["cell"] == 1.0 for out in expected["degenerate_box_point"])
    assert all(out["cell"] == 1.0 for out in expected["degenerate_box_line_target"])


def test_shifted_runs_have_the_unmoved_runs_clusters(expected):
    base = expected["shifted_0"]
    for sh in SC.SHIFTS[1:]:
        for a, b in zip(base, expected[f"shifted_{int(sh)}"]):
            assert np.array_equal(a["cluster_of"], b["cluster_of"]) and same(a["faces"], b["faces"]) and same(a["map"], b["map"])
            assert not same(a["vertices"], b["vertices"])


def test_attributes_cancel_and_saturate(expected):
    both = expected["attributes_both"]
    for out in both:
        ln = np.sqrt((out["normals"].astype(np.float64) ** 2).sum(axis=1))
        assert (ln == 0.0).any() and (ln > 0.99).any()                    # a cluster whose normals cancel keeps the raw sum: len <= 1e-12
        assert (out["colors"] == 255).all()
    assert all(out["normals"] is None for out in expected["attributes_colors"]) and all(out["colors"] is None for out in expected["attributes_normals"])


def test_limits_fail_in_the_order_of_the_checks():
    for name, v, f, params, status, text in SC.LIMITS:
        with pytest.raises(K.CheckFailed, match=text.replace(".", r"\.")) as e:
            K.simplify(v, f, **params)
        assert e.value.status == status, name


def test_wide_keys_pass_two_to_the_21():
    v, f, params = SC.wide_keys()
    assert len(v) > 2 ** 21 and 3 * _lib_bits(len(v) - 1) > 64


def _lib_bits(v):
    b = 1
    while (1 << b) <= v:
        b += 1
    return b


# ---- mutants: one rule changed, and the named case shows it ----
MUTANTS = {
    "dot_le": ("classes_box", "dot <= cos: the equalities at 0 and 1"),
    "boundary_le2": ("reference_plane_6", "an edge with two incidences made boundary as well"),
    "class_ignored": ("reference_plane_6", "the class left out of the key"),
    "centroid_f32": ("cluster_sizes_4097", "centroid sums in f32"),
    "valence_unclamped": ("blocks_unreferenced_inside", "valence 0 not clamped to 1"),
    "last_face_wins": ("faces_twice_interleaved_reversed", "the last face of equal triples survives"),
    "faces_resorted": ("reference_tetrahedron", "survivors in triple order, not input order"),
    "orientation_canonical": ("reference_triangle", "survivors written as their sorted triple"),
    "unused_kept": ("blocks_257", "clusters in no surviving face kept"),
    "colour_nearest": ("blocks_255", "colour division rounding to nearest"),
    "normals_raw": ("blocks_255", "normals not normalised"),
    "extent_ge": ("degenerate_box_extent_equal", "the extents filter at >= 1e-6"),
    "target_f64": ("degenerate_box_line_target", "the target computed in f64"),
}
# a mutant no case can show, and why
INVISIBLE = {
    "single_divided": "a cluster of one through the weighted road's division: f64(x) * w is exact for a 24-bit x and an integer w below 2^29, "
                      "and the exact product divided by w gives x back, so f32(s / W) has the vertex's own bits",
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_shows_on_its_named_case(expected, mutant):
    name, _ = MUTANTS[mutant]
    case = SC.CASES[name]
    shown = [signature(checker(case, p, mutant)) != signature(want) for p, want in zip(case["runs"], expected[name])]
    assert any(shown), (mutant, name)


@pytest.mark.parametrize("mutant", sorted(INVISIBLE))
def test_invisible_mutants_are_invisible_everywhere(expected, mutant):
    for name, case in SC.CASES.items():
        for p, want in zip(case["runs"], expected[name]):
            assert signature(checker(case, p, mutant)) == signature(want), (mutant, name)


# ---- the Python surface ----
def test_python_surface():
    assert "ClusteringSimplifier" in threecrate.__all__ and not hasattr(threecrate, "simplify_mesh")
    assert "simplify_mesh" in threecrate.ClusteringSimplifier.__doc__                 # says that the wheel's quadric call stays absent
    s = threecrate.ClusteringSimplifier()
    assert (s.mode, s.representative_strategy, s.preserve_boundary) == ("uniform", "centroid", True)
    assert F(s.feature_angle_threshold).view(np.uint32) == 0x3F490FDB
    with pytest.raises(tc.Unsupported):
        threecrate.ClusteringSimplifier(mode="adaptive")
    with pytest.raises(tc.Unsupported):
        threecrate.ClusteringSimplifier(representative_strategy="minimum_error")
    assert hasattr(tc.GpuContext, "simplify_mesh_clustering")
    assert _lib.SIMPLIFY_EXPORTS == ["tc_simplify_config_default", "tc_simplify_clustering", "tc_simplify_clustering_device"]


def test_box_mesh_is_closed_welded_and_exactly_axis_aligned():
    for k in (1, 3, 4):
        v, f, nrm = synth.box_mesh(k)
        assert len(v) == 6 * k * k + 2 and len(f) == 12 * k * k and f.dtype == np.uint32 and v.dtype == nrm.dtype == F
        fn = K.face_normals(v, f.astype(np.int64))
        assert (np.abs(fn).max(axis=1) == 1.0).all() and (np.abs(fn).sum(axis=1) == 1.0).all()      # exactly +-axis
        assert ((fn * (v[f].mean(axis=1) - F(0.5))).sum(axis=1) > 0).all()                           # outward
        assert (np.abs(nrm).sum(axis=1) == 1.0).all()
        agrees = np.zeros(len(v), bool)                           # a vertex's normal is the normal of one of its faces
        for corner in range(3):
            agrees[f[:, corner][(nrm[f[:, corner]] == fn).all(axis=1)]] = True
        assert agrees.all()
        edges = np.sort(np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1)
        assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()                          # closed
        vo, fo, _ = synth.box_mesh(k, open_side=True)
        eo = np.sort(np.stack([fo[:, [0, 1]], fo[:, [1, 2]], fo[:, [2, 0]]], axis=1).reshape(-1, 2), axis=1)
        assert len(fo) == 10 * k * k and (np.unique(eo, axis=0, return_counts=True)[1] == 1).sum() == 4 * k
