"""The marching-cubes case table (tools/gen_mc_table.py -> threecrate_amd/csrc/mc_table.h) held to its invariants, and the numpy checker
(tests/mc_checker.py) held to its own rules by mutants.  No GPU.

The table is generated from a stated rule and is not the classic table; these invariants are what make it a correct table:
every case uses exactly its crossing edges, its triangles close along every crossing edge, every triangle faces the inside, and two
cubes that share a face draw the same segments on it, so that the welded mesh of ANY field is an oriented manifold."""
import itertools
import os
import subprocess
import sys
from collections import Counter

import numpy as np

from tests import mc_cases as MC
from tests import mc_checker as K

G = K.G
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_regenerating_gives_the_committed_header_byte_for_byte():
    assert open(G.HEADER).read() == G.render()
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "gen_mc_table.py"), "--check"]) == 0
    text = open(G.HEADER).read()
    assert "GENERATED" in text.splitlines()[0] and "DO NOT EDIT" in text.splitlines()[0]
    rows, _ = G.table()
    width, total = 3 * max(len(r) for r in rows), sum(len(r) for r in rows)
    assert f"#define TC_MC_ROW {width}\n" in text and f"#define TC_MC_TOTAL_TRIS {total}\n" in text
    assert (width, total) == (15, 820)                  # what the header and STATE.md record
    state = open(os.path.join(ROOT, "STATE.md")).read()
    assert "15 edge numbers" in state and "820 triangles" in state


def test_numbering_and_winding_are_the_references():
    assert G.triangles(1) == [(0, 8, 3)]                # case 1: the triangle of edges 0, 8, 3, its normal at corner 0
    assert G.triangles(0) == [] and G.triangles(255) == []


def _sides(tris):
    """the directed boundary sides of a list of triangles"""
    return [(t[k], t[(k + 1) % 3]) for t in tris for k in range(3)]


def test_every_case_closes_along_its_crossing_edges_and_faces_the_inside():
    for c in range(256):
        tris, cross = G.triangles(c), G.crossing_edges(c)
        assert sorted({e for t in tris for e in t}) == cross, c                     # exactly the crossing edges
        # a side between two crossing edges that lie on one cube face is a boundary side (it lies in the face, the neighbouring cube
        # continues there); every other side is a chord inside the cube and is used once in each direction
        directed = Counter(_sides(tris))
        boundary = Counter()
        for (a, b), k in directed.items():
            if directed.get((b, a), 0):
                assert k == 1 and directed[(b, a)] == 1 and not G.same_face(a, b), (c, a, b)   # a chord never lies in a face
            else:
                assert k == 1 and G.same_face(a, b), (c, a, b)
                boundary[a] += 1
                boundary[b] += 1
        assert all(boundary[e] == 2 for e in cross) and set(boundary) == set(cross), c     # every crossing edge meets exactly two boundary sides
        for t in tris:                                                              # the triangle's normal points to ITS inside ends
            n, d = G.newell(list(t)), G.inward(c, list(t))
            assert n[0] * d[0] + n[1] * d[1] + n[2] * d[2] > 0, (c, t)


def test_two_cubes_that_share_a_face_draw_the_same_segments_in_opposite_directions():
    """all 3 x 2^12 sign patterns of two cubes side by side along each axis"""
    step = {0: (1, 0, 0), 1: (0, 1, 0), 2: (0, 0, 1)}
    rows = {c: G.triangles(c) for c in range(256)}
    sides = {c: set(_sides(rows[c])) for c in range(256)}
    for axis in range(3):
        hi_face = 2 * axis + 1                   # FACES: x = 0, x = 1, y = 0, y = 1, z = 0, z = 1
        # corner of the first cube's upper face -> the same grid point as a corner of the second cube's lower face
        twin = {a: G.CORNERS.index(tuple(p - s for p, s in zip(G.CORNERS[a], step[axis]))) for a in G.FACES[hi_face]}
        edge_twin = {G.edge_of(a, b): G.edge_of(twin[a], twin[b]) for a, b in G.EDGES if a in twin and b in twin}
        free = [k for k in range(8) if k not in twin]
        lo_free = [k for k in range(8) if k not in twin.values()]
        for bits in itertools.product((0, 1), repeat=12):
            shared = dict(zip(sorted(twin), bits[:4]))
            c1 = sum(shared[a] << a for a in twin) | sum(b << k for k, b in zip(free, bits[4:8]))
            c2 = sum(shared[a] << twin[a] for a in twin) | sum(b << k for k, b in zip(lo_free, bits[8:12]))
            s1 = {(edge_twin[a], edge_twin[b]) for a, b in sides[c1] if a in edge_twin and b in edge_twin and (b, a) not in sides[c1]}
            s2 = {(a, b) for a, b in sides[c2] if a in edge_twin.values() and b in edge_twin.values() and (b, a) not in sides[c2]}
            assert s1 == {(b, a) for a, b in s2}, (axis, c1, c2)


def _manifold(v, f, dims, vs, org):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    directed = Counter(map(tuple, e))
    und = Counter()
    for (a, b), k in directed.items():
        und[(min(a, b), max(a, b))] += k
    lo = np.asarray(org, np.float32)
    hi = lo + (np.asarray(dims, np.float32) - 1) * np.asarray(vs, np.float32)
    for (a, b), k in und.items():
        on_boundary = any((v[a, ax] == lo[ax] and v[b, ax] == lo[ax]) or (v[a, ax] == hi[ax] and v[b, ax] == hi[ax]) for ax in range(3))
        if k == 2:
            assert directed[(a, b)] == 1 and directed[(b, a)] == 1, (a, b)
        else:
            assert k == 1 and on_boundary, (a, b, k)
    return len(und)


def test_the_welded_mesh_of_a_random_field_is_an_oriented_manifold():
    """a random 9^3 field has many ambiguous faces; every mesh edge not on the grid's boundary belongs to exactly two faces with opposite
    directions, every boundary edge to one.  This holds by construction of the table"""
    v = np.random.default_rng(5).standard_normal((9, 9, 9)).astype(np.float32)
    inside = v < 0
    # faces in the x-y planes whose diagonals agree and differ from each other: ambiguous
    ambiguous = int(((inside[:-1, :-1] == inside[1:, 1:]) & (inside[:-1, 1:] == inside[1:, :-1]) & (inside[:-1, :-1] != inside[:-1, 1:])).sum())
    assert ambiguous > 50
    for layout in ("z_fastest", "x_fastest"):
        p, _, f = K.marching_cubes(MC.from_xyz(v, layout), (9, 9, 9), weld=True, normals=False, layout=layout)
        assert _manifold(p, f, (9, 9, 9), (1, 1, 1), (0, 0, 0)) > 2000


def test_the_sphere_is_closed_and_synth_follows_the_reference_helpers():
    case = MC.sphere(33)
    v, n, f = K.marching_cubes(case["values"], case["dims"], case["voxel_size"], case["origin"], weld=True)
    edges = _manifold(v, f, case["dims"], case["voxel_size"], case["origin"])
    assert len(v) - edges + len(f) == 2
    assert np.float32(case["voxel_size"][0]) == np.float32(3.0) / np.float32(32) and np.float32(case["origin"][0]) == np.float32(0.1) - np.float32(1.5)
    # the normals point to the inside (the negative gradient): towards the centre
    to_centre = np.array([0.1, -0.2, 0.3]) - v.astype(np.float64)
    assert (np.sum(to_centre * n, axis=1) > 0.9 * np.linalg.norm(to_centre, axis=1)).all()
    # and so does every face's geometric normal
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    assert (np.sum(fn * (np.array([0.1, -0.2, 0.3]) - v[f[:, 0]]), axis=1) > 0).all()
    b = MC.box(33)
    assert (b["values"] == 0).sum() > 0                 # faces on grid planes: values equal to iso


def _differs(a, b):
    return any((x is None) != (y is None) or (x is not None and (x.shape != y.shape or x.tobytes() != y.tobytes())) for x, y in zip(a, b))


def test_mutants_of_the_checker_are_visible(capsys):
    """each deliberate deviation of the checker differs from the real checker on a named case"""
    table = [("le", "exact_iso037", dict()), ("no_half", "exact_iso0", dict()), ("weld_reversed", "random9_z_fastest", dict(weld=True)),
             ("normals_plus", "sphere33", dict()), ("bound_gt", "line_z_256_z_fastest", dict()), ("other_order", "dims_17_5_3_z_fastest", dict()),
             ("no_mask", "mask20", dict()), ("other_ambiguous", "random9_x_fastest", dict(weld=True))]
    shown = []
    for mutant, name, kw in table:
        c = MC.CASES[name]()
        args = (c["values"], c["dims"], c["voxel_size"], c["origin"], c["iso_level"], True, kw.get("weld", False), c["valid"], c["layout"])
        real, mut = K.marching_cubes(*args), K.marching_cubes(*args, mutant=mutant)
        which = [k for k, x, y in zip(("vertices", "normals", "faces"), real, mut) if _differs((x,), (y,))]
        shown.append((mutant, name, which))
    with capsys.disabled():
        print()
        for mutant, name, which in shown:
            print(f"  mutant {mutant:16s} on {name:24s} differs in: {', '.join(which) or 'NOTHING'}")
    assert all(which for _, _, which in shown), shown


def test_the_plain_fan_from_the_first_vertex_would_break_the_invariants():
    """why step 5 of the rule is amended (tools/gen_mc_table.py): fanned from l0, 20 loops put a chord into a cube face"""
    bad = [(c, loop) for c in range(256) for loop in G.loops(c) if len(loop) > 3 and G.fan_start(loop) != 0]
    assert len(bad) == 20 and all(any(G.same_face(loop[0], loop[k]) for k in range(2, len(loop) - 1)) for _, loop in bad)
    assert sum(1 for c in range(256) for loop in G.loops(c) if len(loop) > 3) == 214
