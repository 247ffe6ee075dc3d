#!/usr/bin/env python3
"""Generate threecrate_amd/csrc/mc_table.h, the marching-cubes case table of csrc/mc.hip, from a stated rule.  This file is the only
implementation of the rule: the numpy checker (tests/mc_checker.py) and the table tests (tests/test_mc_table_cpu.py) import it.

The table is NOT the classic published table and not the reference's (threecrate-reconstruction/src/marching_cubes.rs): only the
numbering of corners and edges and the winding are the reference's.  The per-cube triangulation is this project's own.

Numbering: corners 0..7 = (0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1) (1,1,1) (0,1,1); edges 0..11 join corners
0-1 1-2 2-3 3-0 4-5 5-6 6-7 7-4 0-4 1-5 2-6 3-7; bit i of a case is set when value[corner i] < iso (the corner is inside).

Rule for case c:
  1. the crossing edges are the edges whose ends differ
  2. on each of the six faces 0, 2 or 4 edges cross.  Two are joined by a segment.  Four (two diagonal inside corners): each INSIDE
     corner is cut off on its own.  Only the face's four signs are read, so both cubes that share a face draw the same segments
  3. every crossing edge lies on two faces: the segments close into loops.  A loop starts at its smallest edge number; the loops are
     ordered by that number
  4. a loop is oriented so that its normal (right-hand rule over the edge midpoints) points to the inside: the sign of
     (Newell normal) . (sum over the loop's edges of inside end - outside end) is positive; it is never zero (asserted)
  5. a loop is fanned from its first vertex: (l0, l1, l2), (l0, l2, l3), ...
     AMENDED where that cannot hold the table's invariants: a fan chord that joins two edges of ONE cube face lies in that face, where
     the neighbouring cube may draw the same chord (an edge of four triangles in the welded mesh), and a fan triangle with all three
     edges on one face is flat in it (its normal has no component to the inside).  So the fan starts at the first vertex IN LOOP ORDER
     none of whose chords joins two edges of one cube face; the triangles are (la, la+1, la+2), (la, la+2, la+3), ... around the loop.
     Such a vertex exists for every loop (asserted); for 194 of the 214 loops of four or more edges it is l0, as the rule first said
  6. the row width is the maximum found

    python tools/gen_mc_table.py            write the header
    python tools/gen_mc_table.py --check    exit 1 when the committed header differs
"""
import os
import sys

CORNERS = ((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
# the six faces as corner cycles: x = 0, x = 1, y = 0, y = 1, z = 0, z = 1
FACES = ((0, 3, 7, 4), (1, 2, 6, 5), (0, 1, 5, 4), (3, 2, 6, 7), (0, 1, 2, 3), (4, 5, 6, 7))
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "threecrate_amd", "csrc", "mc_table.h")


def edge_of(a, b):
    return EDGES.index((a, b)) if (a, b) in EDGES else EDGES.index((b, a))


def inside(case, corner):
    return (case >> corner) & 1


def crossing_edges(case):
    return [e for e, (a, b) in enumerate(EDGES) if inside(case, a) != inside(case, b)]


def face_segments(signs, cut_inside=True):
    """The segments on one face, from its four signs alone (1 = inside, in the order of the face's corner cycle): pairs (k, l) of
    positions in the cycle, position k meaning the face's edge from corner k to corner k + 1.  cut_inside=False is the OTHER way to
    join an ambiguous face (each outside corner cut off): what the mutant of the table tests uses."""
    cross = [k for k in range(4) if signs[k] != signs[(k + 1) % 4]]
    if len(cross) == 2:
        return [(cross[0], cross[1])]
    if len(cross) == 4:
        cut = [k for k in range(4) if signs[k] == (1 if cut_inside else 0)]
        return [((k - 1) % 4, k) for k in cut]          # the two edges that meet in corner k
    assert not cross
    return []


def segments(case, face, cut_inside=True):
    """the segments of `case` on face `face` as pairs of cube edge numbers"""
    cyc = FACES[face]
    fe = [edge_of(cyc[k], cyc[(k + 1) % 4]) for k in range(4)]
    return [(fe[k], fe[l]) for k, l in face_segments([inside(case, c) for c in cyc], cut_inside)]


def midpoint2(e):
    """twice the midpoint of edge e: integers"""
    a, b = EDGES[e]
    return tuple(CORNERS[a][k] + CORNERS[b][k] for k in range(3))


def newell(loop):
    n = [0, 0, 0]
    for i, e in enumerate(loop):
        p, q = midpoint2(e), midpoint2(loop[(i + 1) % len(loop)])
        n[0] += (p[1] - q[1]) * (p[2] + q[2])
        n[1] += (p[2] - q[2]) * (p[0] + q[0])
        n[2] += (p[0] - q[0]) * (p[1] + q[1])
    return n


def inward(case, loop):
    """sum over the loop's edges of (inside end - outside end)"""
    d = [0, 0, 0]
    for e in loop:
        a, b = EDGES[e]
        i, o = (a, b) if inside(case, a) else (b, a)
        for k in range(3):
            d[k] += CORNERS[i][k] - CORNERS[o][k]
    return d


def loops(case, cut_inside=True):
    link = {e: [] for e in crossing_edges(case)}
    for f in range(6):
        for a, b in segments(case, f, cut_inside):
            link[a].append(b)
            link[b].append(a)
    assert all(len(v) == 2 for v in link.values()), case
    out, seen = [], set()
    for start in sorted(link):
        if start in seen:
            continue
        loop, prev, cur = [start], None, start
        seen.add(start)
        while True:
            a, b = link[cur]
            nxt = a if a != prev or (a == b and len(loop) == 1) else b
            if nxt == start and len(loop) > 1:
                break
            loop.append(nxt)
            seen.add(nxt)
            prev, cur = cur, nxt
        assert len(loop) >= 3 and len(set(loop)) == len(loop), (case, loop)
        n, d = newell(loop), inward(case, loop)
        s = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
        assert s != 0, (case, loop)
        if s < 0:
            loop = [loop[0]] + loop[:0:-1]
        out.append(loop)
    return out


def same_face(e, f):
    """edges e and f lie on one face of the cube"""
    return any(set(EDGES[e] + EDGES[f]) <= set(cyc) for cyc in FACES)


def fan_start(loop):
    """step 5: the first position of the loop whose fan has no chord inside a cube face"""
    for s in range(len(loop)):
        r = loop[s:] + loop[:s]
        if not any(same_face(r[0], r[k]) for k in range(2, len(r) - 1)):
            return s
    raise AssertionError(("no fan without a chord in a face", loop))


def triangles(case, cut_inside=True):
    """the triangles of one case: a list of (e0, e1, e2), cube edge numbers"""
    out = []
    for loop in loops(case, cut_inside):
        s = fan_start(loop)
        r = loop[s:] + loop[:s]
        out += [(r[0], r[k], r[k + 1]) for k in range(1, len(r) - 1)]
    return out


def table(cut_inside=True):
    """-> (rows, edge_masks): rows[c] the triangles of case c, edge_masks[c] its crossing edges as 12 bits"""
    rows = [triangles(c, cut_inside) for c in range(256)]
    masks = [sum(1 << e for e in crossing_edges(c)) for c in range(256)]
    return rows, masks


def render():
    rows, masks = table()
    width = 3 * max(len(r) for r in rows)
    total = sum(len(r) for r in rows)
    out = ["// mc_table.h -- GENERATED by tools/gen_mc_table.py, DO NOT EDIT: change the generator and run it again.",
           "// The marching-cubes case table of mc.hip.  It is generated from the rule stated in the generator (face segments that cut off",
           "// every inside corner, loops by smallest edge, fans from the first vertex that puts no chord into a cube face) and is NOT the",
           "// classic published table nor the reference's: the per-cube triangulation is where this surface deliberately differs from",
           "// marching_cubes.rs.  Corner and edge numbering and the winding (normals to the inside; case 1 = edges 0, 8, 3) are the reference's.",
           f"// Maximum row width: {width} edge numbers ({width // 3} triangles).  Triangles over the 256 cases: {total}.",
           "#pragma once",
           "#include <stdint.h>",
           "",
           "// mc.hip places the arrays in constant memory; any other reader gets plain constants",
           "#ifndef TC_MC_TABLE_STORAGE",
           "#define TC_MC_TABLE_STORAGE static const",
           "#endif",
           "",
           f"#define TC_MC_ROW {width}",
           f"#define TC_MC_MAX_TRIS {width // 3}",
           f"#define TC_MC_TOTAL_TRIS {total}",
           "",
           "// the number of triangles of every case",
           "TC_MC_TABLE_STORAGE uint8_t kMcTriCount[256] = {"]
    for r in range(0, 256, 32):
        out.append("    " + ", ".join(str(len(rows[c])) for c in range(r, r + 32)) + ",")
    out += ["};", "", "// the crossing edges of every case, bit e = edge e", "TC_MC_TABLE_STORAGE uint16_t kMcEdgeMask[256] = {"]
    for r in range(0, 256, 16):
        out.append("    " + ", ".join("0x%03x" % masks[c] for c in range(r, r + 16)) + ",")
    out += ["};", "", "// the triangles of every case: three cube edge numbers each, the row padded with 255", "TC_MC_TABLE_STORAGE uint8_t kMcTris[256][TC_MC_ROW] = {"]
    for c in range(256):
        flat = [e for t in rows[c] for e in t]
        flat += [255] * (width - len(flat))
        out.append("    {" + ", ".join("%3d" % e for e in flat) + "},")
    out += ["};", ""]
    return "\n".join(out)


def main(argv):
    text = render()
    if "--check" in argv:
        return 0 if open(HEADER).read() == text else 1
    with open(HEADER, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
