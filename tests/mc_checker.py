"""numpy checker of include/threecrate_hip_mc.h (test infrastructure): a literal, vectorised restatement of the header's pinned rules in
f32, one rounding per operation -- both vertex modes, both layouts, the normals.  The case table is imported from the generator
(tools/gen_mc_table.py), which is the only implementation of the table's rule.

marching_cubes(...) -> (vertices (n, 3) f32, normals (n, 3) f32 or None, faces (m, 3) uint32).

`mutant` names one deliberate deviation (tests/test_mc_table_cpu.py shows that each one is visible on a named case):
    "le"             <= instead of < in the case             "no_half"        t without the 0.5 branch
    "weld_reversed"  welded vertices from the upper end       "normals_plus"   normals not negated
    "bound_gt"       the sample's bound > instead of >=       "other_order"    cube order of the other layout
    "no_mask"        the mask ignored                         "other_ambiguous"  ambiguous faces joined the other way
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import gen_mc_table as G     # noqa: E402

F = np.float32
CORNERS = np.array(G.CORNERS, np.int64)
EDGES = np.array(G.EDGES, np.int64)
Z_FASTEST, X_FASTEST = 0, 1
LAYOUTS = {"z_fastest": Z_FASTEST, "x_fastest": X_FASTEST}


def _tables(cut_inside=True):
    rows, masks = G.table(cut_inside)
    tri = np.full((256, max(len(r) for r in rows), 3), -1, np.int64)
    for c, r in enumerate(rows):
        for k, t in enumerate(r):
            tri[c, k] = t
    return tri, np.array([len(r) for r in rows], np.int64), np.array(masks, np.int64)


_TABLES = {True: _tables(True), False: _tables(False)}


def as_xyz(flat, dims, layout):
    """the flat array of `layout` as a view indexed [x, y, z]"""
    nx, ny, nz = dims
    flat = np.asarray(flat).reshape(-1)
    return flat.reshape(nx, ny, nz) if layout == Z_FASTEST else flat.reshape(nz, ny, nx).transpose(2, 1, 0)


def voxel_index(x, y, z, dims, layout):
    nx, ny, nz = dims
    return (x * ny + y) * nz + z if layout == Z_FASTEST else (z * ny + y) * nx + x


def _sample(V, dims, vs, org, q, bound_gt=False):
    """sample_grid_at_world_position for the points q (n, 3)"""
    g = [(q[:, k] - org[k]) / vs[k] for k in range(3)]
    lim = [F(dims[k] - 1) for k in range(3)]
    out = np.zeros(len(q), bool)
    for k in range(3):
        out |= (g[k] < F(0.0)) | ((g[k] > lim[k]) if bound_gt else (g[k] >= lim[k]))
    i0, i1, f = [], [], []
    for k in range(3):
        fl = np.floor(np.where(out, F(0.0), g[k]))
        a = np.clip(fl.astype(np.int64), 0, dims[k] - 1)
        i0.append(a)
        i1.append(np.minimum(a + 1, dims[k] - 1))
        f.append(g[k] - a.astype(F))
    (x0, y0, z0), (x1, y1, z1), (fx, fy, fz) = i0, i1, f
    ox, oy, oz = F(1.0) - fx, F(1.0) - fy, F(1.0) - fz
    v00 = V[x0, y0, z0] * ox + V[x1, y0, z0] * fx
    v10 = V[x0, y1, z0] * ox + V[x1, y1, z0] * fx
    v01 = V[x0, y0, z1] * ox + V[x1, y0, z1] * fx
    v11 = V[x0, y1, z1] * ox + V[x1, y1, z1] * fx
    v0 = v00 * oy + v10 * fy
    v1 = v01 * oy + v11 * fy
    return np.where(out, F(0.0), v0 * oz + v1 * fz).astype(F)


def normals_at(V, dims, vs, org, p, plus=False, bound_gt=False):
    """compute_gradient_at_position for the points p (n, 3)"""
    delta = F(0.001)
    grad = []
    with np.errstate(all="ignore"):
        for k in range(3):
            qp, qn = p.copy(), p.copy()
            qp[:, k] = p[:, k] + delta
            qn[:, k] = p[:, k] - delta
            grad.append((_sample(V, dims, vs, org, qp, bound_gt) - _sample(V, dims, vs, org, qn, bound_gt)) / (F(2.0) * delta))
        gx, gy, gz = grad
        n = np.sqrt((gx * gx + gy * gy) + gz * gz)
        ok = n > F(1e-6)
        s = F(1.0) if plus else F(-1.0)
        out = np.stack([np.where(ok, s * (gx / n), F(0.0)), np.where(ok, s * (gy / n), F(0.0)), np.where(ok, s * (gz / n), F(1.0))], axis=1)
    return out.astype(F)


def _interpolate(V, vs, org, ca, cb, iso, no_half=False):
    """interpolate_vertex from the voxels ca (n, 3) to cb (n, 3)"""
    va, vb = V[ca[:, 0], ca[:, 1], ca[:, 2]], V[cb[:, 0], cb[:, 1], cb[:, 2]]
    with np.errstate(all="ignore"):
        d = vb - va
        t = (iso - va) / d
        if not no_half:
            t = np.where(np.abs(d) < F(1e-6), F(0.5), t)
        p = np.empty((len(ca), 3), F)
        for k in range(3):
            pa = org[k] + ca[:, k].astype(F) * vs[k]
            pb = org[k] + cb[:, k].astype(F) * vs[k]
            p[:, k] = pa + t.astype(F) * (pb - pa)
    return p


def marching_cubes(values, dims, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), iso_level=0.0, normals=True, weld=False, valid=None,
                   layout=Z_FASTEST, mutant=None):
    layout = LAYOUTS.get(layout, layout)
    dims = tuple(int(d) for d in dims)
    vs, org, iso = [F(v) for v in voxel_size], [F(o) for o in origin], F(iso_level)
    tri, ntri, masks = _TABLES[mutant != "other_ambiguous"]
    empty = (np.zeros((0, 3), F), np.zeros((0, 3), F) if normals else None, np.zeros((0, 3), np.uint32))
    if min(dims) < 2:
        return empty
    V = as_xyz(np.asarray(values, F), dims, layout)
    usable = np.isfinite(V)
    if valid is not None and mutant != "no_mask":
        usable = usable & (as_xyz(np.asarray(valid), dims, layout) != 0)
    nx, ny, nz = dims
    inside = (V <= iso) if mutant == "le" else (V < iso)
    case = np.zeros((nx - 1, ny - 1, nz - 1), np.int64)
    ok = np.ones((nx - 1, ny - 1, nz - 1), bool)
    for k, (dx, dy, dz) in enumerate(G.CORNERS):
        sl = (slice(dx, nx - 1 + dx), slice(dy, ny - 1 + dy), slice(dz, nz - 1 + dz))
        case |= inside[sl].astype(np.int64) << k
        ok &= usable[sl]
    ok &= (case != 0) & (case != 255)
    cx, cy, cz = np.nonzero(ok)
    order_layout = layout if mutant != "other_order" else 1 - layout
    order = np.argsort(voxel_index(cx, cy, cz, dims, order_layout), kind="stable")
    base = np.stack([cx[order], cy[order], cz[order]], axis=1)          # the emitting cubes, in order
    if len(base) == 0:
        return empty
    cc = case[base[:, 0], base[:, 1], base[:, 2]]
    # the triangles: (cube, k) in order
    t_cube = np.repeat(np.arange(len(base)), ntri[cc])
    t_first = np.concatenate([[0], np.cumsum(ntri[cc])])
    t_k = np.arange(len(t_cube)) - t_first[t_cube]
    t_edges = tri[cc[t_cube], t_k]                                      # (m, 3) cube edge numbers
    if not weld:
        mask = masks[cc]
        has = ((mask[:, None] >> np.arange(12)) & 1).astype(bool)             # (cubes, 12): edge e crosses
        vcount = has.sum(axis=1)
        first = np.concatenate([[0], np.cumsum(vcount)])
        v_cube, v_edge = np.nonzero(has)                                      # row-major: by cube, then by edge number
        ca = base[v_cube] + CORNERS[EDGES[v_edge, 0]]
        cb = base[v_cube] + CORNERS[EDGES[v_edge, 1]]
        rank = np.cumsum(has, axis=1) - has                                   # crossing edges in front of edge e
        faces = first[t_cube][:, None] + rank[t_cube[:, None], t_edges]
    else:
        a = base[t_cube][:, None, :] + CORNERS[EDGES[t_edges, 0]]       # (m, 3, 3)
        b = base[t_cube][:, None, :] + CORNERS[EDGES[t_edges, 1]]
        lower = np.minimum(a, b)
        axis = np.argmax(a != b, axis=2)
        key = 3 * voxel_index(lower[..., 0], lower[..., 1], lower[..., 2], dims, layout) + axis
        uniq, first_at, inv = np.unique(key.reshape(-1), return_index=True, return_inverse=True)
        faces = inv.reshape(-1, 3)
        ca = lower.reshape(-1, 3)[first_at]
        cb = ca.copy()
        cb[np.arange(len(cb)), axis.reshape(-1)[first_at]] += 1
        if mutant == "weld_reversed":
            ca, cb = cb, ca
    p = _interpolate(V, vs, org, ca, cb, iso, no_half=mutant == "no_half")
    nrm = normals_at(V, dims, vs, org, p, plus=mutant == "normals_plus", bound_gt=mutant == "bound_gt") if normals else None
    return p, nrm, faces.astype(np.uint32)
