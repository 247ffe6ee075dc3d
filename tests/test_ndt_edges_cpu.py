"""NDT at its edges without a GPU: what every case of tests/ndt_cases.py is there for, proved on the checker (tests/ndt_checker.py) alone.
The extended checker gives the answers of its predecessor, of which a literal copy stands below (parent_*); the preconditions of every
family (key shares, bit totals, table kinds, run lengths, condition numbers, hit counts, loop decisions); the floor of the voxel map's
tight bound against exact rationals; and the mutant table -- every mutant must be told apart by a named case that
tests/test_gpu_ndt_edges.py runs (`python tests/test_ndt_edges_cpu.py` prints the table)."""
import ctypes as C_
import os
import sys
import time
from fractions import Fraction as Fr

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from threecrate_amd import _lib
from tests import ndt_cases as C
from tests import ndt_checker as NC

F = np.float32


# ---- the checker's functions as they were before key_dtype, rules and the wide lookup: a literal copy, names prefixed ----
def parent_keys_of(p, res, dtype):
    """(floor(x / res), ...) as i32: true division, floor (:61-67)"""
    return np.floor(np.asarray(p, dtype) / dtype(res)).astype(np.int64)


def parent_build(target, res, min_points, dtype=np.float32):
    """-> keys (V, 3) int64 ascending by (kx, ky, kz), counts (V,), mean (V, 3), inv_cov (V, 3, 3), all sums in input order.
    A point with a non-finite coordinate takes no part (the header's deviation)."""
    t = np.asarray(target, np.float32).reshape(-1, 3)
    t = t[np.isfinite(t).all(axis=1)].astype(dtype)
    k = parent_keys_of(t, res, dtype)
    order = np.lexsort((k[:, 2], k[:, 1], k[:, 0]))             # stable: a voxel keeps input order
    ks = k[order]
    heads = np.r_[True, (ks[1:] != ks[:-1]).any(axis=1)] if len(ks) else np.zeros(0, bool)
    starts = np.r_[np.nonzero(heads)[0], len(ks)]
    keys, counts, means, invs = [], [], [], []
    for s, e in zip(starts[:-1], starts[1:]):
        if e - s < min_points:
            continue
        pts = t[order[s:e]]
        n = dtype(e - s)
        mean = (np.cumsum(pts, axis=0, dtype=dtype)[-1] / n).astype(dtype)
        d = (pts - mean).astype(dtype)
        cov = np.cumsum((d[:, :, None] * d[:, None, :]).astype(dtype), axis=0, dtype=dtype)[-1] / n
        cov = (cov + np.eye(3, dtype=dtype) * dtype(1e-4)).astype(dtype)
        inv = NC._inverse3(cov, dtype)
        if inv is None:
            continue
        keys.append(ks[s]); counts.append(e - s); means.append(mean); invs.append(inv)
    v = len(keys)
    return (np.array(keys, np.int64).reshape(v, 3), np.array(counts, np.int64), np.array(means, dtype).reshape(v, 3),
            np.array(invs, dtype).reshape(v, 3, 3))


def parent__pack(keys, lo, dims):
    r = keys - lo
    return (r[:, 0] * dims[1] + r[:, 1]) * dims[2] + r[:, 2]


def parent_evaluate(source, grid, pose, res, dtype=np.float32):
    """-> score, g (6), H (6, 6), record {keys, hit (mask), dist (per point: the smallest distance of a coordinate from a voxel face, in units
    of the resolution), face (its minimum)}"""
    vkeys, _, means, invs = grid
    s = np.asarray(source, np.float32).astype(dtype)
    p = NC.apply(pose, s, dtype)
    R = NC.rotation_matrix(np.asarray(pose, dtype)[:4], dtype)
    rs = np.stack([(R[r, 0] * s[:, 0] + R[r, 1] * s[:, 1]) + R[r, 2] * s[:, 2] for r in range(3)], axis=1).astype(dtype)
    ok = np.isfinite(p).all(axis=1)
    u = np.where(ok[:, None], p, dtype(0.5) * dtype(res)) / dtype(res)
    keys = np.floor(u).astype(np.int64)
    frac = u - np.floor(u)
    dist = np.where(ok[:, None], np.minimum(frac, 1 - frac), 0.5).min(axis=1)      # per point, in units of the resolution
    face = float(dist.min())
    lo, hi = vkeys.min(axis=0), vkeys.max(axis=0)
    dims = hi - lo + 1
    inside = ok & ((keys >= lo) & (keys <= hi)).all(axis=1)
    packed_v = parent__pack(vkeys, lo, dims)                           # ascending, as the voxels are
    hit = np.zeros(len(s), bool)
    vox = np.zeros(len(s), np.int64)
    if inside.any():
        pk = parent__pack(keys[inside], lo, dims)
        pos = np.searchsorted(packed_v, pk)
        pos = np.minimum(pos, len(packed_v) - 1)
        found = packed_v[pos] == pk
        idx = np.nonzero(inside)[0]
        hit[idx[found]] = True
        vox[idx[found]] = pos[found]
    rec = {"keys": keys, "hit": hit, "face": face, "dist": dist}
    if not hit.any():
        return dtype(0), np.zeros(6, dtype), np.zeros((6, 6), dtype), rec
    p, rs, v = p[hit], rs[hit], vox[hit]
    A = invs[v]                                                  # (m, 3, 3)
    d = (p - means[v]).astype(dtype)
    c = np.stack([(A[:, r, 0] * d[:, 0] + A[:, r, 1] * d[:, 1]) + A[:, r, 2] * d[:, 2] for r in range(3)], axis=1).astype(dtype)
    e = np.exp(dtype(-0.5) * ((d[:, 0] * c[:, 0] + d[:, 1] * c[:, 1]) + d[:, 2] * c[:, 2])).astype(dtype)
    m = len(p)
    zero, one = np.zeros(m, dtype), np.ones(m, dtype)
    # J (3 x 6) by entries: [I | (0, -rs.z, rs.y), (rs.z, 0, -rs.x), (-rs.y, rs.x, 0)] as columns
    J = [[one, zero, zero, zero, rs[:, 2], -rs[:, 1]],
         [zero, one, zero, -rs[:, 2], zero, rs[:, 0]],
         [zero, zero, one, rs[:, 1], -rs[:, 0], zero]]
    gv = np.stack([(J[0][i] * c[:, 0] + J[1][i] * c[:, 1]) + J[2][i] * c[:, 2] for i in range(6)], axis=1).astype(dtype)
    T = [[(J[0][i] * A[:, 0, j] + J[1][i] * A[:, 1, j]) + J[2][i] * A[:, 2, j] for j in range(3)] for i in range(6)]     # J^T A
    Hc = np.stack([np.stack([(T[i][0] * J[0][j] + T[i][1] * J[1][j]) + T[i][2] * J[2][j] for j in range(6)], axis=1) for i in range(6)], axis=1).astype(dtype)
    score = np.cumsum(e, dtype=dtype)[-1]
    g = np.cumsum((e[:, None] * gv).astype(dtype), axis=0, dtype=dtype)[-1]
    H = np.cumsum((e[:, None, None] * Hc).astype(dtype), axis=0, dtype=dtype)[-1]
    return dtype(score), g.astype(dtype), H.astype(dtype), rec


def parent_register(source, target, init=None, resolution=1.0, step_size=0.1, max_iterations=35, epsilon=1e-4, min_points_per_voxel=5, dtype=np.float32,
             grid=None):
    """-> dict(pose, score, iterations, converged, n_voxels, n_hits, evals: the records of the evaluations, deltas: the applied updates)"""
    source = np.asarray(source, np.float32).reshape(-1, 3)
    target = np.asarray(target, np.float32).reshape(-1, 3)
    if len(source) == 0:
        raise NC.NdtError("Source point cloud is empty")
    if len(target) < min_points_per_voxel:
        raise NC.NdtError("Target point cloud has too few points for NDT voxel grid")
    if grid is None:
        grid = parent_build(target, resolution, min_points_per_voxel, dtype)
    if len(grid[0]) == 0:
        raise NC.NdtError("NDT voxel grid is empty — try a larger resolution or lower min_points_per_voxel")
    pose = np.array(NC.IDENTITY if init is None else init, dtype)
    out = {"converged": False, "iterations": 0, "score": dtype(0), "n_voxels": len(grid[0]), "n_hits": 0, "evals": [], "deltas": []}
    for it in range(max_iterations):
        out["iterations"] = it + 1
        score, g, H, rec = parent_evaluate(source, grid, pose, resolution, dtype)
        out["score"], out["n_hits"] = score, int(rec["hit"].sum())
        out["evals"].append(rec)
        delta = NC.lu_solve(H + np.eye(6, dtype=dtype) * dtype(1e-6), -g, dtype)
        if delta is None:
            break
        norm = np.sqrt(np.cumsum(delta * delta, dtype=dtype)[-1])
        if norm > dtype(step_size):
            delta = (delta * (dtype(step_size) / norm)).astype(dtype)
        out["deltas"].append(delta)
        if np.sqrt(np.cumsum(delta * delta, dtype=dtype)[-1]) < dtype(epsilon):
            out["converged"] = True
            break
        pose = NC.compose(NC.euler_quaternion(delta[3], delta[4], delta[5], dtype), delta[:3], pose, dtype)
    out["pose"] = pose
    return out


# ---- the extended checker gives the parent's answers ----------------------------------------------------------------------------------
def _same(x, y):
    x, y = np.asarray(x), np.asarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_build_is_bit_equal_to_the_parents(dtype):
    clouds = [(C.lattice_cloud(v), 1.0) for v in (1, 255, 256, 257)] + [(NC.surface_pair(4096, 2048, 0.5)[1], 0.5), (NC.surface(20000, 1), 0.25)]
    for cloud, res in clouds:
        for x, y in zip(NC.build(cloud, res, 5, dtype), parent_build(cloud, res, 5, dtype)):
            assert _same(x, y)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nt,ns,res,iters", [(4096, n, 0.5, 1) for n in (1, 63, 64, 65, 255, 256, 257, 4096, 4097)] + [(4096, 2048, 0.5, 35), (20000, 20000, 0.25, 1)])
def test_register_is_bit_equal_to_the_parents(dtype, nt, ns, res, iters):
    src, tgt, init = NC.surface_pair(nt, ns, res, **(dict(max_iterations=35) if iters == 35 else {}))
    a = NC.register(src, tgt, init, resolution=res, max_iterations=iters, dtype=dtype)
    b = parent_register(src, tgt, init, resolution=res, max_iterations=iters, dtype=dtype)
    assert (a["iterations"], a["converged"], a["n_voxels"], a["n_hits"]) == (b["iterations"], b["converged"], b["n_voxels"], b["n_hits"])
    assert _same(a["pose"], b["pose"]) and _same(a["score"], b["score"]) and all(_same(x, y) for x, y in zip(a["deltas"], b["deltas"]))
    assert all(_same(x["keys"], y["keys"]) and _same(x["hit"], y["hit"]) and _same(x["dist"], y["dist"]) for x, y in zip(a["evals"], b["evals"]))


def test_keys_saturate_as_the_cast_does():
    p = np.array([[3e9, -3e9, 2147483520.0], [2147483648.0, -2147483648.0, -2147483904.0], [3e38, -3e38, 0.0]], F)
    assert NC.keys_of(p, 1.0, F).tolist() == [[NC.I32_MAX, NC.I32_MIN, 2147483520], [NC.I32_MAX, NC.I32_MIN, NC.I32_MIN], [NC.I32_MAX, NC.I32_MIN, 0]]
    assert NC.keys_of(p, 1e-30, F).tolist()[0] == [NC.I32_MAX, NC.I32_MIN, NC.I32_MAX]          # x / res overflows to +-inf first


def test_the_lookup_holds_a_key_box_of_2_to_the_64_cells():
    src, tgt, init = C.case_input(C.by_id("saturated-bits64"))
    bits, cells = C.key_box_bits(tgt, 1.0)
    assert sum(bits) == 64 and cells >= 2.0 ** 63
    b = C.ref_runs(C.by_id("saturated-bits64"))[1]
    assert b["n_hits"] == len(src) - 1 and b["evals"][0]["hit"][-1] == False and b["evals"][0]["hit"][-6:-1].all()       # the far probes hit


# ---- preconditions, per family ----------------------------------------------------------------------------------------------------------
def _key_share(p, res, rules=None, dtype=F):
    return float((NC.keys_of(p, res, dtype, rules) != NC.keys_of(p, res, F)).any(axis=1).mean())


@pytest.mark.parametrize("res", C.FACE_RES)
def test_faces_sites_tell_the_key_rules_apart(res):
    """the share of points whose key differs from the header's: f64 division (of the f64 resolution, as the checker's f64 run does, and of
    the f32 one, as a device would), the reciprocal, truncation.  One coordinate of every point is on a face, the other two are not."""
    p = C.faces_cloud(res)
    assert len(p) == 3645 and np.isfinite(p).all()
    shares = {m: _key_share(p, res, MUTANT_RULES[m]) for m in ("keys_f64", "keys_reciprocal", "trunc")}
    shares["f64 checker"] = _key_share(p, res, None, np.float64)
    print(f"faces res {res:.4f}: " + ", ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    if res == 0.5:
        assert shares["keys_f64"] == shares["keys_reciprocal"] == shares["f64 checker"] == 0.0
    else:
        assert shares["keys_f64"] >= 0.05 and shares["f64 checker"] >= 0.05
        # per point, one coordinate of three on a face: 3.7 / 7.0 / 9.9 / 4.1 % measured; the floor of each is what the mutant table rests on
        assert shares["keys_reciprocal"] >= {0.1: 0.035, 0.3: 0.065, 1.0 / 3.0: 0.09, 0.7: 0.04}[res]
    assert shares["trunc"] >= 0.3                       # every negative non-integer quotient
    g = C.ref_voxels(C.by_id(f"faces-res{C._res_name(res)}"))
    assert g[0][:, 0].min() in (-C.FACE_J - 1, -C.FACE_J) and g[0][:, 0].max() == C.FACE_J and g[1].sum() == len(p)


@pytest.mark.parametrize("c", C.of("register", "faces_source"), ids=C.case_id)
def test_faces_source_is_exact_and_every_cell_is_there(c):
    src, tgt, init = C.case_input(c)
    res = c.params["resolution"]
    assert np.array_equal(NC.keys_of(tgt, res, F), NC.keys_of(tgt, res, np.float64))            # the target is nowhere near a face
    p32, p64 = NC.apply(init, src, F), NC.apply(init, src.astype(np.float64), np.float64)
    assert np.array_equal(p32.astype(np.float64), p64)                                          # the transformed positions are exact
    if init[4:].any():
        q = p64 / C.FACE_GRID
        assert np.array_equal(q, np.round(q)) and (np.abs(p64[:, 0] / res - np.round(p64[:, 0] / res)) == 0).sum() >= 81
    a, b = C.ref_runs(c)
    assert a["n_hits"] == b["n_hits"] == len(src) and np.array_equal(a["evals"][0]["keys"], b["evals"][0]["keys"])
    assert b["evals"][0]["face"] == 0.0                                                         # some point sits on a face


def test_saturated_bit_totals_and_tables():
    for which, bits in (("pos", [32, 1, 1]), ("neg", [32, 1, 1]), ("both", [32, 1, 1]), ("bits64", [31, 31, 2]), ("bits65", [31, 31, 3]), ("xyz", [31, 31, 32])):
        src, tgt = C.saturated(which)
        got, cells = C.key_box_bits(tgt, 1.0)
        assert got == bits and cells > C.DENSE_CELLS, which
    assert sum(C.key_box_bits(C.saturated("bits64")[1], 1.0)[0]) == 64 and sum(C.key_box_bits(C.saturated("bits65")[1], 1.0)[0]) == 65
    k = NC.keys_of(C.saturated("both")[1], 1.0, F)
    assert k[:, 0].min() == NC.I32_MIN and k[:, 0].max() == NC.I32_MAX and k[:, 0].max() - k[:, 0].min() + 1 == 2 ** 32
    for c in C.of("voxels", "saturated"):
        g = C.ref_voxels(c)
        far = np.abs(g[0]).max(axis=1) > 2 ** 30
        cond = C.voxel_conds(g)
        assert far.sum() == {"pos-map": 1, "neg-map": 1, "both-map": 2, "bits64-map": 2}[c.name] and (g[1][far] == 6).all()
        assert (cond[far] > 1e9).all() and (cond[~far] <= C.COND_MAX).all() and np.isfinite(g[3]).all()
    for c in C.of("register", "saturated"):
        a, b = C.ref_runs(c)
        e = b["evals"][0]
        far = np.abs(np.asarray(C.case_input(c)[0])).max(axis=1) > 1e9
        assert far.sum() >= 2 and e["hit"][far].all() and a["n_hits"] == b["n_hits"] == len(far) - 1
        # the far hits score nothing: the score is that of the near points alone
        near_only = NC.register(C.case_input(c)[0][~far], C.case_input(c)[1], None, max_iterations=1, dtype=np.float64, key_dtype=F)
        assert near_only["score"] == b["score"] and np.isfinite(b["pose"]).all()


def test_long_source_sizes_reach_the_stride_and_hits_are_not_ns():
    t0 = time.perf_counter()
    hits = []
    for c in C.of("register", "long_source"):
        ns = len(C.case_input(c)[0])
        a, b = C.ref_runs(c)
        assert (a["iterations"], a["converged"], a["n_hits"]) == (b["iterations"], b["converged"], b["n_hits"]) == (1, False, b["n_hits"])
        assert 0.5 * ns < b["n_hits"] < 0.7 * ns and b["n_voxels"] == 363
        hits.append((ns, b["n_hits"]))
    took = time.perf_counter() - t0
    print(f"long_source: (ns, hits) {hits}; the checker's ten runs took {took:.1f} s")
    assert [n for n, _ in hits] == [C.EVAL_SPAN - 1, C.EVAL_SPAN, C.EVAL_SPAN + 1, C.EVAL_SPAN + 257, 2 * C.EVAL_SPAN + 1]
    assert len({h for _, h in hits}) >= 4


def test_many_long_runs_run_lengths():
    g = C.ref_voxels(C.by_id("many_long_runs-1100x129"))
    assert (g[1] > C.LONG_RUN).sum() == C.MANY_LONG > 1024 and (g[1] == 6).sum() == C.MANY_SHORT and len(g[0]) == 1400
    assert len(C.many_long_runs()) // C.LONG_RUN + 1 >= C.MANY_LONG                               # the list holds them
    assert C.ref_voxels(C.by_id("many_long_runs-single"))[1].tolist() == list(C.SINGLE_RUNS)


def test_degenerate_voxels_are_what_they_say():
    keys, counts, mean, inv = C.ref_voxels(C.by_id("degenerate-voxels"))
    assert keys.tolist() == [[-3, 1, -2], [0, 0, 0], [2, 0, 0], [4, 0, 0]] and counts.tolist() == [5, 5, 5, 6]
    for v in (0, 1):
        assert np.array_equal(inv[v], np.diag(np.diag(inv[v]))) and np.abs(np.diag(inv[v]) / 1e4 - 1).max() < 1e-12
        assert np.array_equal(mean[v].astype(F), C.degenerate()[np.nonzero((NC.keys_of(C.degenerate(), 1.0, F) == keys[v]).all(axis=1))[0][0]])
    assert abs(inv[2][1, 1] / 1e4 - 1) < 1e-12 and inv[2][0, 0] < 1e3 and abs(inv[3][2, 2] / 1e4 - 1) < 1e-12
    for m in (0, 1):
        keys, counts, mean, inv = C.ref_voxels(C.by_id(f"degenerate-scattered-min{m}"))
        assert len(keys) == len(C.scattered()) == 500 and (counts == 1).all()
        order = np.lexsort(NC.keys_of(C.scattered(), 1.0, F).T[::-1])
        assert np.array_equal(mean.astype(F), C.scattered()[order])
    with pytest.raises(NC.NdtError, match="too few points"):
        NC.register(C.scattered(), C.scattered(), min_points_per_voxel=501)


def own_home_slots(target, res):
    """the hash table of ndt.hip for a map of one voxel per point: capacity, and each key's home slot (ndt_pack + ndt_hash in uint64)"""
    k = NC.keys_of(target, res, F)
    lo, dims = k.min(axis=0), k.max(axis=0) - k.min(axis=0) + 1
    bits = [C.bits_for(int(d) - 1) for d in dims]
    r = (k - lo).astype(np.uint64)
    key = (r[:, 0] << np.uint64(bits[1] + bits[2])) | (r[:, 1] << np.uint64(bits[2])) | r[:, 2]
    cap = 2
    while cap < 2 * len(k):
        cap <<= 1
    with np.errstate(over="ignore"):
        h = key ^ (key >> np.uint64(30)); h = h * np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(27); h = h * np.uint64(0x94D049BB133111EB); h ^= h >> np.uint64(31)
    return cap, (h & np.uint64(0xFFFFFFFF)) & np.uint64(cap - 1)


@pytest.mark.parametrize("spread", [False, True])
def test_own_points_keys_are_distinct_and_the_table_is_the_intended_one(spread):
    src, tgt = C.own_points(spread)
    k, ks = NC.keys_of(tgt, C.OWN_RES, F), NC.keys_of(src, C.OWN_RES, F)
    assert np.array_equal(k, NC.keys_of(tgt, C.OWN_RES, np.float64)) and len(np.unique(k, axis=0)) == C.OWN_N == len(tgt) and len(src) == 2 * C.OWN_N
    cells = np.prod((k.max(axis=0) - k.min(axis=0) + 1).astype(np.float64))
    assert (cells > C.DENSE_CELLS) == spread and (not spread or own_home_slots(tgt, C.OWN_RES)[0] == 65536)
    assert ((ks >= k.min(axis=0)) & (ks <= k.max(axis=0))).all()                                  # every source point is inside the key box
    occupied = {tuple(r) for r in k.tolist()}
    assert all(tuple(r) in occupied for r in ks[:C.OWN_N].tolist()) and not any(tuple(r) in occupied for r in ks[C.OWN_N:].tolist())
    assert set(map(tuple, src[:C.OWN_N].view(np.uint32).tolist())) == set(map(tuple, tgt.view(np.uint32).tolist()))


def test_nonfinite_source_rows_and_their_twin():
    c = C.by_id("nonfinite_source-rows")
    src, tgt, init = C.case_input(c)
    twin = C.nonfinite_source(True)[0]
    rows = [r for r, _ in C.NONFINITE_ROWS]
    assert rows == [0, 1, len(src) // 2, len(src) - 1] and not np.isfinite(src[rows]).all(axis=1)[[0, 2, 3]].any() and np.isfinite(twin).all()
    assert np.array_equal(np.delete(src, rows, axis=0), np.delete(twin, rows, axis=0))
    g = NC.build(tgt, 0.5, 5, np.float64, key_dtype=F)
    assert [0, 0, 0] in g[0].tolist() and (twin[rows] / 0.5 > g[0].max() + 50).all()
    kw = C.loop_of(c)
    b, bt = C.ref_runs(c)[1], NC.register(twin, tgt, init, dtype=np.float64, key_dtype=F, **kw)
    assert b["n_hits"] == bt["n_hits"] and _same(b["pose"], bt["pose"]) and b["score"] == bt["score"] and b["iterations"] == C.NONFINITE_ITERS
    assert not any(e["hit"][rows].any() for e in b["evals"])
    with np.errstate(over="ignore", invalid="ignore"):
        p = NC.apply(init, src[rows], F)
    assert np.isfinite(p[1]).all() and NC.keys_of(p[1:2], 0.5, F)[0, 1] == NC.I32_MAX       # the 3e38 row stays finite: its key saturates, a miss by the box


@pytest.mark.parametrize("i", range(len(C.SHIFTS)))
def test_shifted_pairs_are_cleaned_for_the_loops_they_run(i):
    """every multi-step input is cleaned for its own loop: the f32 run and the yardstick see the same keys in every evaluation, no coordinate
    within FACE_MARGIN of a face in the yardstick's f64 positions.  At 2^10 the cleaning for 35 iterations runs out of points (so 3 and 5
    there); at 2^13 the default run is a case.  Neither arithmetic converges this far out -- the update turns about the origin -- and the
    pose budget is whole units from the lever arm of the translation: what binds the device there is the exact n_hits, iterations, converged"""
    off = C.SHIFTS[i]
    src, tgt, init = C.shifted(off)
    assert np.abs(tgt[:, :2] - np.asarray(off, F)[:2]).max() <= 2.0 and not np.array_equal(init, NC.start_pose())
    assert C.SHIFT_LOOPS == ((3, 5), (5, 35))
    for its in (1,) + C.SHIFT_LOOPS[i]:
        c = [c for c in C.of("register", "shifted") if c.input[1] == off and (c.input[2:] or (1,))[0] == its][0]
        a, b = C.ref_runs(c)
        full = NC.register(*C.case_input(c), dtype=np.float64, **C.loop_of(c))        # f64 keys: the margin is of the exact positions
        assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"]) == (full["iterations"], full["converged"]) == (its, False)
        assert len(b["evals"]) == its and min(e["face"] for e in full["evals"]) >= NC.FACE_MARGIN
        assert all(np.array_equal(x["keys"], y["keys"]) and np.array_equal(x["keys"], z["keys"]) for x, y, z in zip(a["evals"], b["evals"], full["evals"]))
        assert a["n_hits"] == b["n_hits"] > 1900
        print(f"{C.case_id(c)}: {its} iterations, hits {b['n_hits']}, the reference's f32-to-f64 distance {NC.distances(a, b)}")
    if i == 0:
        with pytest.raises(AssertionError, match="ran out of replacement points"):
            NC.surface_pair(4096, 2048, 0.5, offset=off, max_iterations=35)


@pytest.mark.parametrize("c", [c for c in C.of("register") if c.params["expect"] == "budget"], ids=C.case_id)
def test_budgeted_runs_take_the_same_loop_decisions(c):
    a, b = C.ref_runs(c)
    assert (a["iterations"], a["converged"], a["n_voxels"], a["n_hits"]) == (b["iterations"], b["converged"], b["n_voxels"], b["n_hits"])
    assert all(np.array_equal(x["keys"], y["keys"]) for x, y in zip(a["evals"], b["evals"])) and 0 < b["n_hits"]
    bp, bs = C.budget(c)
    print(f"{C.case_id(c)}: hits {b['n_hits']} of {len(C.case_input(c)[0])}, budget pose {bp:.2e}, score {bs:.2e}")
    assert 0 < bp < np.inf and 0 < bs < np.inf
    if c.family != "shifted":                                   # (there the lever arm of the translation makes the rule's budget units wide)
        assert bp < 1e-3 and bs < 1e-3


# ---- the tight bound's floor, against exact rationals -----------------------------------------------------------------------------------
def exact_voxel(pts):
    """mean and inverse of cov + 1e-4 I (the f64 constant) of float32 points, in rationals"""
    P = [[Fr(float(x)) for x in p] for p in pts]
    n = len(P)
    m = [sum(p[a] for p in P) / n for a in range(3)]
    c = [[sum((p[a] - m[a]) * (p[b] - m[b]) for p in P) / n + (Fr(1e-4) if a == b else 0) for b in range(3)] for a in range(3)]
    (xx, xy, xz), (_, yy, yz), (_, _, zz) = c
    adj = [yy * zz - yz * yz, xz * yz - xy * zz, xy * yz - xz * yy, xx * zz - xz * xz, xy * xz - xx * yz, xx * yy - xy * xy]
    det = xx * adj[0] + xy * adj[1] + xz * adj[2]
    return [float(v) for v in m], [float(a / det) for a in adj]


@pytest.mark.parametrize("c", [c for c in C.of("voxels") if c.params[2]], ids=C.case_id)
def test_tight_bound_applies_and_its_floor_holds(c):
    """cond <= 1e4 on every voxel of the family, and the f64 yardstick is within 2^-40 of the matrix's largest element of the exact inverse
    (all voxels of `degenerate`, a sample of 50 elsewhere); its mean within 2^-45 relative"""
    cloud, res = C.case_input(c)[0], c.params[0]
    g = C.ref_voxels(c)
    cond = C.voxel_conds(g)
    assert len(cond) and cond.max() <= C.COND_MAX
    k = NC.keys_of(cloud, res, F)
    pick = np.arange(len(g[0])) if c.family == "degenerate" and len(g[0]) < 50 else np.random.default_rng(0).permutation(len(g[0]))[:50]
    worst = 0.0
    for v in pick:
        pts = cloud[(k == g[0][v]).all(axis=1)]
        m, inv = exact_voxel(pts)
        got = np.array([g[3][v][i, j] for i, j in C.IU])
        worst = max(worst, np.abs(got - inv).max() / np.abs(inv).max())
        assert np.abs(g[2][v] - m).max() <= 2.0 ** -45 * max(np.abs(m).max(), 1e-30)
    print(f"{C.case_id(c)}: cond <= {cond.max():.0f}, yardstick to exact inverse {worst:.1e} of the largest element (floor {C.INV_FLOOR:.1e})")
    assert worst <= C.INV_FLOOR
    em, ei = C.voxel_excess(g[2].astype(F), np.stack([g[3][:, i, j] for i, j in C.IU], axis=1).astype(F), g)
    assert em <= 0.5 and ei <= 0.5                              # the yardstick rounded once is half an ulp away


def test_saturated_maps_are_outside_the_tight_bound_only_in_the_far_voxel():
    for c in C.of("voxels", "saturated"):
        assert not c.params[2]


# ---- mutants ----------------------------------------------------------------------------------------------------------------------------
def _wrap(f):
    return ((np.clip(np.nan_to_num(f.astype(np.float64), nan=0.0), -2.0 ** 62, 2.0 ** 62).astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.float64)


MUTANT_RULES = {                                                # a mutant of the checker: NC.RULES entries replaced
    "keys_f64": dict(key_arith=lambda x, res: x.astype(np.float64) / np.float64(res)),
    "keys_reciprocal": dict(key_arith=lambda x, res: x * (type(res)(1) / res)),
    "trunc": dict(floor=np.trunc),
    "wrap": dict(saturate=_wrap),
    "nan_keyed_zero": dict(source_scores=lambda p: np.ones(len(p), bool)),
    "count_gt_min": dict(survives=lambda count, m: count > m),
    "divisor_n_minus_1": dict(divisor=lambda n: n - 1),
    "no_regulariser": dict(regular=0.0),
}
# mutant -> (the case that tells it, how).  The last three are mutants of the device's structure, modelled here on the checker's answers.
TELLS = {
    "keys_f64": "faces-res0.3", "keys_reciprocal": "faces-resthird", "trunc": "faces-res0.5", "wrap": "saturated-pos-map",
    "nan_keyed_zero": "nonfinite_source-rows", "count_gt_min": "degenerate-voxels", "divisor_n_minus_1": "degenerate-voxels",
    "no_regulariser": "degenerate-voxels", "source_cut_at_span": "long_source-ns262145", "long_list_cut_at_1024": "many_long_runs-1100x129",
    "hash_probe_stops": "own_points-hash",
}
ALSO = {"keys_f64": ("faces_source-res0.3-identity", "faces-res0.1", "faces-resthird", "faces-res0.7"),
        "keys_reciprocal": ("faces_source-resthird-identity", "faces-res0.1", "faces-res0.3", "faces-res0.7"),
        "trunc": ("faces_source-res0.5-translated", "faces_source-res0.25-translated"), "wrap": ("saturated-neg-map", "saturated-both", "saturated-bits64"),
        "source_cut_at_span": ("long_source-ns262401", "long_source-ns524289"), "count_gt_min": ("faces-res0.1",), "divisor_n_minus_1": ("many_long_runs-single",)}


def tells(mutant, cid):
    """how the case tells the mutant from the contract, or None"""
    c = C.by_id(cid)
    rules = MUTANT_RULES.get(mutant)
    if mutant == "source_cut_at_span":
        src, tgt, init = C.case_input(c)
        b = C.ref_runs(c)[1]
        m = NC.register(src[:C.EVAL_SPAN], tgt, init, dtype=np.float64, key_dtype=F, **C.loop_of(c))
        return f"n_hits {m['n_hits']} for {b['n_hits']}" if m["n_hits"] != b["n_hits"] else None
    if mutant == "long_list_cut_at_1024":
        g = C.ref_voxels(c)
        lost = np.nonzero(g[1] > C.LONG_RUN)[0][1024:]            # whichever 1 024 of the listed runs are served, the others keep no record
        mean, inv = g[2].astype(F), np.stack([g[3][:, i, j] for i, j in C.IU], axis=1).astype(F)
        mean[lost], inv[lost] = 0, 0
        ex = C.voxel_excess(mean, inv, g)
        return f"{len(lost)} voxels without a record: {max(ex):.1e} x the bound" if len(lost) and max(ex) > 1 else None
    if mutant == "hash_probe_stops":
        src, tgt, _ = C.case_input(c)
        cap, home = own_home_slots(tgt, C.OWN_RES)
        found = len(np.unique(home))                            # at most one key per home slot sits in it, whatever the insertion order
        return f"n_hits <= {found} for {C.OWN_N} (capacity {cap})" if found < C.OWN_N else None
    if c.kind == "voxels":
        res, min_points, tight = c.params
        g, m = C.ref_voxels(c), NC.build(C.case_input(c)[0], res, min_points, np.float64, key_dtype=F, rules=rules)
        if not (np.array_equal(g[0], m[0]) and np.array_equal(g[1], m[1])):
            return f"keys or counts: {len(m[0])} voxels for {len(g[0])}, {int((m[1].sum()))} points for {int(g[1].sum())}" if len(m[0]) != len(g[0]) else \
                f"keys or counts of {int((g[0] != m[0]).any(axis=1).sum() + (g[1] != m[1]).sum())} voxels"
        ex = C.voxel_excess(m[2].astype(F), np.stack([m[3][:, i, j] for i, j in C.IU], axis=1).astype(F), g)
        return f"{max(ex):.1e} x the bound" if tight and max(ex) > 1 else None
    src, tgt, init = C.case_input(c)
    b = C.ref_runs(c)[1]
    m = NC.register(src, tgt, init, dtype=np.float64, key_dtype=F, rules=rules, **C.loop_of(c))
    if m["n_hits"] != b["n_hits"]:
        return f"n_hits {m['n_hits']} for {b['n_hits']}"
    if c.params["expect"] == "budget":
        fro, rel = NC.distances(m, b)
        bp, bs = C.budget(c)
        if not (fro <= bp and rel <= bs):                       # (NaN tells too)
            return f"pose {fro / bp:.1e} x, score {rel / bs:.1e} x the budget"
    return None


@pytest.mark.parametrize("mutant", sorted(TELLS))
def test_every_mutant_is_told_apart_by_a_case_the_gpu_file_runs(mutant):
    assert set(MUTANT_RULES) <= set(TELLS) and len(TELLS) == 11
    for cid in (TELLS[mutant],) + ALSO.get(mutant, ()):
        how = tells(mutant, cid)
        print(f"{mutant}: {cid}: {how}")
        assert how is not None, (mutant, cid)


def test_the_control_resolution_tells_no_key_arithmetic():
    """at the dyadic resolution every division rule gives the same keys: what tells them apart at the others is the arithmetic alone"""
    assert tells("keys_f64", "faces-res0.5") is None and tells("keys_reciprocal", "faces-res0.5") is None


# ---- raw entry points -------------------------------------------------------------------------------------------------------------------
def test_raw_entry_points_refuse_without_a_context_whatever_the_key_box():
    L = _lib.load()
    src, tgt = C.saturated("bits65")
    r = _lib.NdtResultC()
    r.iterations = 7
    for cfg in (_lib.NdtConfigC(1.0, 0.1, 35, 1e-4, 5), _lib.NdtConfigC(1.0, 0.1, 35, 1e-4, len(tgt) + 1), _lib.NdtConfigC(1.0, 0.1, 35, 1e-4, 0)):
        for fn in (L.tc_ndt_registration, L.tc_ndt_registration_device):
            assert fn(None, src.ctypes.data, len(src), tgt.ctypes.data, len(tgt), None, C_.byref(cfg), C_.byref(r)) == _lib.TC_INVALID_DATA
    assert r.iterations == 7
    nv = C_.c_size_t(7)
    for m in (0, 1, len(tgt) + 1):
        assert L.tc_ndt_voxels(None, tgt.ctypes.data, len(tgt), 1.0, m, None, None, None, None, 0, C_.byref(nv)) == _lib.TC_INVALID_DATA and nv.value == 7
    assert _lib.TC_UNSUPPORTED == 4


if __name__ == "__main__":                                      # the mutant table of STATE.md
    t0 = time.perf_counter()
    print("| mutant | told apart by | how |\n|---|---|---|")
    for mutant in TELLS:
        for cid in (TELLS[mutant],) + ALSO.get(mutant, ()):
            print(f"| {mutant} | `{cid}` | {tells(mutant, cid)} |")
    print(f"({time.perf_counter() - t0:.1f} s)")
