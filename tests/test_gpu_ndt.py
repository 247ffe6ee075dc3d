"""NDT registration on the device (csrc/ndt.hip, include/threecrate_hip_ndt.h) against the f64 checker (tests/ndt_checker.py).

Budgets: a device pose may be at most 4 x the largest f32-to-f64 distance of the reference (the checker's two dtypes) over the inputs
of that test away from the f64 checker (Frobenius of the 4 x 4), the score the same relatively; the voxel map's keys and counts are
exact, mean and inv_cov within 4 x the reference's own f32-to-f64 distance on that cloud, relative to |inv_cov|.  The factor covers expf
implementations and the order of f32 products.  The inputs' preconditions (no coordinate near a voxel face, the same keys and the same
loop control in f32 and f64) are asserted in tests/test_ndt_cpu.py and again here where a test makes its own input."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import _lib
from tests import ndt_checker as NC

pytestmark = pytest.mark.gpu
F = np.float32
LONG_RUN = 128          # kNdtLongRun of csrc/ndt.hip: runs of more points get a block each
CHUNK = 64              # kNdtChunk: iterations between two reads of the state


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def reference(nt, ns, res, **kw):
    """the input and the checker's two runs of it, made once"""
    loop = dict(kw)
    src, tgt, init = NC.surface_pair(nt, ns, res, **kw)
    loop.setdefault("max_iterations", 1)
    a = NC.register(src, tgt, init, resolution=res, dtype=np.float32, **loop)
    b = NC.register(src, tgt, init, resolution=res, dtype=np.float64, **loop)
    assert (a["iterations"], a["converged"]) == (b["iterations"], b["converged"])
    assert min(r["face"] for r in b["evals"]) >= NC.FACE_MARGIN
    assert all(np.array_equal(x["keys"], y["keys"]) for x, y in zip(a["evals"], b["evals"]))
    return src, tgt, init, a, b


def check_against(r, b, budget_pose, budget_score, what):
    fro, rel = NC.distances((r.transformation, r.score), b)
    print(f"{what}: pose {fro:.2e} (budget {budget_pose:.2e}), score {rel:.2e} (budget {budget_score:.2e}), hits {r.n_hits}")
    assert (r.iterations, r.converged, r.n_voxels, r.n_hits) == (b["iterations"], b["converged"], b["n_voxels"], b["n_hits"]), what
    assert fro <= budget_pose and rel <= budget_score, what


# ---- the voxel map ----
def voxel_budget(cloud, res, min_points):
    g32, g64 = NC.build(cloud, res, min_points, np.float32), NC.build(cloud, res, min_points, np.float64)
    assert np.array_equal(g32[0], g64[0])
    scale = np.linalg.norm(g64[3], axis=(1, 2))
    d_inv = (np.linalg.norm(g32[3].astype(np.float64) - g64[3], axis=(1, 2)) / scale).max()
    d_mean = np.abs(g32[2].astype(np.float64) - g64[2]).max()
    return g64, 4 * max(d_inv, np.finfo(F).eps), 4 * max(d_mean, np.finfo(F).eps * np.abs(g64[2]).max())


def check_voxels(ctx, cloud, res, min_points, what=""):
    keys, counts, mean, inv = ctx.ndt_voxels(cloud, res, min_points)
    g64, b_inv, b_mean = voxel_budget(cloud, res, min_points)
    assert keys.dtype == np.int32 and np.array_equal(keys, g64[0]) and np.array_equal(counts, g64[1]), what
    if len(keys):
        scale = np.linalg.norm(g64[3], axis=(1, 2))
        full = np.zeros((len(keys), 3, 3))
        iu = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        for c, (i, j) in enumerate(iu):
            full[:, i, j] = full[:, j, i] = inv[:, c]
        d_inv = (np.linalg.norm(full - g64[3], axis=(1, 2)) / scale).max()
        d_mean = np.abs(mean.astype(np.float64) - g64[2]).max()
        print(f"voxels {what}: V = {len(keys)}, inv_cov {d_inv:.2e} (budget {b_inv:.2e}), mean {d_mean:.2e} (budget {b_mean:.2e})")
        assert d_inv <= b_inv and d_mean <= b_mean, what
    return keys, counts, mean, inv


def lattice_cloud(v, per_voxel=6, seed=0):
    """v voxels of resolution 1 along a 16-wide lattice that straddles the origin on all axes, per_voxel points each"""
    rng = np.random.default_rng(seed)
    cells = np.array([[i % 16 - 8, (i // 16) % 16 - 8, i // 256 - 1] for i in range(v)], np.float64)
    pts = cells[:, None, :] + rng.uniform(0.05, 0.95, (v, per_voxel, 3))
    return rng.permutation(pts.reshape(-1, 3)).astype(F)


@pytest.mark.parametrize("v", [1, 255, 256, 257])
def test_voxel_counts_around_a_block(ctx, v):
    keys, counts, _, _ = check_voxels(ctx, lattice_cloud(v), 1.0, 5, f"V = {v}")
    assert len(keys) == v and (counts == 6).all() and keys.min() < 0 < keys.max() + 2


def test_voxel_of_min_points_and_one_less_side_by_side(ctx):
    rng = np.random.default_rng(1)
    cloud = np.r_[rng.uniform(0.1, 0.9, (4, 3)), rng.uniform(0.1, 0.9, (5, 3)) + [1, 0, 0]].astype(F)
    keys, counts, _, _ = check_voxels(ctx, cloud, 1.0, 5)
    assert keys.tolist() == [[1, 0, 0]] and counts.tolist() == [5]
    keys, _, _, _ = check_voxels(ctx, cloud, 1.0, 4)
    assert keys.tolist() == [[0, 0, 0], [1, 0, 0]]


def test_runs_around_the_long_run_threshold(ctx):
    rng = np.random.default_rng(2)
    sizes = [LONG_RUN - 1, LONG_RUN, LONG_RUN + 1, 3 * LONG_RUN + 17, 7]
    cloud = np.concatenate([rng.uniform(0.02, 0.98, (m, 3)) * [1, 1, 0.3] + [2 * i - 3, -1, 0] for i, m in enumerate(sizes)])
    cloud = rng.permutation(cloud).astype(F)
    _, counts, _, _ = check_voxels(ctx, cloud, 1.0, 5, "long runs")
    assert sorted(counts.tolist()) == sorted(sizes)


def test_cloud_straddling_the_origin(ctx):
    rng = np.random.default_rng(3)
    cloud = rng.uniform(-1.0, 1.0, (4000, 3)).astype(F)
    cloud[:3] = [[-0.1, -0.5, -1e-7], [0.0, 0.0, 0.0], [-0.5, 0.5, -1.0]]
    keys, _, _, _ = check_voxels(ctx, cloud, 0.5, 5, "origin")
    assert keys.min() == -2 and keys.max() == 1 and len(keys) == 64


def test_non_finite_target_points_are_left_out(ctx):
    clean = lattice_cloud(40, seed=4)
    dirty = np.insert(clean, [0, 17, 17, 100, len(clean)], [[np.nan, 0, 0], [0, np.inf, 0], [0.5, 0.5, -np.inf], [np.nan] * 3, [1, np.nan, 1]], axis=0).astype(F)
    a, b = ctx.ndt_voxels(clean, 1.0, 5), check_voxels(ctx, dirty, 1.0, 5, "non-finite")
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    keys, _, _, _ = ctx.ndt_voxels(np.full((9, 3), np.nan, F), 1.0, 5)
    assert keys.shape == (0, 3)


def test_voxels_capacity_and_null_outputs(ctx):
    cloud = lattice_cloud(20, seed=5)
    L, nv = ctx._L, C.c_size_t(0)
    keys = np.full((20, 3), 77, np.int32)
    assert L.tc_ndt_voxels(ctx._h, cloud.ctypes.data, len(cloud), 1.0, 5, keys.ctypes.data, None, None, None, 19, C.byref(nv)) == _lib.TC_INVALID_DATA
    assert nv.value == 20 and (keys == 77).all()
    assert L.tc_ndt_voxels(ctx._h, cloud.ctypes.data, len(cloud), 1.0, 5, None, None, None, None, 0, C.byref(nv)) == _lib.TC_INVALID_DATA and nv.value == 20
    assert L.tc_ndt_voxels(ctx._h, cloud.ctypes.data, len(cloud), 1.0, 5, keys.ctypes.data, None, None, None, 20, C.byref(nv)) == _lib.TC_OK
    assert np.array_equal(keys, ctx.ndt_voxels(cloud, 1.0, 5)[0])
    dev = [torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x for x in ctx.ndt_voxels(torch.from_numpy(cloud).cuda(), 1.0, 5)]
    for x, y in zip(dev, ctx.ndt_voxels(cloud, 1.0, 5)):
        assert x.is_cuda and np.array_equal(x.cpu().numpy().view(np.uint32).reshape(-1), y.view(np.uint32).reshape(-1))


# ---- one step ----
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096, 4097]


def one_step_budget(ns):
    """4 x the family's largest f32-to-f64 distance.  One source point is a family of its own: its H has rank 3, the solve rests on the 1e-6 I
    alone, and the reference's two dtypes are 1e-2 apart there -- as a member it would widen every other size's budget by four decades."""
    d = [NC.distances(reference(4096, n, 0.5)[3], reference(4096, n, 0.5)[4]) for n in ([1] if ns == 1 else SIZES[1:])]
    return 4 * max(x[0] for x in d), 4 * max(x[1] for x in d)


@pytest.mark.parametrize("ns", SIZES)
def test_one_step_source_sizes(ctx, ns):
    src, tgt, init, _, b = reference(4096, ns, 0.5)
    bp, bs = one_step_budget(ns)
    check_against(ctx.ndt_registration(src, tgt, init, resolution=0.5, max_iterations=1), b, bp, bs, f"ns = {ns}")


def test_one_step_large(ctx):
    src, tgt, init, a, b = reference(20000, 20000, 0.25)
    fro, rel = NC.distances(a, b)
    check_against(ctx.ndt_registration(src, tgt, init, resolution=0.25, max_iterations=1), b, 4 * fro, 4 * rel, "20 000 points")


def test_source_outside_the_key_box(ctx):
    src, tgt, init, _, _ = reference(4096, 256, 0.5)
    far = (src + np.array([50.0, 0.0, 0.0], F)).astype(F)
    r = ctx.ndt_registration(far, tgt, init, resolution=0.5, max_iterations=5)
    assert (r.score, r.iterations, r.converged, r.n_hits) == (0.0, 1, True, 0)     # g = 0: the step is 0 < epsilon
    assert np.array_equal(bits(r.transformation), bits(init))


def test_source_half_inside_the_key_box(ctx):
    src, tgt, init, _, _ = reference(4096, 256, 0.5)
    half = src.copy()
    half[::2] += np.array([0.0, 50.0, 0.0], F)
    b = NC.register(half, tgt, init, resolution=0.5, max_iterations=1, dtype=np.float64)
    a = NC.register(half, tgt, init, resolution=0.5, max_iterations=1, dtype=np.float32)
    assert np.array_equal(a["evals"][0]["keys"], b["evals"][0]["keys"]) and b["evals"][0]["face"] >= NC.FACE_MARGIN and 0 < b["n_hits"] <= 128
    fro, rel = NC.distances(a, b)
    check_against(ctx.ndt_registration(half, tgt, init, resolution=0.5, max_iterations=1), b, 4 * fro, 4 * rel, "half inside")


def test_dense_and_hash_tables_give_the_same_bits(ctx):
    """Two copies of the pair ~1 000 apart in x and y at resolution 0.25: the key box has more than 2^24 cells, V stays small -> the hash table.
    The far copy of the target adds voxels no source point reaches, so the sums are those of the near pair alone, which fits the dense table."""
    off = (1024.0, 1024.0, 0.0)
    src, tgt, init, _, b = reference(20000, 2048, 0.25)
    far = (tgt.astype(np.float64) + off).astype(F)
    both = np.r_[tgt, far]                                      # the near points first: their voxels keep their points' order
    dense = ctx.ndt_registration(src, tgt, init, resolution=0.25, max_iterations=3)
    hashed = ctx.ndt_registration(src, both, init, resolution=0.25, max_iterations=3)
    kb = NC.keys_of(both, 0.25, np.float32)
    assert np.prod((kb.max(axis=0) - kb.min(axis=0) + 1).astype(np.float64)) > 2 ** 24 and hashed.n_voxels > dense.n_voxels
    assert np.array_equal(bits(dense.transformation), bits(hashed.transformation)) and bits(dense.score) == bits(hashed.score)
    assert (dense.iterations, dense.n_hits) == (hashed.iterations, hashed.n_hits) == (3, hashed.n_hits) and dense.n_hits > 1500
    # and the far copy is found through the table too
    src_far = (src.astype(np.float64) + off).astype(F)
    r = ctx.ndt_registration(src_far, both, None, resolution=0.25, max_iterations=1)
    assert r.n_hits > 1000


# ---- loop control ----
@pytest.mark.parametrize("iters", [0, 1, 2, CHUNK, CHUNK + 1])
def test_epsilon_zero_never_converges(ctx, iters):
    src, tgt, init, _, _ = reference(4096, 256, 0.5)
    r = ctx.ndt_registration(src, tgt, init, resolution=0.5, max_iterations=iters, epsilon=0.0)
    assert r.iterations == iters and not r.converged
    if iters == 0:
        assert r.score == 0.0 and r.n_hits == 0 and np.array_equal(bits(r.transformation), bits(init))
    else:
        assert r.score > 0.0 and not np.array_equal(bits(r.transformation), bits(init))


def test_the_clamp_binds(ctx):
    kw = dict(step_size=0.002, max_iterations=3, epsilon=0.0)
    src, tgt, init, a, b = reference(4096, 2048, 0.5, **kw)
    for d in b["deltas"]:
        assert abs(np.linalg.norm(d) - 0.002) < 1e-9                 # every step was clamped
    fro, rel = NC.distances(a, b)
    r = ctx.ndt_registration(src, tgt, init, resolution=0.5, **kw)
    check_against(r, b, 4 * fro, 4 * rel, "clamped steps")


def test_large_epsilon_converges_at_once(ctx):
    src, tgt, init, _, b = reference(4096, 2048, 0.5)
    r = ctx.ndt_registration(src, tgt, init, resolution=0.5, epsilon=10.0)
    assert (r.iterations, r.converged) == (1, True) and np.array_equal(bits(r.transformation), bits(init))
    assert abs(r.score - float(b["score"])) <= 1e-4 * float(b["score"]) and r.n_hits == b["n_hits"]


def test_default_config_to_convergence(ctx):
    src, tgt, init, a, b = reference(4096, 2048, 0.5, max_iterations=35)
    assert b["converged"] and 2 < b["iterations"] < 35
    fro, rel = NC.distances(a, b)
    check_against(ctx.ndt_registration(src, tgt, init, resolution=0.5), b, 4 * fro, 4 * rel, "default configuration")


# ---- roads ----
def test_numpy_torch_and_repeated_calls_give_the_same_bits(ctx):
    src, tgt, init, _, _ = reference(4096, 2048, 0.5)
    runs = [ctx.ndt_registration(src, tgt, init, resolution=0.5, max_iterations=4) for _ in range(2)]
    runs.append(ctx.ndt_registration(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), init, resolution=0.5, max_iterations=4))
    for r in runs[1:]:
        assert np.array_equal(bits(r.transformation), bits(runs[0].transformation)) and bits(r.score) == bits(runs[0].score)
        assert (r.iterations, r.converged, r.n_voxels, r.n_hits) == (runs[0].iterations, runs[0].converged, runs[0].n_voxels, runs[0].n_hits)
    with pytest.raises(Exception):
        ctx.ndt_registration(torch.from_numpy(src).cuda(), tgt, init, resolution=0.5)     # the first array chose the device road


def test_raw_entry_points_and_module_functions(ctx):
    import threecrate_amd.compat as threecrate
    src, tgt, init, _, b = reference(4096, 2048, 0.5)
    L = ctx._L
    cfg, res = _lib.NdtConfigC(0.5, 0.1, 1, 1e-4, 5), _lib.NdtResultC()
    assert L.tc_ndt_registration(ctx._h, src.ctypes.data, len(src), tgt.ctypes.data, len(tgt), init.ctypes.data, C.byref(cfg), C.byref(res)) == _lib.TC_OK
    host = (bytes(bits(np.array(res.transformation[:], F))), res.score, res.iterations, res.n_hits)
    ds, dt = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    torch.cuda.synchronize()
    res2 = _lib.NdtResultC()
    assert L.tc_ndt_registration_device(ctx._h, ds.data_ptr(), len(src), dt.data_ptr(), len(tgt), init.ctypes.data, C.byref(cfg), C.byref(res2)) == _lib.TC_OK
    assert host == (bytes(bits(np.array(res2.transformation[:], F))), res2.score, res2.iterations, res2.n_hits) and res.n_hits == b["n_hits"]
    # init NULL is the identity
    ident = ctx.ndt_registration(src, tgt, None, resolution=0.5, max_iterations=2)
    assert L.tc_ndt_registration(ctx._h, src.ctypes.data, len(src), tgt.ctypes.data, len(tgt), None, C.byref(_lib.NdtConfigC(0.5, 0.1, 2, 1e-4, 5)), C.byref(res)) == _lib.TC_OK
    assert np.array_equal(bits(np.array(res.transformation[:], F)), bits(ident.transformation))
    m = tc.ndt_registration(src, tgt, init, tc.NdtConfig(resolution=0.5, max_iterations=1), ctx=ctx)
    assert np.array_equal(bits(m.transformation), bits(np.array(res2.transformation[:], F)))
    d = tc.ndt_registration_default(src, tgt, init, ctx=ctx)
    assert d.iterations >= 1 and d.n_voxels < b["n_voxels"]                          # resolution 1.0
    c = threecrate.ndt_registration(threecrate.PointCloud(src), threecrate.PointCloud(tgt), init_transform=NC.matrix4(init), resolution=0.5, max_iterations=1)
    assert repr(c).startswith("NdtResult(converged=false, score=") and c.transformation().shape == (4, 4) and c.iterations == 1
    assert np.abs(c.transformation() - NC.matrix4(m.transformation)).max() < 1e-5


def test_errors_in_the_reference_order_through_every_road(ctx):
    import threecrate_amd.compat as threecrate
    src, tgt, init, _, _ = reference(4096, 256, 0.5)
    empty, two = np.zeros((0, 3), F), tgt[:2].copy()
    for road in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        s, t, e, t2 = road(src), road(tgt), road(empty), road(two)
        with pytest.raises(tc.AlgorithmError, match="Source point cloud is empty"):
            ctx.ndt_registration(e, t2, init)                                       # the first error wins over the second
        with pytest.raises(tc.AlgorithmError, match="Target point cloud has too few points for NDT voxel grid"):
            ctx.ndt_registration(s, t2, init)
        with pytest.raises(tc.AlgorithmError, match="NDT voxel grid is empty — try a larger resolution or lower min_points_per_voxel"):
            ctx.ndt_registration(s, t, init, resolution=0.5, min_points_per_voxel=2000)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(tc.InvalidData, match="Resolution must be positive and finite"):
                ctx.ndt_registration(e, t2, init, resolution=bad)                   # checked before the reference's errors
            with pytest.raises(tc.InvalidData, match="Resolution must be positive and finite"):
                ctx.ndt_voxels(t, bad)
    with pytest.raises(RuntimeError, match="Source point cloud is empty"):
        threecrate.ndt_registration(threecrate.PointCloud(), threecrate.PointCloud(tgt))


def test_a_failed_call_writes_iterations_only(ctx):
    src, tgt, init, _, _ = reference(4096, 256, 0.5)
    L = ctx._L
    cfg = _lib.NdtConfigC(0.5, 0.1, 5, 1e-4, 5000)
    for fn, s, t in ((L.tc_ndt_registration, src.ctypes.data, tgt.ctypes.data),):
        res = _lib.NdtResultC()
        res.score, res.iterations, res.converged, res.n_voxels, res.n_hits = 7.0, 7, 7, 7, 7
        for c in range(7):
            res.transformation[c] = 7.0
        assert fn(ctx._h, s, len(src), t, len(tgt), init.ctypes.data, C.byref(cfg), C.byref(res)) == _lib.TC_ALGORITHM
        assert res.iterations == 0 and (res.score, res.converged, res.n_voxels, res.n_hits) == (7.0, 7, 7, 7) and list(res.transformation) == [7.0] * 7
        assert fn(ctx._h, s, len(src), t, len(tgt), init.ctypes.data, None, C.byref(res)) == _lib.TC_INVALID_DATA
        assert fn(ctx._h, None, len(src), t, len(tgt), init.ctypes.data, C.byref(cfg), C.byref(res)) == _lib.TC_INVALID_DATA
        assert fn(ctx._h, s, len(src), t, len(tgt), init.ctypes.data, C.byref(cfg), None) == _lib.TC_INVALID_DATA


def test_ndt_after_the_other_users_of_the_pinned_block(ctx):
    """NDT's read-back records have a region of their own in the pinned block; run after the calls that use the shared one, on the same
    context, it gives the bits a fresh context gives."""
    src, tgt, init, _, _ = reference(4096, 2048, 0.5)
    fresh = tc.GpuContext(0)
    want = fresh.ndt_registration(src, tgt, init, resolution=0.5, max_iterations=3)
    fresh.close()
    ctx.voxel_grid_filter(tgt, 0.3)
    ctx.segment_plane(tgt, 0.05, 64)
    ctx.radius_outlier_removal(tgt, 0.3, 3)
    ctx.icp_point_to_point(src, tgt, init, 5)
    got = ctx.ndt_registration(src, tgt, init, resolution=0.5, max_iterations=3)
    assert np.array_equal(bits(got.transformation), bits(want.transformation)) and bits(got.score) == bits(want.score) and got.n_hits == want.n_hits
    down = ctx.voxel_grid_filter(tgt, 0.3)
    assert len(down) > 0
