"""The numpy road and the torch road of every method that has both, on one 2 048-point pair: bit for bit.

numpy input takes the host entry point (the library stages the arrays itself), a torch device tensor the *_device twin; the
binding picks between them in one place per method, and both must hand the same values to the same kernels.  k = 8 and
5 iterations: enough for pairs, a refine list and more than one cluster.  Every comparison here is exact: on the commit
before the binding was rewritten around the array adapters (dbb2449) the two roads were bit-identical for every entry point
below, in every `correspondences` mode, so none of them needs the tolerance of its parity test in test_gpu_parity.py.
"""
import numpy as np
import pytest
import torch

import threecrate_amd as tc
from threecrate_amd import synth

pytestmark = pytest.mark.gpu

N, K, ITERS, MAX_DIST = 2048, 8, 5, 0.2
MODES = [True, False, "device"]


@pytest.fixture(scope="module")
def pair():
    src, tgt, _ = synth.registration_pair(N, seed=7, transform=synth.small_transform(N))
    return {"src": src, "tgt": tgt, "dsrc": torch.from_numpy(src).cuda(), "dtgt": torch.from_numpy(tgt).cuda()}


@pytest.fixture(scope="module")
def normals(ctx, pair):
    return ctx.estimate_normals(pair["tgt"], K)


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def same_result(a, b, mode, n_corr=N, device_bits=True):
    """a: the numpy road's ICPResult, b: the torch road's; device_bits: correspondences="device" keeps the int32 the kernel wrote"""
    assert np.array_equal(a.transformation, b.transformation), (a.transformation, b.transformation)
    assert (a.mse, a.iterations, a.converged) == (b.mse, b.iterations, b.converged)
    assert np.array_equal(a.correspondences, b.correspondences)
    if not mode:
        assert a.corr_target is None and b.corr_target is None
        return
    ca, cb = host(a.corr_target), host(b.corr_target)
    assert ca.dtype == np.uint32 and cb.dtype == (np.int32 if mode == "device" and device_bits else np.int64)
    assert len(ca) == len(cb) == n_corr
    assert np.array_equal(ca, cb.astype(np.uint32))              # int32 bits (-1 = none) and masked int64 read the same as u32
    assert (ca != 0xFFFFFFFF).sum() > n_corr // 2                # there are pairs to compare
    if mode is True:
        assert len(a.correspondences) == (ca != 0xFFFFFFFF).sum()


def test_normals(ctx, pair):
    a, b = ctx.estimate_normals(pair["tgt"], K), ctx.estimate_normals(pair["dtgt"], K)
    assert a.shape == (N, 6) and np.array_equal(a, host(b))
    cfg = tc.NormalEstimationConfig(k_neighbors=K, radius=0.12, consistent_orientation=False)
    assert np.array_equal(ctx.estimate_normals_with_config(pair["tgt"], cfg), host(ctx.estimate_normals_with_config(pair["dtgt"], cfg)))


def test_voxel_grid_filter(ctx, pair):
    a, b = ctx.voxel_grid_filter(pair["tgt"], 0.1), ctx.voxel_grid_filter(pair["dtgt"], 0.1)
    assert 1 < len(a) < N and np.array_equal(a, host(b))


def test_clusters(ctx, pair):
    la, ma, oa = ctx.extract_euclidean_clusters_labels(pair["tgt"], 0.06, 2, N)
    lb, mb, ob = ctx.extract_euclidean_clusters_labels(pair["dtgt"], 0.06, 2, N)
    assert len(oa) > 2                                                                # more than one cluster
    assert (la.dtype, ma.dtype, oa.dtype) == (np.uint32, np.uint32, np.uint64)
    assert (lb.dtype, mb.dtype, ob.dtype) == (torch.int32, torch.int32, torch.int64)
    assert np.array_equal(la, host(lb).astype(np.uint32)) and np.array_equal(ma, host(mb).astype(np.uint32))
    assert np.array_equal(oa, host(ob).astype(np.uint64))
    ca, cb = ctx.extract_euclidean_clusters(pair["tgt"], 0.06, 2, N), ctx.extract_euclidean_clusters(pair["dtgt"], 0.06, 2, N)
    assert len(ca) == len(cb) == len(oa) - 1
    for x, y in zip(ca, cb):
        assert x.dtype == np.int64 and y.dtype == torch.int64 and np.array_equal(x, host(y))


def test_fpfh(ctx, pair, normals):
    a, b = ctx.extract_fpfh_features(pair["tgt"], 0.15, K), ctx.extract_fpfh_features(pair["dtgt"], 0.15, K)
    assert a.shape == (N, 33) and a.any() and np.array_equal(a, host(b))
    a = ctx.extract_fpfh_features_with_normals(normals, 0.15, K)
    b = ctx.extract_fpfh_features_with_normals(torch.from_numpy(normals).cuda(), 0.15, K)
    assert a.shape == (N, 33) and a.any() and np.array_equal(a, host(b))


@pytest.mark.parametrize("mode", MODES)
def test_icp_detailed(ctx, pair, mode):
    a = ctx.icp_detailed(pair["src"], pair["tgt"], None, ITERS, MAX_DIST, 0.0, mode)
    b = ctx.icp_detailed(pair["dsrc"], pair["dtgt"], None, ITERS, MAX_DIST, 0.0, mode)
    assert a.iterations == ITERS
    same_result(a, b, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cols", [3, 6])
def test_icp_point_to_plane_detailed(ctx, pair, normals, mode, cols):
    nrm = normals if cols == 6 else np.ascontiguousarray(normals[:, 3:])
    init = synth.yaw_isometry((0.01, 0.0, -0.01), 0.01)
    a = ctx.icp_point_to_plane_detailed(pair["src"], pair["tgt"], nrm, init, ITERS, MAX_DIST, 0.0, mode)
    b = ctx.icp_point_to_plane_detailed(pair["dsrc"], pair["dtgt"], torch.from_numpy(nrm).cuda(), init, ITERS, MAX_DIST, 0.0, mode)
    assert a.iterations == ITERS
    same_result(a, b, mode)


@pytest.mark.parametrize("mode", MODES)
def test_gicp(ctx, pair, mode):
    cfg = tc.GicpConfig(max_iterations=ITERS, max_correspondence_distance=MAX_DIST, convergence_threshold=0.0, k_correspondences=K)
    a, b = ctx.gicp(pair["src"], pair["tgt"], None, cfg, mode), ctx.gicp(pair["dsrc"], pair["dtgt"], None, cfg, mode)
    assert a.iterations >= 1
    same_result(a, b, mode)


@pytest.mark.parametrize("mode", MODES)
def test_kiss_icp(ctx, pair, mode):
    cfg = tc.KissIcpConfig(voxel_size=0.08, max_range=100.0, min_range=0.1, max_iterations=ITERS)
    a, b = ctx.kiss_icp(pair["src"], pair["tgt"], None, cfg, mode), ctx.kiss_icp(pair["dsrc"], pair["dtgt"], None, cfg, mode)
    assert a.iterations >= 1
    n_down = 0 if not mode else len(a.corr_target)
    assert not mode or 1 < n_down < N                       # the pairs index the voxel-downsampled source
    same_result(a, b, mode, n_down, device_bits=False)          # this road has always masked


def test_search_index_queries(ctx, pair):
    ia, ib = tc.SearchIndex(ctx, pair["tgt"], K), tc.SearchIndex(ctx, pair["dtgt"], K)
    try:
        assert len(ia) == len(ib) == N
        for qa, qb in ((ia, ib), (ib, ia)):                 # either index, queried over either road
            idx, dist, cnt = qa.find_k_nearest_batch(pair["src"], K)
            didx, ddist, dcnt = qb.find_k_nearest_batch(pair["dsrc"], K)
            assert idx.dtype == np.int64 and didx.dtype == torch.int32 and (cnt == K).all()
            assert np.array_equal(idx, host(didx)) and np.array_equal(dist, host(ddist)) and np.array_equal(cnt, host(dcnt).astype(np.uint32))
            idx, dist, cnt = qa.find_radius_neighbors_batch(pair["src"], 0.1, K)
            didx, ddist, dcnt = qb.find_radius_neighbors_batch(pair["dsrc"], 0.1, K)
            assert np.array_equal(cnt, host(dcnt).astype(np.uint32)) and 0 < cnt.min() + cnt.max() and cnt.max() <= K
            live = np.arange(K)[None, :] < cnt[:, None]         # entries past count[q] are undefined
            assert live.sum() > N and np.array_equal(idx[live], host(didx)[live]) and np.array_equal(dist[live], host(ddist)[live])
    finally:
        ia.close(), ib.close()
