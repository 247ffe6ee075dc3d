"""The neighbour-search exports at their edges (tc_knn, tc_radius_search, tc_search_index_query, tc_search_index_radius_count /
_fill and their _device twins): every result goes through tests/search_checker.py, which accepts any valid choice among ties and
nothing else -- counts, distance bits, index sets.  No tolerance anywhere.  tests/test_search_cpu.py proves the same inputs on the
oracle alone (that the checker agrees with the reference, what each family is there for, that wrong answers fail).

Roads: the context's one-shot calls with numpy and with torch input, the persistent handle (tc.SearchIndex); where named, also the
handle built from and asked with device tensors, and the raw *_device exports on torch device memory."""
import ctypes as C

import numpy as np
import pytest
import torch

import threecrate_amd as tc
from tests import search_checker as S
from threecrate_amd import _lib

pytestmark = pytest.mark.gpu

KNN_CASES, MANY_CASES, RADIUS_ALL_CASES = S.knn_cases(), S.many_query_cases(), S.radius_all_cases()
DEVICE_ROAD_FAMILIES = ("lists", "duplicates", "placed", "clamped", "shell_radius", "no_radius", "small", "nq")
_handles = {}


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _handles.values():
        h.close()
    _handles.clear()


def handle(ctx, cloud, device=False):
    """one tc.SearchIndex per cloud (and per input kind) for the whole file"""
    key = (cloud, device)
    if key not in _handles:
        pts = getattr(S, cloud[0])(*cloud[1])[0]
        _handles[key] = tc.SearchIndex(ctx, torch.from_numpy(pts).cuda() if device else pts)
    return _handles[key]


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def raw_device(ctx, pts, qs, k, radius):
    """tc_knn_device / tc_radius_search_device on torch device memory"""
    p, q = torch.from_numpy(pts).cuda(), torch.from_numpy(qs).cuda()
    idx = torch.zeros((len(qs), max(k, 1)), dtype=torch.int32, device="cuda")
    dist = torch.zeros((len(qs), max(k, 1)), dtype=torch.float32, device="cuda")
    cnt = torch.full((len(qs),), -1, dtype=torch.int32, device="cuda")
    ctx._order(p.device)
    if radius is None:
        rc = ctx._L.tc_knn_device(ctx._h, p.data_ptr(), len(pts), q.data_ptr(), len(qs), k, idx.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    else:
        rc = ctx._L.tc_radius_search_device(ctx._h, p.data_ptr(), len(pts), q.data_ptr(), len(qs), radius, k, idx.data_ptr(), dist.data_ptr(), cnt.data_ptr())
    ctx._check(rc)
    return idx, dist, cnt


def roads(ctx, c, pts, qs, device_roads):
    """(name, thunk) of every road of a case"""
    k, r = c.k, c.radius
    tp, tq = torch.from_numpy(pts), torch.from_numpy(qs)
    if r is None:
        out = [("numpy", lambda: ctx.find_k_nearest_batch(pts, qs, k)), ("torch", lambda: ctx.find_k_nearest_batch(tp, tq, k)),
               ("handle", lambda: handle(ctx, c.cloud).find_k_nearest_batch(qs, k))]
        if device_roads:
            out.append(("handle_device", lambda: handle(ctx, c.cloud, True).find_k_nearest_batch(tq.cuda(), k)))
    else:
        out = [("numpy", lambda: ctx.find_radius_neighbors_batch(pts, qs, r, k)), ("torch", lambda: ctx.find_radius_neighbors_batch(tp, tq, r, k)),
               ("handle", lambda: handle(ctx, c.cloud).find_radius_neighbors_batch(qs, r, k))]
        if device_roads:
            out.append(("handle_device", lambda: handle(ctx, c.cloud, True).find_radius_neighbors_batch(tq.cuda(), r, k)))
    if device_roads:
        out.append(("raw_device", lambda: raw_device(ctx, pts, qs, k, r)))
    return out


def run_case(ctx, c, only=None):
    pts, qs, b = S.case_input(c)
    reports = {}
    for name, call in roads(ctx, c, pts, qs, c.family in DEVICE_ROAD_FAMILIES):
        if only is None or name == only:
            idx, dist, cnt = (_host(a) for a in call())
            try:
                reports[name] = (S.check_knn(pts, qs, c.k, idx, dist, cnt, c.radius, brute=b), dist, cnt)
            except AssertionError as e:
                raise AssertionError(f"road {name}: {e}") from None
    return reports


@pytest.mark.parametrize("c", KNN_CASES, ids=S.case_id)
def test_knn_and_radius_among_the_k_nearest(ctx, c):
    """lists: either side of every list size; lattice / lattice3 / duplicates: plateaus at the cut; small / degenerate: K1 = min(k,
    finite points), boxes without extent, ring growth over empty cells; placed: faces, corners, 1 / 10^3 / 10^6 diagonals outside,
    NaN and infinite queries among finite ones; nq: block boundaries of the 256-, 128- and 64-lane kernels; clamped: a grid
    narrower than the cloud; shifted: far from the origin; shell_radius: radii on, one ulp below and one ulp above a shell, k_max
    below, at and above the true count; no_radius: radius 0, negative and NaN give count 0."""
    reports = run_case(ctx, c)
    assert len(reports) >= 3
    if c.family == "no_radius":
        assert all((cnt == 0).all() for _, _, cnt in reports.values())


@pytest.mark.parametrize("kind", ["uniform", "lattice"])
@pytest.mark.parametrize("k", S.FAR_KS)
def test_translation_leaves_the_distances_alone(ctx, kind, k):
    """the same differences at every shift: the checker's d2 are the same bits, so are the distances that come back"""
    base = run_case(ctx, S.Case("shifted", ("shifted", (kind, 0.0)), k, None, None), only="numpy")["numpy"][1]
    for s in S.FAR_SHIFTS:
        for name, (_, dist, _) in run_case(ctx, S.Case("shifted", ("shifted", (kind, s)), k, None, None)).items():
            assert np.array_equal(dist.view(np.uint32), base.view(np.uint32)), (s, name)


@pytest.mark.parametrize("road", ["numpy", "torch", "handle"])
@pytest.mark.parametrize("c", MANY_CASES, ids=S.case_id)
def test_more_queries_than_blocks(ctx, c, road):
    """knn_coop_kernel runs min(nq, 65 536) blocks: queries 65 536 and above are a block's second trip, with another answer (and
    with a radius another count) than the first trip's"""
    rep = run_case(ctx, c, only=road)[road][0]
    assert rep.queries == c.nq


def test_k_beyond_the_limit_is_unsupported_on_every_road(ctx):
    c = S.Case("lists", ("uniform", ()), 2049, None, None)
    pts, qs, _ = S.case_input(c)
    for r in (None, 0.1):
        for name, call in roads(ctx, c._replace(radius=r), pts, qs[:5], True):
            with pytest.raises(tc.Unsupported):
                call()
    ok = run_case(ctx, c._replace(k=2048, nq=5))                    # and the context is usable afterwards
    assert len(ok) == 5


def test_handle_radius_forms(ctx):
    """radius < 0 at the handle's entry point means k-NN; its Python radius form gives no neighbours for 0, negative and NaN"""
    pts, qs, b = S.case_input(S.Case("lattice", ("lattice", (1,)), 10, None, 200))
    h = handle(ctx, ("lattice", (1,)))
    S.check_knn(pts, qs, 10, *h._query(qs, 10, -1.0), brute=b)
    S.check_knn(pts, qs, 10, *h._query(qs, 10, -0.25), brute=b)
    for r in (0.0, -1.0, float("nan")):
        assert (h.find_radius_neighbors_batch(qs, r, 10)[2] == 0).all()
        assert (ctx.find_radius_neighbors_batch(pts, qs, r, 10)[2] == 0).all()
        assert h.find_radius_neighbors(qs[0], r, 10) == [] and ctx.find_radius_neighbors(pts, qs[0], r, 10) == []


@pytest.mark.parametrize("name,cloud,radius,nq", RADIUS_ALL_CASES, ids=[r[0] for r in RADIUS_ALL_CASES])
def test_unbounded_radius_search(ctx, name, cloud, radius, nq):
    """find_radius_neighbors_all: radii on and next to a shell, nq around the 128-lane block, empty segments between filled ones,
    the whole cloud in every ball, a clamped grid"""
    pts, qs, b = S.case_input(S.Case(name, cloud, 0, radius, nq))
    for h in (handle(ctx, cloud), handle(ctx, cloud, True)):
        off, idx, dist = h.find_radius_neighbors_all(qs, radius)
        total = S.check_radius_all(pts, qs, radius, off, idx, dist, brute=b)
        assert total == len(idx)
        assert np.array_equal(h.radius_counts(qs, radius), np.diff(off))


def test_single_query_forms_stop_at_count(ctx):
    """entries beyond count are not part of the answer: 8 points asked for 20, a radius that holds 4"""
    cube = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float32)
    h = tc.SearchIndex(ctx, cube)
    q = np.zeros((1, 3), np.float32)
    for res, k, r in ((ctx.find_k_nearest(cube, q[0], 20), 20, None), (h.find_k_nearest(q[0], 20), 20, None),
                      (ctx.find_radius_neighbors(cube, q[0], 1.0, 20), 20, 1.0), (h.find_radius_neighbors(q[0], 1.0, 20), 20, 1.0)):
        assert len(res) == (8 if r is None else 4)
        idx, dist = np.zeros((1, k), np.int64), np.zeros((1, k), np.float32)
        idx[0, :len(res)], dist[0, :len(res)] = [i for i, _ in res], [d for _, d in res]
        S.check_knn(cube, q, k, idx, dist, [len(res)], r)
    h.close()


def test_the_intended_kernels_ran(ctx):
    """tc_profile_read: one knn_batch launch per k-NN / radius call of every family, one radius_count and one radius_fill for the
    unbounded form, and nothing else that searches"""
    firsts = {}
    for c in KNN_CASES + MANY_CASES[:1]:
        if c.family != "no_radius":
            firsts.setdefault((c.family, c.radius is None), c)
    ctx.profile_enable(True)
    try:
        for c in firsts.values():
            pts, qs, b = S.case_input(c)
            for name, call in roads(ctx, c, pts, qs, True):
                if name == "handle_device":
                    handle(ctx, c.cloud, True)                  # (built outside the measured call)
                if name == "handle":
                    handle(ctx, c.cloud)
                ctx.profile_reset()
                call()
                rows = ctx.profile_read()
                assert [rows.get(r, (0,))[0] for r in ("knn_batch", "radius_count", "radius_fill")] == [1, 0, 0], (S.case_id(c), name, rows)
        for name, cloud, radius, nq in RADIUS_ALL_CASES:
            if S.radius_sq(radius) is not None:
                pts, qs, b = S.case_input(S.Case(name, cloud, 0, radius, nq))
                h = handle(ctx, cloud)
                ctx.profile_reset()
                h.find_radius_neighbors_all(qs, radius)
                rows = ctx.profile_read()
                assert [rows.get(r, (0,))[0] for r in ("knn_batch", "radius_count", "radius_fill")] == [0, 1, 1], (name, rows)
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- entry-point rules at the raw ABI ---------------------------------------------------------------------------------------------
SENTINEL = 0xDEADBEEF


def _sentinels(nq, k, device):
    mk = (lambda n: torch.full((n,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")) if device else (lambda n: np.full(n, SENTINEL, np.uint32))
    return mk(max(nq * k, 1)), mk(max(nq * k, 1)), mk(max(nq, 1))


def _untouched(a):
    return bool((_host(a).view(np.uint32) == SENTINEL).all())


def _ptr(a):
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_raw_entry_points_with_nothing_to_do(ctx, device):
    """nq = 0: TC_OK, nothing written; k = 0 or n = 0: count zeroed, idx / dist untouched"""
    L, (pts, qs) = ctx._L, S.uniform()
    pts, qs = pts.copy(), qs[:16].copy()
    give = (lambda a: torch.from_numpy(a).cuda()) if device else (lambda a: a)
    p, q = give(pts), give(qs)
    knn = L.tc_knn_device if device else L.tc_knn
    rad = L.tc_radius_search_device if device else L.tc_radius_search
    ask = L.tc_search_index_query_device if device else L.tc_search_index_query
    h, empty = handle(ctx, ("uniform", ()), device), tc.SearchIndex(ctx, np.zeros((0, 3), np.float32))
    if device:
        ctx._order(p.device)
    calls = {
        "knn": lambda n, nq, k, o: knn(ctx._h, _ptr(p), n, _ptr(q), nq, k, *o),
        "radius": lambda n, nq, k, o: rad(ctx._h, _ptr(p), n, _ptr(q), nq, 0.1, k, *o),
        "handle": lambda n, nq, k, o: ask((h if n else empty)._h, _ptr(q), nq, k, -1.0, *o),
        "handle_radius": lambda n, nq, k, o: ask((h if n else empty)._h, _ptr(q), nq, k, 0.1, *o),
    }
    for name, call in calls.items():
        idx, dist, cnt = _sentinels(16, 4, device)
        assert call(len(pts), 0, 4, (_ptr(idx), _ptr(dist), _ptr(cnt))) == _lib.TC_OK, name
        assert _untouched(idx) and _untouched(dist) and _untouched(cnt), name
        for n, k in ((len(pts), 0), (0, 4), (0, 0)):
            idx, dist, cnt = _sentinels(16, 4, device)
            assert call(n, 16, k, (_ptr(idx), _ptr(dist), _ptr(cnt))) == _lib.TC_OK, (name, n, k)
            assert _untouched(idx) and _untouched(dist) and (_host(cnt) == 0).all(), (name, n, k)
    empty.close()


def test_raw_unbounded_radius_entry_points(ctx):
    L, (pts, qs) = ctx._L, S.uniform()
    qs = qs[:16].copy()
    h = handle(ctx, ("uniform", ()))
    cnt, idx, dist = np.full(16, SENTINEL, np.uint32), np.full(8, SENTINEL, np.uint32), np.full(8, SENTINEL, np.uint32)
    off = np.zeros(17, np.uint64)
    assert L.tc_search_index_radius_count(h._h, qs.ctypes.data, 0, 0.1, cnt.ctypes.data) == _lib.TC_OK and _untouched(cnt)
    assert L.tc_search_index_radius_fill(h._h, qs.ctypes.data, 0, 0.1, off.ctypes.data, 8, idx.ctypes.data, dist.ctypes.data) == _lib.TC_OK
    assert L.tc_search_index_radius_fill(h._h, qs.ctypes.data, 16, 0.1, off.ctypes.data, 0, idx.ctypes.data, dist.ctypes.data) == _lib.TC_OK
    assert L.tc_search_index_radius_fill(h._h, qs.ctypes.data, 16, 0.0, off.ctypes.data, 0, idx.ctypes.data, dist.ctypes.data) == _lib.TC_OK
    assert _untouched(idx) and _untouched(dist)
    for r in (0.0, -1.0, float("nan")):
        assert L.tc_search_index_radius_fill(h._h, qs.ctypes.data, 16, r, off.ctypes.data, 8, idx.ctypes.data, dist.ctypes.data) == _lib.TC_INVALID_DATA
        assert _untouched(idx) and _untouched(dist)
        cnt[:] = SENTINEL
        assert L.tc_search_index_radius_count(h._h, qs.ctypes.data, 16, r, cnt.ctypes.data) == _lib.TC_OK and (cnt == 0).all()
    off, idx, dist = h.find_radius_neighbors_all(qs, 0.1)          # and the handle still answers
    S.check_radius_all(pts, qs, 0.1, off, idx, dist)
