"""SHOT and USC descriptors on the device (include/threecrate_hip_shot.h, csrc/shot.hip) against the numpy restatement of the rule
(tests/shot_checker.py), for every case of tests/shot_cases.py.  The tolerances are derived, not measured: on a CLEAN row (margin >= 1e-6;
f64 sums in another order move nothing by more than ~1e-9, three orders inside) the integer counts agree, so a descriptor entry is two
roundings of one real number in [0, 1] (|device - checker| <= 2^-23) and a frame component is the f32 rounding of a unit vector plus that
1e-9 (<= 1e-6).  Flags agree exactly on every row.  A row that is not clean is still finite, >= 0, of unit L2 norm or all zero, bit-equal
between two calls and between the host and the _device road.  tests/test_shot_cpu.py proves that at least 98 % of every case's rows are clean."""
import numpy as np
import pytest

from threecrate_amd import _lib
from tests import shot_cases as CASES
from tests import shot_checker as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import threecrate_amd as tc
    c = tc.GpuContext(0)
    yield c
    c.close()


def _run(ctx, road, np6, radius, k, variant):
    import torch
    x = np6 if road == "host" else torch.from_numpy(np.array(np6)).to("cuda:0")
    d, f, fl = ctx.extract_shot_features(x, radius, k, variant, return_frames=True)
    if road == "device":
        assert isinstance(d, torch.Tensor) and d.is_cuda and f.is_cuda and fl.is_cuda
        d, f, fl = d.cpu().numpy(), f.cpu().numpy(), fl.cpu().numpy().view(np.uint32)
    assert d.dtype == np.float32 and d.shape == (len(np6), SC.dim(variant)) and f.shape == (len(np6), 9) and fl.shape == (len(np6),)
    return d, f, fl


@pytest.mark.parametrize("variant", CASES.VARIANTS)
@pytest.mark.parametrize("name", list(CASES.CASES))
def test_rows_frames_and_flags_equal_the_checker(ctx, name, variant):
    c, want = CASES.case(name), CASES.expected(name, variant)
    d, f, fl = _run(ctx, "host", c["np6"], c["radius"], c["k"], variant)
    rows = want["rows"]
    assert not SC.invariants(d)
    bad = SC.compare(d[rows], f[rows], fl[rows], want)
    assert not bad, bad
    if name == "degenerate_identical":
        assert not d.any()                                      # all-zero rows, exactly


@pytest.mark.parametrize("variant", CASES.VARIANTS)
@pytest.mark.parametrize("name", CASES.BOTH_ROADS)
def test_the_device_road_gives_the_host_roads_bits_and_two_calls_the_same(ctx, name, variant):
    c, want = CASES.case(name), CASES.expected(name, variant)
    host = _run(ctx, "host", c["np6"], c["radius"], c["k"], variant)
    dev = _run(ctx, "device", c["np6"], c["radius"], c["k"], variant)
    again = _run(ctx, "device", c["np6"], c["radius"], c["k"], variant)
    for a, b, e in zip(host, dev, again):
        assert a.tobytes() == b.tobytes() == e.tobytes()
    rows = want["rows"]
    assert not SC.compare(dev[0][rows], dev[1][rows], dev[2][rows], want)


@pytest.mark.parametrize("variant", CASES.VARIANTS)
def test_a_shift_by_a_power_of_two_changes_no_bit(ctx, variant):
    """the snapped cloud moved by 2^10 and 2^13: dv is exact, so descriptors, frames and flags are those of the unmoved cloud"""
    base = _run(ctx, "host", CASES.snapped(), CASES.EDGE_R, 10, variant)
    assert (base[2] & _lib.TC_SHOT_ROAD_MASK == _lib.TC_SHOT_ROAD_BALL).all()
    for shift in CASES.SHIFTS:
        moved = _run(ctx, "host", CASES.shifted(shift), CASES.EDGE_R, 10, variant)
        for a, b, what in zip(base, moved, ("desc", "lrf", "flags")):
            assert a.tobytes() == b.tobytes(), (shift, what, np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))[:10])


def test_the_outputs_that_may_be_absent_and_the_pair_input(ctx):
    import torch
    c = CASES.case("blocks_257")
    d, f, fl = _run(ctx, "host", c["np6"], c["radius"], c["k"], "shot")
    only = ctx.extract_shot_features(c["np6"], c["radius"], c["k"])
    assert isinstance(only, np.ndarray) and only.tobytes() == d.tobytes()
    pair = ctx.extract_shot_features((c["np6"][:, :3], c["np6"][:, 3:]), c["radius"], c["k"], "shot")
    assert pair.tobytes() == d.tobytes()
    t = torch.from_numpy(np.array(c["np6"])).to("cuda:0")
    pair = ctx.extract_shot_features((t[:, :3], t[:, 3:]), c["radius"], c["k"], "usc")
    assert pair.is_cuda and pair.shape == (257, 128)
    for empty in (np.zeros((0, 6), np.float32), torch.zeros((0, 6), device="cuda:0")):
        e = ctx.extract_shot_features(empty, 0.2, 10, "usc", return_frames=True)
        assert e[0].shape == (0, 128) and e[1].shape == (0, 9) and e[2].shape == (0,)


def test_the_intended_code_ran(ctx):
    """the profile rows: no fallback launch where every ball is full, both where some are not, two chunks of lists in the chunked case"""
    def rows(name, variant="shot"):
        c = CASES.case(name)
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            ctx.extract_shot_features(c["np6"], c["radius"], c["k"], variant)
            return ctx.profile_read()
        finally:
            ctx.profile_enable(False)
    full = rows("list_lengths")
    assert full["shot_ball"][0] == 1 and "shot_knn_fallback" not in full and "shot_fallback" not in full
    mixed = rows("bumpy_mixed", "usc")
    assert mixed["shot_ball"][0] == 1 and mixed["shot_knn_fallback"][0] == 1 and mixed["shot_fallback"][0] == 1
    chunked = rows("chunked")
    assert chunked["shot_knn_fallback"][0] == 2 and chunked["shot_fallback"][0] == 2
    want = CASES.expected("chunked", "shot")
    assert (want["flags"] & _lib.TC_SHOT_ROAD_MASK == _lib.TC_SHOT_ROAD_FALLBACK).all() and (want["length"] == CASES.K_MAX - 1).all()


def test_errors_and_the_context_serves_the_next_call(ctx):
    import threecrate_amd as tc
    c = CASES.case("blocks_64")
    with pytest.raises(tc.Unsupported, match="k_neighbors > 2047"):
        ctx.extract_shot_features(c["np6"], 0.1, 2048)
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(tc.InvalidData, match="search_radius must be positive"):
            ctx.extract_shot_features(c["np6"], r, 10)
    with pytest.raises(tc.InvalidData, match="variant"):
        ctx.extract_shot_features(c["np6"], 0.1, 10, "fpfh")
    d, f, fl = _run(ctx, "host", c["np6"], c["radius"], c["k"], "shot")
    want = CASES.expected("blocks_64", "shot")
    assert not SC.compare(d, f, fl, want)


def test_compat_mirrors_the_references_names(ctx):
    import threecrate_amd.compat as threecrate
    c = CASES.case("blocks_257")
    cloud = threecrate.NormalPointCloud.from_numpy(np.array(c["np6"][:, :3]), np.array(c["np6"][:, 3:]))
    for variant, dim in ((threecrate.ShotVariant.Standard, 352), (threecrate.ShotVariant.UniqueShapeContext, 128)):
        rows = threecrate.extract_shot_features_with_normals(cloud, threecrate.ShotConfig(search_radius=c["radius"], k_neighbors=c["k"], variant=variant))
        assert isinstance(rows, list) and len(rows) == 257 and all(len(r) == dim for r in rows)
        assert np.array(rows, np.float32).tobytes() == ctx.extract_shot_features(c["np6"], c["radius"], c["k"], variant).tobytes()
    cfg = threecrate.ShotConfig()
    assert (cfg.search_radius, cfg.k_neighbors, cfg.variant) == (0.2, 10, threecrate.ShotVariant.Standard)
    assert threecrate.extract_shot_features_with_normals(threecrate.NormalPointCloud()) == []
    with pytest.raises(RuntimeError, match="search_radius must be positive"):
        threecrate.extract_shot_features_with_normals(cloud, threecrate.ShotConfig(search_radius=0.0))
