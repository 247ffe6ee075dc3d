"""One table of colorization cases (include/threecrate_hip_color.h), read by tests/test_color_cpu.py (preconditions, mutants) and by
tests/test_gpu_color.py (the device against tests/color_checker.py, bit for bit).

Pixel coordinates are CONSTRUCTED, not random: with fx = fy = FOCAL a power of two, cx = cy = 0, c_z = 1 and an identity or
pure-translation matrix, x = u / FOCAL is exact and the device's u = (fx c_x) / c_z + cx is the intended float.  A case that states
`uv` has that asserted by the CPU file.  Each case: name -> dict(xyz, sources, cfg[, uv]); a source is (image, (fx, fy, cx, cy),
matrix of 12 floats[, depth])."""
import numpy as np

F = np.float32
FOCAL = 4.0
K0 = (FOCAL, FOCAL, 0.0, 0.0)
IDENTITY = np.eye(4, dtype=F)[:3].reshape(12)
SLICES = 16                     # kColorSlices of tc_internal.h: a block counts into slice blockIdx % 16
GREY = (128, 128, 128)


def shifted(tx=0.0, ty=0.0, tz=0.0):
    m = IDENTITY.copy()
    m[3], m[7], m[11] = tx, ty, tz
    return m


def image(w, h, seed):
    """random bytes, none of them a grey (128, 128, 128) pixel"""
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[(img == 128).all(axis=2)] = (127, 128, 129)
    return img


def at_pixels(u, v, z=1.0, shift_x=0.0):
    """the points that project to (u, v) through K0 at depth 1 of a camera shifted by shift_x"""
    u, v = np.asarray(u, F).reshape(-1), np.asarray(v, F).reshape(-1)
    return np.stack([u / F(FOCAL) + F(shift_x), v / F(FOCAL), np.full(len(u), z, F)], axis=1).astype(F)


def cfg(default_color=GREY, interpolation=1, min_depth=1e-4, depth_tolerance=0.05):
    return dict(default_color=tuple(default_color), interpolation=interpolation, min_depth=min_depth, depth_tolerance=depth_tolerance)


def _edges():
    out = {}
    for w, h in ((1, 1), (1, 5), (5, 1), (2, 2), (4, 4), (7, 5)):           # 7 x 5: a row of 21 bytes
        us, vs = np.arange(-1.5, w + 0.5 + 0.125, 0.25, dtype=F), np.arange(-1.5, h + 0.5 + 0.125, 0.25, dtype=F)
        u, v = (a.reshape(-1) for a in np.meshgrid(us, vs))
        for mode, name in ((1, "bilinear"), (0, "nearest")):
            out[f"edges_{w}x{h}_{name}"] = dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(image(w, h, 10 * w + h), K0, IDENTITY)],
                                                cfg=cfg(interpolation=mode))
    return out


# (c00, c10, tx): found by the search of tests/test_color_cpu.py::test_the_tie_inputs_are_what_the_search_finds.  HALF: val lands
# exactly on k + 0.5 and must round up (half-even rounds 0.5 and 2.5 down).  FUSED: the three-operation lerp gives exactly k + 0.5, the
# fused multiply-add a value just below it: they round to different bytes
TIES_HALF = ((0, 1, 0.5), (2, 3, 0.5), (4, 5, 0.5), (7, 4, 0.5), (255, 254, 0.5))
TIES_FUSED = ((1, 4, 0.166666641831398), (1, 6, 0.09999998658895493), (1, 11, 0.7499999403953552), (1, 19, 0.861111044883728))


def _ties():
    rows = TIES_HALF + TIES_FUSED
    img = np.zeros((2 * len(rows) + 1, 3, 3), np.uint8)         # pair r lives in rows 2r, 2r + 1 (both alike: ty does not matter), columns 0, 1
    u, v = [], []
    for r, (a, b, t) in enumerate(rows):
        img[2 * r:2 * r + 2, 0], img[2 * r:2 * r + 2, 1] = (a, a, a), (b, b, b)
        u.append(F(t)), v.append(F(2 * r))
    u, v = np.array(u, F), np.array(v, F)
    return {"ties": dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(img, K0, IDENTITY)], cfg=cfg(default_color=(9, 8, 7)))}


def _depth_gate():
    out = {}
    one = F(1)
    zs = np.array([np.nextafter(one, F(0)), one, np.nextafter(one, F(2)), F(-1)], F)     # min_depth = 1: below, at, above, behind
    pts = np.stack([np.zeros(4, F), np.zeros(4, F), zs], axis=1)
    for mode, name in ((1, "bilinear"), (0, "nearest")):
        out[f"depth_gate_min_depth_{name}"] = dict(xyz=pts, sources=[(image(4, 4, 3), K0, IDENTITY)], cfg=cfg(interpolation=mode, min_depth=1.0))
    lo, hi = F(0.75), F(1.25)                                   # c_z = 1, tolerance 0.25: both differences are exact
    depth = np.array([[0.0, lo, hi, np.nextafter(lo, F(0))],
                      [np.nextafter(hi, F(2)), 1.0, -1.0, np.nan],
                      [np.inf, -np.inf, np.nextafter(lo, F(1)), np.nextafter(hi, F(1))],
                      [1.0, 1.0, 1.0, 1.0]], F)
    u, v = (a.reshape(-1).astype(F) for a in np.meshgrid(np.arange(4), np.arange(4)))
    # bilinear neighbourhood inside, (xn, yn) the NEXT pixel: (0.75, 0.75) -> depth (1, 1) valid, (0, 0) not; (1.75, 0.75) -> (2, 1) not, (1, 0) valid
    u, v = np.concatenate([u, F([0.75, 1.75])]), np.concatenate([v, F([0.75, 0.75])])
    for mode, name in ((1, "bilinear"), (0, "nearest")):
        out[f"depth_gate_tolerance_{name}"] = dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(image(4, 4, 4), K0, IDENTITY, depth)],
                                                   cfg=cfg(interpolation=mode, depth_tolerance=0.25))
    return out


def _camera_row(k, seed):
    """k cameras side by side: camera s is shifted by s along x and sees x in [s, s + 1) as its 4 x 4 image"""
    return [(image(4, 4, seed + s), K0, shifted(tx=-float(s))) for s in range(k)]


def _sources():
    out = {}
    u, v = (a.reshape(-1).astype(F) for a in np.meshgrid(np.arange(4), np.arange(4)))
    for k in (2, 3, 4, 5):
        src = _camera_row(k, 20)
        out[f"sources_first_wins_{k}"] = dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(image(4, 4, 30 + s), K0, IDENTITY) for s in range(k)], cfg=cfg(interpolation=0))
        out[f"sources_only_last_sees_{k}"] = dict(xyz=at_pixels(u, v, shift_x=k - 1), sources=src, cfg=cfg())
        out[f"sources_nobody_sees_{k}"] = dict(xyz=at_pixels(u, v, shift_x=100.0), sources=src, cfg=cfg())
    grey = image(4, 4, 40)
    grey[:, :2] = GREY                                          # columns 0 and 1 ARE the default colour: they colour nothing
    out["sources_default_pixel_falls_through"] = dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(grey, K0, IDENTITY), (image(4, 4, 41), K0, IDENTITY)],
                                                      cfg=cfg(interpolation=0))
    out["sources_default_pixel_alone"] = dict(xyz=at_pixels(u, v), uv=(u, v), sources=[(grey, K0, IDENTITY)], cfg=cfg(interpolation=0))
    many = _camera_row(64, 100)                                 # TC_COLOR_MAX_SOURCES
    xyz = np.concatenate([at_pixels(u, v, shift_x=s) for s in range(64)])
    out["sources_max"] = dict(xyz=xyz, sources=many, cfg=cfg())
    return out


def _bad_points():
    u, v = F([0, 1, 2, 3, 0, 1, 2, 3, 1]), F([0, 0, 1, 1, 2, 2, 3, 3, 3])
    xyz = at_pixels(u, v)
    n = len(xyz)
    xyz[0, 0], xyz[n // 2, 1], xyz[n - 1, 2] = np.nan, np.inf, -np.inf
    out = {}
    for mode, name in ((1, "bilinear"), (0, "nearest")):
        out[f"bad_points_{name}"] = dict(xyz=xyz, sources=[(image(4, 4, 5), K0, IDENTITY)], cfg=cfg(interpolation=mode))
    # finite matrices that overflow: source 0 gives c_z = inf - inf = NaN (3), source 1 c_x = inf, u = inf (5); source 2 sees the points
    big = F(3e38)
    m_nan, m_inf = IDENTITY.copy(), IDENTITY.copy()
    m_nan[8], m_nan[9] = big, -big
    m_inf[0] = big
    pts = at_pixels(F([1, 2, 3]), F([1, 2, 3])) + F([2, 2, 0])
    src = [(image(4, 4, 6), K0, m_nan), (image(4, 4, 7), K0, m_inf), (image(4, 4, 8), K0, shifted(tx=-2.0, ty=-2.0))]
    out["bad_points_matrix_overflow"] = dict(xyz=pts, sources=src, cfg=cfg())
    return out


BLOCK_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513, SLICES * 256 + 1)


def _blocks():
    out = {}
    for n in BLOCK_SIZES:
        i = np.arange(n)
        u, v = (i % 4).astype(F), ((i // 4) % 4).astype(F)
        xyz = at_pixels(u, v)
        xyz[i % 3 == 1, 0] = 100.0                              # a miss every third point (n = 1: a hit; n = 2: one of each)
        out[f"blocks_{n}"] = dict(xyz=xyz, sources=[(image(4, 4, 9), K0, IDENTITY)], cfg=cfg())
    return out


def _reference_units():
    """the unit tests of colorization.rs:362-456 as literals: the 4 x 4 red image, fx = fy = 2, cx = cy = 1.5"""
    red, blue = np.tile(np.uint8([255, 0, 0]), (4, 4, 1)), np.tile(np.uint8([0, 0, 255]), (4, 4, 1))
    k = (2.0, 2.0, 1.5, 1.5)
    unit = lambda p, src, **c: dict(xyz=np.array([p], F), sources=src, cfg=cfg(**c))
    return {
        "reference_single_point_in_view": dict(unit((0, 0, 1), [(red, k, IDENTITY)]), want=([255, 0, 0], 1)),
        "reference_point_behind_camera": dict(unit((0, 0, -1), [(red, k, IDENTITY)], default_color=(0, 0, 0)), want=([0, 0, 0], 0)),
        "reference_point_out_of_frame": dict(unit((1000, 0, 1), [(red, k, IDENTITY)], default_color=(1, 2, 3)), want=([1, 2, 3], 0)),
        "reference_multi_image_first_wins": dict(unit((0, 0, 1), [(red, k, IDENTITY), (blue, k, IDENTITY)]), want=([255, 0, 0], 1)),
        "reference_camera_translated_along_x": dict(unit((1, 0, 1), [(red, k, shifted(tx=-1.0))]), want=([255, 0, 0], 1)),
    }


def _projection():
    """(fx c_x) / c_z against fx (c_x / c_z): found by search, the two round to different pixels (fx = 3, c_z = 5; u = 0.5 against
    0.49999997, 5.4999995 against 5.5)"""
    xyz = np.array([[0.8333333134651184, 0, 5], [9.166666030883789, 0, 5]], F)
    return {"projection_order": dict(xyz=xyz, sources=[(image(8, 2, 11), (3.0, 3.0, 0.0, 0.0), IDENTITY)], cfg=cfg(interpolation=0))}


CASES = {}
for _group in (_edges, _ties, _depth_gate, _sources, _bad_points, _blocks, _reference_units, _projection):
    CASES.update(_group())

# the rule of tests/color_checker.RULES -> the cases that tell its mutant from the contract
TELLS = {
    "min_depth_strict": ["depth_gate_min_depth_bilinear", "depth_gate_min_depth_nearest"],
    "round_half_even": ["edges_4x4_nearest", "ties"],
    "floor_trunc": ["edges_4x4_bilinear", "edges_7x5_bilinear"],
    "no_border_fallback": ["edges_4x4_bilinear", "edges_1x1_bilinear"],
    "fused_lerp": ["ties"],
    "val_trunc": ["edges_7x5_bilinear", "ties"],
    "default_is_hit": ["sources_default_pixel_falls_through", "sources_default_pixel_alone"],
    "last_wins": ["sources_first_wins_2", "sources_first_wins_5"],
    "depth_tol_strict": ["depth_gate_tolerance_bilinear", "depth_gate_tolerance_nearest"],
    "depth_at_floor": ["depth_gate_tolerance_bilinear"],
    "project_div_first": ["projection_order"],
    "nonfinite_point_samples": ["bad_points_bilinear", "bad_points_nearest"],
}
