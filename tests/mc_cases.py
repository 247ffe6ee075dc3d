"""The marching-cubes case table of the tests (test infrastructure): read by tests/test_mc_table_cpu.py (mutants of the checker) and by
tests/test_gpu_mc.py (the device against the checker).  A case is a dict of the arguments both take: values (flat, in `layout`), dims,
voxel_size, origin, iso_level, valid (or None), layout.  The shapes are the smallest at which the device code can go wrong
(tests/test_gpu_mc.py says which path each one reaches)."""
import numpy as np

from threecrate_amd import synth
from tests import mc_checker as K

SCAN_TILE = 2048        # kScanTile of csrc/grid.hip (kScanItems 8 x kScanBlock 256); tests/test_gpu_mc.py reads it from the source too


def case(values, dims, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), iso_level=0.0, valid=None, layout="z_fastest"):
    values = np.ascontiguousarray(values, np.float32).reshape(-1)
    assert values.size == dims[0] * dims[1] * dims[2]
    return dict(values=values, dims=tuple(dims), voxel_size=tuple(voxel_size), origin=tuple(origin), iso_level=iso_level,
                valid=None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1), layout=layout)


def from_xyz(v_xyz, layout):
    """an array indexed [x, y, z] as the flat array of `layout`"""
    return np.ascontiguousarray(v_xyz if layout == "z_fastest" else v_xyz.transpose(2, 1, 0)).reshape(-1)


def one_cube(c, layout):
    """a 2 x 2 x 2 grid whose single cube has case c: -1 at the inside corners, +1 at the others"""
    v = np.ones((2, 2, 2), np.float32)
    for k, (x, y, z) in enumerate(K.G.CORNERS):
        if (c >> k) & 1:
            v[x, y, z] = -1.0
    return case(from_xyz(v, layout), (2, 2, 2), layout=layout)


def alternating(dims, layout):
    """+1 / -1 by the parity of x + y + z: every cube emits"""
    x, y, z = np.meshgrid(*[np.arange(d) for d in dims], indexing="ij")
    return case(from_xyz(np.where((x + y + z) % 2 == 0, 1.0, -1.0).astype(np.float32), layout), dims, layout=layout)


def random_field(dims, seed, layout="z_fastest", **kw):
    v = np.random.default_rng(seed).standard_normal(dims).astype(np.float32)
    return case(from_xyz(v, layout), dims, layout=layout, **kw)


ANISO = dict(voxel_size=(0.1, 0.25, 0.5), origin=(-3.0, 7.0, 0.5))


def exact_values(iso):
    """values equal to iso at corners, and pairs whose difference is just below and just above 1e-6"""
    v = np.random.default_rng(11).standard_normal((5, 5, 5)).astype(np.float32) + np.float32(iso)
    f = np.float32
    v[1, 1, 1] = v[3, 2, 1] = v[2, 2, 2] = v[0, 0, 0] = v[4, 4, 4] = f(iso)
    lo = np.nextafter(f(iso), f(-np.inf))
    v[1, 3, 3], v[2, 3, 3] = lo, f(lo + f(0.9e-6))          # |vb - va| just below 1e-6, the ends on both sides of iso
    v[3, 1, 3], v[3, 2, 3] = lo, f(lo + f(1.1e-6))          # just above
    v[3, 3, 0], v[3, 3, 1] = f(iso + f(0.4e-6)), f(iso - f(0.4e-6))
    return case(v, (5, 5, 5), iso_level=iso, **ANISO)


def unusable():
    """NaN at voxel 0 (and at one more), +inf in the middle, -inf at the last voxel.  A NaN reaches a normal only as a NaN gradient, which
    gives (0, 0, 1).  An infinite sample would give inf / inf; the 26 neighbours of an infinite voxel share its sign, so no vertex lies on
    an edge of a cube that has the voxel as a corner and no sample of any vertex reads it with a non-zero weight: no NaN in any output"""
    v = np.random.default_rng(7).standard_normal((9, 9, 9)).astype(np.float32)
    v[3:6, 3:6, 3:6], v[7:, 7:, 7:] = 5.0, -5.0
    v[4, 4, 4], v[8, 8, 8] = np.inf, -np.inf
    v[0, 0, 0] = v[1, 2, 1] = np.nan
    return case(v, (9, 9, 9), **ANISO)


def masked(fraction, seed=3):
    c = random_field((9, 9, 9), 7, **ANISO)
    c["valid"] = (np.random.default_rng(seed).random(9 ** 3) >= fraction).astype(np.uint8)
    return c


def sphere(res, layout="z_fastest"):
    v, vs, org = synth.sphere_volume((0.1, -0.2, 0.3), 1.0, (res,) * 3, (3.0, 3.0, 3.0))
    return case(from_xyz(v, layout), (res,) * 3, vs, org, layout=layout)


def box(res):
    v, vs, org = synth.box_volume((0.0, 0.0, 0.0), 0.75, (res,) * 3, (3.0, 3.0, 3.0))      # faces on grid planes: values equal to iso
    return case(v, (res,) * 3, vs, org)


def build():
    """name -> a function that makes the case (the large ones are made when asked for)"""
    t = {}
    for layout in ("z_fastest", "x_fastest"):
        for n in (256, 257, 258, SCAN_TILE // 4, SCAN_TILE // 4 + 1, SCAN_TILE + 1, SCAN_TILE + 2):    # n - 1 cubes and 4 n voxels: either side of a block, of a scan tile of voxels, of a scan tile of cubes
            t[f"line_z_{n}_{layout}"] = lambda n=n, layout=layout: alternating((2, 2, n), layout)
            t[f"line_x_{n}_{layout}"] = lambda n=n, layout=layout: alternating((n, 2, 2), layout)
        for dims in ((17, 5, 3), (3, 17, 5), (5, 3, 17), (17, 3, 5), (3, 5, 17), (5, 17, 3)):
            t["dims_%d_%d_%d_%s" % (dims + (layout,))] = lambda dims=dims, layout=layout: random_field(dims, 2, layout, **ANISO)
        t[f"random9_{layout}"] = lambda layout=layout: random_field((9, 9, 9), 7, layout, **ANISO)
        t[f"random9_iso037_{layout}"] = lambda layout=layout: random_field((9, 9, 9), 7, layout, iso_level=0.37, **ANISO)
    t["exact_iso0"] = lambda: exact_values(0.0)
    t["exact_iso037"] = lambda: exact_values(0.37)
    t["mask20"] = lambda: masked(0.2)
    t["mask_all"] = lambda: masked(2.0)
    t["unusable"] = unusable
    t["all_above"] = lambda: case(np.ones(125, np.float32), (5, 5, 5))
    t["dims_with_1_a"] = lambda: random_field((1, 9, 9), 4)
    t["dims_with_1_b"] = lambda: random_field((9, 1, 9), 4, "x_fastest")
    t["dims_with_1_c"] = lambda: random_field((9, 9, 1), 4)
    t["far_2e10"] = lambda: random_field((9, 9, 9), 7, voxel_size=ANISO["voxel_size"], origin=(-3.0 + 1024.0, 7.0 + 1024.0, 0.5 + 1024.0))
    t["far_2e13"] = lambda: random_field((9, 9, 9), 7, voxel_size=ANISO["voxel_size"], origin=(-3.0 + 8192.0, 7.0 + 8192.0, 0.5 + 8192.0))
    t["sphere33"] = lambda: sphere(33)
    t["sphere33_x"] = lambda: sphere(33, "x_fastest")
    t["box33"] = lambda: box(33)
    return t


CASES = build()
