"""One table of edge cases for NDT (csrc/ndt.hip, include/threecrate_hip_ndt.h), read by tests/test_ndt_edges_cpu.py (which proves on the
checker alone what every case is there for) and by tests/test_gpu_ndt_edges.py (which runs them on the device).  The contract is
tests/ndt_checker.py with key_dtype = float32 and dtype = float64: the header's keys -- floor(x / res) in f32 with true division,
saturating to the i32 range -- and f64 sums.  Its answers are computed once per process.

Which code a case reaches.  ndt_evaluate_kernel runs min(ceil(ns / 256), 1024) blocks of 256 (EVAL_SPAN = 262 144 points before a
lane takes a second one); ndt_finalize_kernel folds that many rows in 8 segments; runs of more than LONG_RUN = 128 points are listed
and get a block each, from a launch of at most 1 024 blocks; a key box of up to 2^24 cells gets the dense table, a larger one the hash
table of the smallest power of two >= 2 V slots; a key box that needs more than 64 bits (bits_for(dim - 1) per axis) is Unsupported.

Families: faces (points on and one float either side of voxel faces, as target and as source), saturated (keys at INT32_MAX / MIN, the
64- and 65-bit key boxes), long_source (source sizes around EVAL_SPAN), many_long_runs (more listed runs than the launch has blocks),
degenerate (voxels of identical, collinear, coplanar points; min_points 0 and 1), own_points (the target's own points as source, both
tables), nonfinite_source, shifted (the pair 2^10 ... 2^13 from the origin: the map, one step, loops of 3 ... 35 iterations)."""
import collections
import functools

import numpy as np

from tests import ndt_checker as NC

F = np.float32
LONG_RUN = 128
EVAL_SPAN = 1024 * 256
DENSE_CELLS = 2 ** 24

Case = collections.namedtuple("Case", "family name kind input params")
# kind "voxels": input -> (cloud,), params (res, min_points, tight: every voxel is held to the one-ulp bound)
# kind "register": input -> (source, target, init), params = register()'s keywords; expect: "budget" | "own" | "twin"
# kind "unsupported": input -> (source, target, init), params (res,)


def _ro(a):
    a = np.ascontiguousarray(a, F)
    a.setflags(write=False)
    return a


def bits_for(v):
    """bits that hold 0 .. v, at least 1 (bits_for_value of grid.hip)"""
    return max(1, int(v).bit_length())


def key_box_bits(cloud, res):
    k = NC.keys_of(np.asarray(cloud, F)[np.isfinite(cloud).all(axis=1)], res, F)
    dims = k.max(axis=0) - k.min(axis=0) + 1
    return [bits_for(int(d) - 1) for d in dims], float(np.prod(dims.astype(np.float64)))


# ---- 1. faces -----------------------------------------------------------------------------------------------------------------------
FACE_RES = (0.1, 0.3, 1.0 / 3.0, 0.7, 0.5)                      # the last is dyadic: every rule agrees there (the control)
FACE_J = 40


def face_sites(res, axis, step=None, shift=0.0):
    """243 sites: coordinate `axis` is j * f32(res), j in [-40, 40], and the float either side (or `step` either side), less `shift`; the
    other two coordinates sit at half a cell"""
    r = F(res)
    x = (np.arange(-FACE_J, FACE_J + 1).astype(F) * r).astype(F)
    lo, hi = (np.nextafter(x, F(-np.inf)), np.nextafter(x, F(np.inf))) if step is None else (x - F(step), x + F(step))
    xs = np.concatenate([lo, x, hi]).astype(F)
    p = np.empty((len(xs), 3), F)
    p[:] = F(0.5) * r
    p[:, axis] = xs
    return p - np.asarray(shift, F)


@functools.lru_cache(None)
def faces_cloud(res, step=None, shift=(0.0, 0.0, 0.0)):
    """five points per site, the four extra ones a quarter cell off along the other two axes only; shuffled.  3 645 points"""
    out = []
    for axis in range(3):
        s = face_sites(res, axis, step, 0.0)
        b, c = [a for a in range(3) if a != axis]
        out.append(s)
        for sb, sc in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            e = s.copy()
            e[:, b] += F(sb * 0.25) * F(res)
            e[:, c] += F(sc * 0.25) * F(res)
            out.append(e)
    p = np.concatenate(out) - np.asarray(shift, F)
    return _ro(np.random.default_rng(11).permutation(p))


@functools.lru_cache(None)
def faces_target(res):
    """every cell a site can fall into, by any rule: keys -42 .. 41 along each axis through the cell (0, 0, 0), eight points each, spread
    over [0.1, 0.5] of the cell on every axis -- the mean sits 0.3 into the cell, so a point on a face is 0.3 cells from the mean of the
    cell above and 0.7 from the mean of the cell below: a wrong key changes its e by orders of magnitude"""
    rng = np.random.default_rng(12)
    cells = {(0, 0, 0)}
    for axis in range(3):
        for k in range(-FACE_J - 2, FACE_J + 2):
            c = [0, 0, 0]
            c[axis] = k
            cells.add(tuple(c))
    cells = np.array(sorted(cells), np.float64)
    pts = (cells[:, None, :] + rng.uniform(0.1, 0.5, (len(cells), 8, 3))) * float(F(res))
    return _ro(rng.permutation(pts.reshape(-1, 3)))


FACE_SHIFT = (3 * 2.0 ** -4, -5 * 2.0 ** -4, 2.0 ** -4)         # the translated variants: x - t and (x - t) + t are exact on the 2^-10 grid
FACE_GRID = 2.0 ** -10


def faces_source_input(res, translated):
    if not translated:
        return faces_cloud(res), faces_target(res), NC.IDENTITY.copy()
    return faces_cloud(res, FACE_GRID, FACE_SHIFT), faces_target(res), np.r_[NC.IDENTITY[:4], FACE_SHIFT].astype(F)


# ---- 2. saturated -------------------------------------------------------------------------------------------------------------------
FAR = 3.0e9                                                     # x / 1.0 >= 2^31: the key saturates; one f32 ulp there is 256
FAR_SOURCE = 3.5e9


def _cells_cloud(cells, per, seed):
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.float64)
    return (cells[:, None, :] + rng.uniform(0.1, 0.9, (len(cells), per, 3))).reshape(-1, 3)


def _far(axis, sign, at=FAR):
    p = np.full((6, 3), 0.5)
    p[:, axis] = sign * (at + 256.0 * np.arange(6))
    return p


@functools.lru_cache(None)
def saturated(which):
    """-> (source, target).  'pos' / 'neg' / 'both': the eight cells around the origin (40 points) + six points beyond +-3e9 on x;
    'bits64' / 'bits65': cells 0 .. 1 in x and y, 4 or 5 cells in z, far voxels on +x and +y (31 + 31 + 2 or 3 bits); 'xyz': far voxels
    on +x, +y and +z.  The source is the near points moved by 0.01 (no face is nearer than 0.1) and points beyond every far voxel."""
    if which in ("pos", "neg", "both"):
        near = _cells_cloud([(i, j, k) for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)], 5, 21)
        far = [_far(0, s) for s in ((1,) if which == "pos" else (-1,) if which == "neg" else (1, -1))]
        probes = [np.array([[s * (FAR_SOURCE + 256.0 * i), 0.5, 0.5] for i in range(2 + (s > 0))]) for s in ((1, -1) if which == "both" else (1,) if which == "pos" else (-1,))]
    else:
        nz = {"bits64": 4, "bits65": 5, "xyz": 4}[which]
        near = _cells_cloud([(i, j, k) for i in (0, 1) for j in (0, 1) for k in range(-2, nz - 2)], 5, 22)
        axes = (0, 1, 2) if which == "xyz" else (0, 1)
        far = [_far(a, 1) for a in axes]
        probes = [_far(a, 1, FAR_SOURCE)[:2 + a] for a in axes]
    target = np.random.default_rng(23).permutation(np.concatenate([near] + far))
    source = np.concatenate([near + 0.01] + probes + [np.array([[0.5, 0.5, 700.0]])])     # the last one misses
    return _ro(source), _ro(target)


# ---- 3. long_source -----------------------------------------------------------------------------------------------------------------
LONG_NS = (EVAL_SPAN - 1, EVAL_SPAN, EVAL_SPAN + 1, EVAL_SPAN + 257, 2 * EVAL_SPAN + 1)


@functools.lru_cache(None)
def long_target():
    return _ro(NC.surface(20000, 1))


@functools.lru_cache(None)
def long_source(ns):
    """the first ns points of one sample of the surface, every third one moved 50 out in y: a lost or repeated stride changes n_hits"""
    p = NC.surface(2 * EVAL_SPAN + 1, 31).copy()
    p[::3, 1] += F(50.0)
    return _ro(p[:ns])


# ---- 4. many_long_runs --------------------------------------------------------------------------------------------------------------
MANY_LONG, MANY_LONG_POINTS, MANY_SHORT = 1100, LONG_RUN + 1, 300
SINGLE_RUNS = (256, 257, 512, 513, 1025)


@functools.lru_cache(None)
def many_long_runs():
    """1 100 voxels of 129 points among 300 of 6, on a 16-wide lattice that straddles the origin; long and short ones interleaved"""
    rng = np.random.default_rng(41)
    v = MANY_LONG + MANY_SHORT
    cells = np.array([[i % 16 - 8, (i // 16) % 16 - 8, i // 256 - 1] for i in range(v)], np.float64)
    long_ones = np.zeros(v, bool)
    long_ones[rng.permutation(v)[:MANY_LONG]] = True
    pts = [c + rng.uniform(0.05, 0.95, (MANY_LONG_POINTS if l else 6, 3)) for c, l in zip(cells, long_ones)]
    return _ro(rng.permutation(np.concatenate(pts)))


@functools.lru_cache(None)
def single_runs():
    rng = np.random.default_rng(42)
    pts = [np.array([3.0 * i - 6, 0, 0]) + rng.uniform(0.05, 0.95, (m, 3)) for i, m in enumerate(SINGLE_RUNS)]
    return _ro(rng.permutation(np.concatenate(pts)))


# ---- 5. degenerate ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def degenerate():
    """cell (0, 0, 0): five identical points; (2, 0, 0): five on a line along x; (4, 0, 0): six in the plane z = 0.375; (-3, 1, -2): five
    identical points away from the axes"""
    same = np.tile([[0.3, 0.7, 0.55]], (5, 1))
    line = np.array([[2.1 + 0.17 * i, 0.4, 0.6] for i in range(5)])
    plane = np.array([[4.2, 0.2, 0.375], [4.8, 0.3, 0.375], [4.5, 0.9, 0.375], [4.3, 0.6, 0.375], [4.7, 0.7, 0.375], [4.6, 0.1, 0.375]])
    same2 = np.tile([[-2.3, 1.1, -1.9]], (5, 1))
    return _ro(np.random.default_rng(51).permutation(np.concatenate([same, line, plane, same2])))


@functools.lru_cache(None)
def scattered(n=500):
    """n points with distinct keys at resolution 1"""
    rng = np.random.default_rng(52)
    cells = rng.permutation(20 ** 3)[:n]
    cells = np.stack([cells % 20 - 10, (cells // 20) % 20 - 10, cells // 400 - 10], axis=1).astype(np.float64)
    return _ro(cells + rng.uniform(0.1, 0.9, (n, 3)))


# ---- 6. own_points ------------------------------------------------------------------------------------------------------------------
OWN_N, OWN_RES = 20000, 0.5


@functools.lru_cache(None)
def own_points(spread):
    """-> (source, target): OWN_N points in distinct cells of a 40 x 40 x 32 lattice of cells (stride 1: 51 200 cells, the dense table;
    stride 16: 2 * 10^8 cells, the hash table of 65 536 slots), the box's two corners among them; the source is the target's points followed
    by as many points in unoccupied cells of the same lattice"""
    rng = np.random.default_rng(61)
    ids = rng.permutation(np.arange(1, 40 * 40 * 32 - 1))[:2 * OWN_N - 2]
    ids = np.r_[0, 40 * 40 * 32 - 1, ids]                        # occupied: the first OWN_N
    cells = np.stack([ids % 40, (ids // 40) % 40, ids // 1600], axis=1).astype(np.float64) * (16 if spread else 1) - (300 if spread else 20)
    pts = ((cells + rng.uniform(0.25, 0.75, (len(ids), 3))) * OWN_RES).astype(F)
    target = pts[:OWN_N]
    order = rng.permutation(OWN_N)
    return _ro(np.concatenate([target[order], pts[OWN_N:]])), _ro(target)


# ---- 7. nonfinite_source ------------------------------------------------------------------------------------------------------------
NONFINITE_ROWS = ((0, (np.nan, 0.1, 0.1)), (1, (0.2, 3e38, 0.1)), (1024, (0.1, np.inf, 0.0)), (2047, (-np.inf, -np.inf, 0.3)))
NONFINITE_ITERS = 3


@functools.lru_cache(None)
def nonfinite_source(twin):
    """the 2 048-point source of the small pair with NaN, 3e38, +inf and -inf rows at 0, 1, n / 2 and n - 1; the twin has those rows 100
    cells outside the key box instead"""
    src, tgt, init = NC.surface_pair(4096, 2048, 0.5)
    src = src.copy()
    for i, (row, bad) in enumerate(NONFINITE_ROWS):
        src[row] = (100.0 + i, 100.0, 100.0) if twin else bad
    return _ro(src), tgt, init


# ---- 8. shifted ---------------------------------------------------------------------------------------------------------------------
SHIFTS = ((2.0 ** 10, 2.0 ** 10, 0.0), (2.0 ** 13, -2.0 ** 13, 2.0 ** 10))


SHIFT_LOOPS = ((3, 5), (5, 35))                                 # iterations of the multi-step cases per shift; 35 is the default run
# (at 2^10 the cleaning for 35 iterations runs out of replacement points, at 2^13 it succeeds: there the default run is a case)


def shifted(offset, iterations=1):
    """the small pair moved by `offset`, the start rotation about the patch's centre, cleaned for the loop it runs (ndt_checker.surface_pair:
    in none of its evaluations a point near a face or with other keys in f32 than in f64)"""
    return NC.surface_pair(4096, 2048, 0.5, offset=offset, **(dict(max_iterations=iterations) if iterations != 1 else {}))


# ---- the table ----------------------------------------------------------------------------------------------------------------------
BUILDERS = {
    "faces": lambda res: (faces_cloud(res),),
    "faces_source": faces_source_input,
    "saturated": lambda which: saturated(which) + (NC.IDENTITY.copy(),),
    "saturated_target": lambda which: (saturated(which)[1],),
    "long_source": lambda ns: (long_source(ns), long_target(), NC.start_pose()),
    "many_long_runs": lambda: (many_long_runs(),),
    "single_runs": lambda: (single_runs(),),
    "degenerate": lambda: (degenerate(),),
    "scattered": lambda: (scattered(),),
    "own_points": lambda spread: own_points(spread) + (NC.IDENTITY.copy(),),
    "nonfinite_source": nonfinite_source,
    "shifted": shifted,
    "shifted_target": lambda offset: (shifted(offset)[1],),
    "lattice257": lambda: (lattice_cloud(257),),
    "surface4096": lambda: (NC.surface_pair(4096, 2048, 0.5)[1],),
}


def lattice_cloud(v, per_voxel=6, seed=0):
    """tests/test_gpu_ndt.py's lattice: v voxels of resolution 1 along a 16-wide lattice that straddles the origin, per_voxel points each"""
    rng = np.random.default_rng(seed)
    cells = np.array([[i % 16 - 8, (i // 16) % 16 - 8, i // 256 - 1] for i in range(v)], np.float64)
    pts = cells[:, None, :] + rng.uniform(0.05, 0.95, (v, per_voxel, 3))
    return rng.permutation(pts.reshape(-1, 3)).astype(F)


def case_input(c):
    return BUILDERS[c.input[0]](*c.input[1:])


def case_id(c):
    return f"{c.family}-{c.name}"


def _res_name(res):
    return {0.1: "0.1", 0.3: "0.3", 1.0 / 3.0: "third", 0.7: "0.7", 0.5: "0.5", 0.25: "0.25"}[res]


@functools.lru_cache(None)
def cases():
    out = []
    one = dict(max_iterations=1)
    for res in FACE_RES:
        out.append(Case("faces", f"res{_res_name(res)}", "voxels", ("faces", res), (res, 5, True)))
    for res in FACE_RES:
        out.append(Case("faces_source", f"res{_res_name(res)}-identity", "register", ("faces_source", res, False), dict(one, resolution=res, expect="budget")))
    for res in (0.5, 0.25):
        out.append(Case("faces_source", f"res{_res_name(res)}-translated", "register", ("faces_source", res, True), dict(one, resolution=res, expect="budget")))
    for which in ("pos", "neg", "both", "bits64"):
        out.append(Case("saturated", f"{which}-map", "voxels", ("saturated_target", which), (1.0, 5, False)))
        out.append(Case("saturated", which, "register", ("saturated", which), dict(one, resolution=1.0, expect="budget")))
    for which in ("bits65", "xyz"):
        out.append(Case("saturated", which, "unsupported", ("saturated", which), (1.0,)))
    for ns in LONG_NS:
        out.append(Case("long_source", f"ns{ns}", "register", ("long_source", ns), dict(one, resolution=0.25, expect="budget")))
    out.append(Case("many_long_runs", "1100x129", "voxels", ("many_long_runs",), (1.0, 5, True)))
    out.append(Case("many_long_runs", "single", "voxels", ("single_runs",), (1.0, 5, True)))
    out.append(Case("degenerate", "voxels", "voxels", ("degenerate",), (1.0, 5, True)))
    for m in (0, 1):
        out.append(Case("degenerate", f"scattered-min{m}", "voxels", ("scattered",), (1.0, m, True)))
    for spread in (False, True):
        out.append(Case("own_points", "hash" if spread else "dense", "register", ("own_points", spread),
                        dict(resolution=OWN_RES, min_points_per_voxel=1, max_iterations=5, expect="own")))
    out.append(Case("nonfinite_source", "rows", "register", ("nonfinite_source", False), dict(resolution=0.5, max_iterations=NONFINITE_ITERS, epsilon=0.0, expect="twin")))
    for i, off in enumerate(SHIFTS):
        out.append(Case("shifted", f"by{i}-map", "voxels", ("shifted_target", off), (0.5, 5, True)))
        out.append(Case("shifted", f"by{i}-step", "register", ("shifted", off), dict(one, resolution=0.5, expect="budget")))
        for its in SHIFT_LOOPS[i]:
            out.append(Case("shifted", f"by{i}-" + ("default" if its == 35 else f"iters{its}"), "register", ("shifted", off, its),
                            dict(resolution=0.5, expect="budget", **({} if its == 35 else dict(max_iterations=its)))))
    out.append(Case("existing", "lattice257", "voxels", ("lattice257",), (1.0, 5, True)))
    out.append(Case("existing", "surface4096", "voxels", ("surface4096",), (0.5, 5, True)))
    return tuple(out)


def of(kind, family=None):
    return [c for c in cases() if c.kind == kind and (family is None or c.family == family)]


# ---- the checker's answers, once per process ----------------------------------------------------------------------------------------
def by_id(cid):
    return {case_id(c): c for c in cases()}[cid]


@functools.lru_cache(None)
def _ref_voxels(cid):
    c = by_id(cid)
    res, min_points, _ = c.params
    return NC.build(case_input(c)[0], res, min_points, np.float64, key_dtype=F)


def ref_voxels(c):
    """the yardstick's map of a "voxels" case: the header's keys, f64 sums"""
    return _ref_voxels(case_id(c))


def loop_of(c):
    return {k: v for k, v in c.params.items() if k != "expect"}


def ref_runs(c):
    """a "register" case's two runs with the header's keys: the reference's arithmetic (f32) and the yardstick (f64)"""
    return _ref_runs(case_id(c))


@functools.lru_cache(None)
def _ref_runs(cid):
    c = by_id(cid)
    src, tgt, init = case_input(c)
    kw = loop_of(c)
    a = NC.register(src, tgt, init, dtype=np.float32, **kw)
    b = NC.register(src, tgt, init, dtype=np.float64, key_dtype=F, **kw)
    return a, b


def budget(c):
    """the project's rule: 4 x the reference's own f32-to-f64 distance on this input (pose: Frobenius of the 4 x 4; score: relative)"""
    a, b = ref_runs(c)
    fro, rel = NC.distances(a, b)
    return 4 * fro, 4 * rel


# ---- the tight bound of the voxel map -------------------------------------------------------------------------------------------------
# The device forms mean, centred covariance and the inverse in f64 and rounds once: the mean is within one f32 ulp of the yardstick's
# f64 mean rounded to f32 (the half ulp of the rounding plus f64 noise that can flip it), inv_cov element by element within one f32 ulp
# of the element plus 2^-40 of the matrix's largest element -- the f64 cancellation floor of the adjugate at cond <= COND_MAX, which
# tests/test_ndt_edges_cpu.py proves against exact rationals.
COND_MAX = 1e4
INV_FLOOR = 2.0 ** -40
IU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(F)
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)


def voxel_conds(grid):
    """cond(cov + 1e-4 I) = cond(inv_cov) per voxel"""
    return np.array([np.linalg.cond(m) for m in grid[3]]) if len(grid[3]) else np.zeros(0)


def voxel_excess(mean, inv6, grid, tight=None):
    """by how much the worst mean and the worst inv_cov element of a map (mean (V, 3), inv6 (V, 6)) miss the tight bound, in units of the
    bound (<= 1 passes), over the voxels of `tight` (a mask; default all)"""
    ref_mean, ref_inv = grid[2], np.stack([grid[3][:, i, j] for i, j in IU], axis=1)
    want = ref_mean.astype(F).astype(np.float64)
    em = np.abs(np.asarray(mean, np.float64) - want) / ulp32(want)
    ei = np.abs(np.asarray(inv6, np.float64) - ref_inv) / (ulp32(ref_inv) + INV_FLOOR * np.abs(ref_inv).max(axis=1, keepdims=True))
    if tight is not None:
        em, ei = em[tight], ei[tight]
    return (float(em.max()) if em.size else 0.0), (float(ei.max()) if ei.size else 0.0)
