"""The contract of include/threecrate_hip_voxelmap.h restated in numpy / plain Python (test infrastructure): the state of a streaming
voxel map after a sequence of chunks, bit for bit.  f32 where the reference is f32 (the key: x * inv, floor), f64 sums folded ONE point
at a time (a Python float is an IEEE f64 and `+` one correctly rounded add), a true f64 division for the centroid.

VoxelMapChecker(voxel_size, **mutant) -- every keyword turns ONE rule into a plausible wrong one; tests/test_voxelmap_cpu.py shows that
each mutant is told apart from the real checker by a named input of tests/voxelmap_cases.py, which tests/test_gpu_voxelmap.py also runs
on the device."""
import numpy as np

KEY_LIMIT = 1 << 20
MIN_CAPACITY, DEFAULT_CAPACITY, MAX_CAPACITY = 1 << 8, 1 << 16, 1 << 28
LONG_RUN = 96               # kVoxelMapLongRun of voxelmap.hip: a longer run of one chunk is folded by a wave


class OutOfRange(Exception):
    """some point of the chunk has a key outside the limit: the insert is refused and the state is what it was"""


class VoxelMapChecker:
    def __init__(self, voxel_size, divide=False, truncate=False, nan_key=0, descending=False, per_chunk=False, reciprocal=False,
                 unsigned_order=False, limit_lo=-KEY_LIMIT, limit_hi=KEY_LIMIT):
        self.voxel_size = np.float32(voxel_size)
        with np.errstate(divide="ignore"):
            self.inv = np.float32(1.0) / self.voxel_size
        self.m = dict(divide=divide, truncate=truncate, nan_key=nan_key, descending=descending, per_chunk=per_chunk, reciprocal=reciprocal,
                      unsigned_order=unsigned_order, limit_lo=limit_lo, limit_hi=limit_hi)
        self.voxels = {}            # (kx, ky, kz) -> [sx, sy, sz, count]
        self.points = 0

    def keys_of(self, pts):
        """(n, 3) int64 keys and (n,) validity of every point"""
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            p = (pts / self.voxel_size) if self.m["divide"] else (pts * self.inv)      # f32 x f32 -> f32
            assert p.dtype == np.float32
            f = np.trunc(p) if self.m["truncate"] else np.floor(p)
        nan = np.isnan(p)
        ok = nan | ((f >= np.float32(self.m["limit_lo"])) & (f < np.float32(self.m["limit_hi"])))
        k = np.where(nan, self.m["nan_key"], np.where(ok, f, 0)).astype(np.int64)
        return k, ok.all(axis=1)

    def insert(self, pts):
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        if len(pts) == 0:
            return
        k, ok = self.keys_of(pts)
        if not ok.all():
            raise OutOfRange(int(np.nonzero(~ok)[0][0]))
        into = {} if self.m["per_chunk"] else self.voxels
        order = range(len(pts) - 1, -1, -1) if self.m["descending"] else range(len(pts))
        kl, pl = k.tolist(), pts.astype(np.float64).tolist()         # f32 -> f64 is exact
        for i in order:
            v = into.get(tuple(kl[i]))
            if v is None:
                v = into[tuple(kl[i])] = [0.0, 0.0, 0.0, 0]
            x, y, z = pl[i]
            v[0] = v[0] + x; v[1] = v[1] + y; v[2] = v[2] + z; v[3] += 1
        if self.m["per_chunk"]:
            for key, c in into.items():
                v = self.voxels.setdefault(key, [0.0, 0.0, 0.0, 0])
                v[0] = v[0] + c[0]; v[1] = v[1] + c[1]; v[2] = v[2] + c[2]; v[3] += c[3]
        self.points += len(pts)

    def __len__(self):
        return len(self.voxels)

    def reset(self):
        self.voxels, self.points = {}, 0

    def extract(self):
        """-> centroids (V, 3) f32, keys (V, 3) int32, counts (V,) uint32, sums (V, 3) f64, in extraction order"""
        if self.m["unsigned_order"]:
            ks = sorted(self.voxels, key=lambda k: tuple(c & 0xFFFFFFFF for c in k))
        else:
            ks = sorted(self.voxels)
        keys = np.array(ks, np.int32).reshape(-1, 3)
        counts = np.array([self.voxels[k][3] for k in ks], np.uint32)
        sums = np.array([self.voxels[k][:3] for k in ks], np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            n = counts.astype(np.float64)[:, None]
            cent = (sums * (1.0 / n) if self.m["reciprocal"] else sums / n).astype(np.float32)
        return cent, keys, counts, sums


def run(voxel_size, chunks, **mutant):
    c = VoxelMapChecker(voxel_size, **mutant)
    for ch in chunks:
        c.insert(ch)
    return c


def same_bits(a, b):
    """equal shapes, dtypes and bits; a NaN equals a NaN (its sign and payload are unspecified)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def same_state(a, b):
    """two extract() results (centroids, keys, counts, sums)"""
    return all(same_bits(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def slots_after(slots, v, r):
    """the table's size after a chunk of r distinct voxels meets a map of v voxels: doubled while 2 (v + r) > slots"""
    while 2 * (v + r) > slots:
        slots *= 2
    return slots
