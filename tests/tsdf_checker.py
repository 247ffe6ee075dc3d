"""The contract of TSDF fusion and surface extraction (include/threecrate_hip_tsdf.h), restated with numpy float32 arrays: the same
operations in the same order, one rounding each, so the device's results are compared with these bit for bit (tests/test_gpu_tsdf.py).
tests/test_tsdf_cpu.py proves, on this file alone, what every GPU input is there for, and that the mutants below (a rule changed the
way an implementation might get it wrong) are told apart by them.

Also here: the inputs both test files share (SCENE, integration_cases, extraction_states).  Everything is generated from fixed
formulas; nothing is random."""
import numpy as np

F = np.float32
U32 = np.uint32

OBSERVED_EDGES = 1
INTEGRATE_MUTANTS = ("no_half", "uv_exchanged", "alpha_from_old_weight")
EXTRACT_MUTANTS = ("lt_for_le", "tau_minus_iso", "yz_edges_exchanged", "colour_from_far_corner")

# the 12 edges in the shader's order as (corner a, corner b, axis), corner = x + 2 y + 4 z
EDGES = [(0, 1, 0), (2, 3, 0), (4, 5, 0), (6, 7, 0), (0, 2, 1), (1, 3, 1), (4, 6, 1), (5, 7, 1), (0, 4, 2), (1, 5, 2), (2, 6, 2), (3, 7, 2)]


class Volume:
    def __init__(self, voxel_size, truncation_distance, resolution, origin=(0, 0, 0), max_weight=100):
        self.vs, self.tau = F(voxel_size), F(truncation_distance)
        self.res = tuple(int(r) for r in resolution)
        self.origin = np.asarray(origin, F)
        self.max_weight = int(max_weight)
        self.n = self.res[0] * self.res[1] * self.res[2]
        self.reset()

    def reset(self):
        self.tsdf = np.ones(self.n, F)
        self.weight = np.zeros(self.n, np.uint8)
        self.rgb = np.zeros((self.n, 3), np.uint8)

    def load(self, tsdf, weight, rgb=None):
        self.tsdf = np.asarray(tsdf, F).reshape(self.n).copy()
        self.weight = np.asarray(weight, np.uint8).reshape(self.n).copy()
        self.rgb = np.zeros((self.n, 3), np.uint8) if rgb is None else np.asarray(rgb, np.uint8).reshape(self.n, 3).copy()

    def coords(self):
        """x, y, z of every voxel in index order: index = (z ry + y) rx + x"""
        rx, ry, _ = self.res
        i = np.arange(self.n, dtype=np.int64)
        return i % rx, (i // rx) % ry, i // (rx * ry)

    def copy(self):
        v = Volume(self.vs, self.tau, self.res, self.origin, self.max_weight)
        v.load(self.tsdf, self.weight, self.rgb)
        return v


class Intrinsics:
    def __init__(self, fx, fy, cx, cy, width, height):
        self.fx, self.fy, self.cx, self.cy = F(fx), F(fy), F(cx), F(cy)
        self.width, self.height = int(width), int(height)


def world_to_camera(pose):
    """the 12 floats the library multiplies by, from a camera-to-world 4 x 4: inverted in float64, rounded to f32 (the facade's rule)"""
    return np.ascontiguousarray(np.linalg.inv(np.asarray(pose, np.float64))[:3, :4].astype(F).reshape(12))


def integrate(vol, depth, intr, w2c, rgb=None, mutant=None, shader_conversion=False):
    """steps 1-12 of the header; updates vol in place and returns a dict: n_updated, the voxels each skip rule took (a voxel is counted
    at the first rule that skips it; the depth rules by the kind of pixel: zero, negative, NaN, infinite) and `half`, the updated voxels
    whose pixel differs from truncation without the + 0.5.
    shader_conversion: not the contract but the reference's shader on an implementation whose u32() clamps and saturates -- c_z is not
    tested, and a voxel whose a or b is negative or NaN is fused with pixel column or row 0 instead of being skipped (the first two
    deviations of the header's list; a + inf saturates and falls outside the image as before).  It exists to reproduce the figures that
    show why the reference passes its own mean-z bound."""
    m = np.asarray(w2c, F).reshape(12)
    W, H = intr.width, intr.height
    depth = np.asarray(depth, F).reshape(H * W)
    x, y, z = vol.coords()
    with np.errstate(all="ignore"):
        wx, wy, wz = x.astype(F) * vol.vs + vol.origin[0], y.astype(F) * vol.vs + vol.origin[1], z.astype(F) * vol.vs + vol.origin[2]
        cx = ((m[0] * wx + m[1] * wy) + m[2] * wz) + m[3]
        cy = ((m[4] * wx + m[5] * wy) + m[6] * wz) + m[7]
        cz = ((m[8] * wx + m[9] * wy) + m[10] * wz) + m[11]
        front = np.ones(vol.n, bool) if shader_conversion else cz > 0
        half = F(0.0) if mutant == "no_half" else F(0.5)
        a = ((cx / cz) * intr.fx + intr.cx) + half
        b = ((cy / cz) * intr.fy + intr.cy) + half
        before = front & ~((a >= 0) & (b >= 0))                     # left of or above the image, or NaN
        if shader_conversion:
            a, b = np.where(a >= 0, a, F(0.0)), np.where(b >= 0, b, F(0.0))
        inside = front & (a >= 0) & (a < F(W)) & (b >= 0) & (b < F(H))
        beyond = front & ~before & ~inside
        u = np.where(inside, a, 0).astype(np.int64)
        v = np.where(inside, b, 0).astype(np.int64)
        pix = (u * H + v) % (W * H) if mutant == "uv_exchanged" else v * W + u
        d = depth[pix]
        zero_depth, negative_depth = inside & (d == 0), inside & (d < 0)
        nan_depth, inf_depth = inside & np.isnan(d), inside & (d == np.inf)
        upd = inside & (d > 0) & np.isfinite(d)
        t = np.fmin(np.fmax(d - cz, -vol.tau), vol.tau)
        w0 = vol.weight.astype(U32)
        w1 = np.minimum(w0 + U32(1), U32(vol.max_weight))
        alpha = F(1.0) / (np.maximum(w0, U32(1)) if mutant == "alpha_from_old_weight" else w1).astype(F)
        keep = F(1.0) - alpha
        tsdf = keep * vol.tsdf + alpha * t
        vol.tsdf = np.where(upd, tsdf, vol.tsdf).astype(F)
        vol.weight = np.where(upd, w1, w0).astype(np.uint8)
        if rgb is not None:
            p = np.asarray(rgb, np.uint8).reshape(H * W, 3)[pix]
            col = upd & p.any(axis=1)
            c = np.fmin(np.fmax(keep[:, None] * vol.rgb.astype(F) + alpha[:, None] * p.astype(F), F(0.0)), F(255.0)).astype(np.uint8)
            vol.rgb = np.where(col[:, None], c, vol.rgb)
        changed = upd & (np.floor(a) != np.floor(a - F(0.5)))
    return {"n_updated": int(upd.sum()), "behind": int((~front).sum()), "before_image": int(before.sum()), "beyond_image": int(beyond.sum()),
            "zero_depth": int(zero_depth.sum()), "negative_depth": int(negative_depth.sum()), "nan_depth": int(nan_depth.sum()),
            "inf_depth": int(inf_depth.sum()), "half": int(changed.sum())}


def extract(vol, iso_value=0.0, flags=0, mutant=None):
    """-> xyz (n, 3) f32, rgb (n, 3) u8 in the contract's order, and the points of every cube (cubes in ascending order of their base voxel)"""
    rx, ry, rz = vol.res
    iso = F(iso_value)
    x, y, z = vol.coords()
    cube = (x < rx - 1) & (y < ry - 1) & (z < rz - 1)
    base = np.nonzero(cube)[0]
    x, y, z = x[base], y[base], z[base]
    nc = len(base)
    if nc == 0:
        return np.zeros((0, 3), F), np.zeros((0, 3), np.uint8), np.zeros(0, np.int64)
    val, seen, pos = [], [], []
    unseen = vol.tau - iso if mutant == "tau_minus_iso" else vol.tau
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        i = base + dx + dy * rx + dz * rx * ry
        s = vol.weight[i] > 0
        seen.append(s)
        val.append(np.where(s, vol.tsdf[i] - iso, unseen).astype(F))
        pos.append(np.stack([vol.origin[0] + (x + dx).astype(F) * vol.vs, vol.origin[1] + (y + dy).astype(F) * vol.vs,
                             vol.origin[2] + (z + dz).astype(F) * vol.vs], 1).astype(F))
    edges = EDGES[:4] + EDGES[8:] + EDGES[4:8] if mutant == "yz_edges_exchanged" else EDGES
    emit, pts = np.zeros((nc, 12), bool), np.zeros((nc, 12, 3), F)
    with np.errstate(all="ignore"):
        for e, (a, b, _) in enumerate(edges):
            va, vb, pa, pb = val[a], val[b], pos[a], pos[b]
            prod = va * vb
            hit = (prod < 0) if mutant == "lt_for_le" else (prod <= 0)
            if flags & OBSERVED_EDGES:
                hit = hit & seen[a] & seen[b]
            emit[:, e] = hit & seen[0]
            near = np.abs(va - vb) < F(0.00001)
            s = np.fmin(np.fmax(va / (va - vb), F(0.0)), F(1.0))
            pts[:, e] = np.where(near[:, None], F(0.5) * (pa + pb), pa + s[:, None] * (pb - pa))
    colour_at = base + (1 + rx + rx * ry if mutant == "colour_from_far_corner" else 0)
    colours = np.broadcast_to(vol.rgb[colour_at][:, None, :], (nc, 12, 3))
    return pts[emit], np.ascontiguousarray(colours[emit]), emit.sum(1)


# ---- the inputs the CPU and the GPU tests share ---------------------------------------------------------------------------------------
# the reference's own test scene (threecrate-gpu/src/tsdf.rs:890-1144)
SCENE = dict(voxel_size=0.02, truncation_distance=0.1, resolution=(32, 32, 32), origin=(-0.32, -0.32, 0.0))
SCENE_CAMERA = (525.0, 525.0, 319.5, 239.5, 640, 480)
IDENTITY_POSE = np.eye(4)


def scene_volume(max_weight=100):
    return Volume(max_weight=max_weight, **SCENE)


def constant_depth(intr, d):
    return np.full((intr.height, intr.width), d, F)


def rotation(axis, angle):
    """Rodrigues, float64"""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(R=None, t=(0, 0, 0)):
    p = np.eye(4)
    if R is not None:
        p[:3, :3] = R
    p[:3, 3] = t
    return p


POSES = {
    "identity": pose(),
    "skew": pose(rotation((1.0, 2.0, 0.5), 0.21), (0.03, -0.02, -0.05)),
    "inside": pose(rotation((0.0, 1.0, 0.2), 0.4), (0.01, 0.0, 0.06)),            # the camera centre is inside the volume: voxels behind it
    "away": pose(rotation((0.0, 1.0, 0.0), np.pi), (0.0, 0.0, -0.1)),             # looks along -z from in front of the volume: nothing in view
    "corner": pose(rotation((0.0, 0.0, 1.0), 0.1), (0.5, 0.4, 0.0)),              # beside the volume: sees its far (+x, +y) corner only
}


def small_camera(width, height):
    """a 60-degree-ish pinhole for a width x height image"""
    f = 0.82 * width
    return Intrinsics(f, f, (width - 1) / 2.0, (height - 1) / 2.0, width, height)


def ramp_depth(intr, flaws=True):
    """a depth ramp with a band of zeros, and -- flaws -- one NaN, one +inf and one negative pixel near the centre"""
    v, u = np.mgrid[0:intr.height, 0:intr.width]
    d = (F(0.12) + F(0.004) * u.astype(F) + F(0.003) * v.astype(F)).astype(F)
    d[:, intr.width // 5] = 0.0
    if flaws:
        cy, cx = intr.height // 2, intr.width // 2
        d[cy, cx] = np.nan
        d[cy - 1, cx + 1] = np.inf
        d[cy + 1, cx - 1] = -0.25
    return d


def colour_image(intr, k=0):
    """every channel varies; a patch of (0, 0, 0) pixels, which must leave a voxel's colour alone"""
    v, u = np.mgrid[0:intr.height, 0:intr.width]
    c = np.stack([(37 * u + 11 * v + 50 * k) % 256, (5 * u + 91 * v + 20 * k) % 256, (u * v + 7 * k) % 256], 2).astype(np.uint8)
    c[: intr.height // 2, : intr.width // 3] = 0
    return c


def shaped_volume(resolution, max_weight=100):
    """a volume of 0.02 m voxels centred on the optical axis, its near face 0.1 m in front of the identity camera"""
    rx, ry, _ = resolution
    return Volume(0.02, 0.06, resolution, (-0.01 * rx, -0.01 * ry, 0.1), max_weight)


# (rx, ry, rz): rx either side of a run of 64 voxels, one and two runs per row, a row far wider than the image; ry, rz in 1..5
RESOLUTIONS = [(1, 1, 1), (1, 3, 2), (2, 2, 2), (63, 2, 3), (64, 3, 2), (65, 4, 5), (257, 5, 3), (32, 32, 32)]
IMAGES = {(1, 1, 1): (8, 6), (1, 3, 2): (8, 6), (2, 2, 2): (8, 6), (63, 2, 3): (16, 12), (64, 3, 2): (24, 18), (65, 4, 5): (32, 24),
          (257, 5, 3): (64, 48), (32, 32, 32): (16, 12)}


def integration_cases():
    """name -> (volume, [(depth, rgb or None, intrinsics, world_to_camera)])"""
    cases = {}
    for res in RESOLUTIONS:
        intr = small_camera(*IMAGES[res])
        cases["x".join(map(str, res)) + " identity"] = (shaped_volume(res), [(ramp_depth(intr), None, intr, world_to_camera(POSES["identity"]))])
    intr = small_camera(16, 12)
    for name in ("skew", "inside", "away", "corner"):
        cases["32x32x32 " + name] = (shaped_volume((32, 32, 32)), [(ramp_depth(intr), None, intr, world_to_camera(POSES[name]))])
    intr = small_camera(32, 24)
    frames = [(ramp_depth(intr, flaws=(k == 1)) + F(0.01 * k), colour_image(intr, k), intr, world_to_camera(POSES[p]))
              for k, p in enumerate(("identity", "skew", "inside"))]
    for mw in (1, 3, 255):
        cases[f"65x4x5 three frames max_weight {mw}"] = (shaped_volume((65, 4, 5), mw), frames)
    cases["32x32x32 three frames"] = (shaped_volume((32, 32, 32)), frames)
    return cases


def extraction_state(resolution, max_weight=100):
    """A state for upload: a tilted plane's clamped signed distance, with what extraction can get wrong planted in it -- voxels whose
    tsdf is exactly 0 or exactly +-0.03 (the iso values of the tests), a slab of unobserved voxels beside observed negative ones,
    two neighbours less than 1e-5 apart across zero, a pair whose product underflows, every channel of the colour varying."""
    vol = shaped_volume(resolution, max_weight)
    x, y, z = vol.coords()
    i = np.arange(vol.n)
    d = (F(0.013) * (x % 7).astype(F) - F(0.02) * (y % 3).astype(F) + F(0.017) * (z % 4).astype(F) - F(0.031) * ((x // 7) % 2).astype(F)).astype(F)
    tsdf = np.fmin(np.fmax(d, -vol.tau), vol.tau).astype(F)
    tsdf[i % 11 == 3] = 0.0
    tsdf[i % 13 == 5] = 0.03
    tsdf[i % 17 == 7] = -0.03
    tsdf[i % 19 == 2] = 3e-6
    tsdf[i % 19 == 3] = -3e-6
    tsdf[i % 23 == 4] = 1e-30
    tsdf[i % 23 == 5] = -1e-30
    weight = (1 + (i * 7) % max_weight).astype(np.uint8)
    weight[(x % 5 == 4) | (i % 29 == 0)] = 0
    rgb = np.stack([(i * 3) % 256, (i * 5 + 1) % 256, (i * 7 + 2) % 256], 1).astype(np.uint8)
    vol.load(tsdf, weight, rgb)
    return vol


# more than 2 049 cube blocks (a block is 4 runs of up to 64 cubes along x: tc_internal.h kTsdfBlock / kTsdfRun) need 8 197 runs.  A run
# costs least with one cube in it (rx = 2), and 2 ry rz is smallest over (ry - 1)(rz - 1) >= 8 197 at 83 x 101: 82 x 100 = 8 200 runs =
# 2 050 blocks in 16 766 voxels (tests/test_tsdf_cpu.py searches the alternatives)
CUBE_BLOCK_RUNS = 4
MANY_BLOCKS = (2, 83, 101)
