"""Synthetic workloads of SURVEY.md section 8(d) (counter-based SplitMix64, identical for the
CPU oracle and the HIP path).  Pure numpy; no device code.

The transforms mirror the reference bench driver: target = T * source with
T = (0.05, -0.02, 0.01) + 0.02 rad yaw (examples/threecrate_dataset_bench.rs:281-287).
"""
import numpy as np

_GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def splitmix_u01(seed, counters):
    """f32 in [0,1): z = seed + GOLDEN*(i+1); SplitMix64 finaliser; (z >> 40) * 2^-24."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + _GOLDEN * (counters.astype(np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def uniform_cloud(n, seed=1, scale=(1.0, 1.0, 1.0)):
    """N points uniform in [0,sx) x [0,sy) x [0,sz); coordinate c of point i uses counter 3i+c."""
    c = np.arange(3 * n, dtype=np.uint64)
    u = splitmix_u01(seed, c).reshape(n, 3)
    return (u * np.asarray(scale, dtype=np.float32)).astype(np.float32)


def sphere_cloud(n, radius=1.0, seed=1):
    """n points on a sphere, uniform in area, in random order: (n, 3) float32"""
    u = splitmix_u01(seed, np.arange(2 * n, dtype=np.uint64)).reshape(n, 2)
    z, phi = 2.0 * u[:, 0] - 1.0, 2.0 * np.pi * u[:, 1]
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    return (radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)).astype(np.float32)


def grid_mesh(nx, ny, noise=0.0, seed=1):
    """A height field over an nx x ny lattice of unit spacing, triangulated row-major: vertex (ix, iy) has index iy * nx + ix and
    z = noise * (u - 0.5), u from counter iy * nx + ix; cell (ix, iy) gives the faces (v, v + 1, v + nx) and (v + 1, v + nx + 1, v + nx).
    -> vertices (nx * ny, 3) float32, faces (2 (nx - 1) (ny - 1), 3) uint32 (none when nx or ny is below 2)."""
    iy, ix = np.divmod(np.arange(nx * ny, dtype=np.uint64), np.uint64(max(nx, 1)))
    z = (splitmix_u01(seed, np.arange(nx * ny, dtype=np.uint64)) - np.float32(0.5)) * np.float32(noise)
    vertices = np.stack([ix.astype(np.float32), iy.astype(np.float32), z.astype(np.float32)], axis=1)
    if nx < 2 or ny < 2:
        return vertices, np.zeros((0, 3), np.uint32)
    cy, cx = np.divmod(np.arange((nx - 1) * (ny - 1), dtype=np.int64), nx - 1)
    v = cy * nx + cx
    faces = np.stack([np.stack([v, v + 1, v + nx], axis=1), np.stack([v + 1, v + nx + 1, v + nx], axis=1)], axis=1).reshape(-1, 3)
    return vertices, faces.astype(np.uint32)


def box_mesh(k, size=(1.0, 1.0, 1.0), open_side=False):
    """A closed axis-aligned box [0, size] with k subdivisions per edge, its sides welded along the box's edges (a lattice point has ONE
    vertex, numbered where the sides -x, +x, -y, +y, -z, +z first reach it), triangulated outward: every face normal is exactly +-axis
    and the dihedral dot across a box edge is exactly 0.  open_side leaves the +z side out: its rim becomes a boundary.
    -> vertices (6 k^2 + 2, 3) float32 when closed, faces (12 k^2 | 10 k^2, 3) uint32, normals: per vertex the exact +-axis normal of
    the first side that reaches it."""
    k = int(k)
    iv, iu = (a.reshape(-1) for a in np.meshgrid(np.arange(k + 1), np.arange(k + 1), indexing="ij"))   # lattice point (iu, iv): iv * (k + 1) + iu
    cv, cu = np.divmod(np.arange(k * k, dtype=np.int64), max(k, 1))
    c = cv * (k + 1) + cu
    quad = np.stack([np.stack([c, c + 1, c + k + 1], axis=1), np.stack([c + 1, c + k + 2, c + k + 1], axis=1)], axis=1).reshape(-1, 3)
    ids, fs, ns = [], [], []
    # (axis of the normal, sign): u and v run over the two other axes in cyclic order, so u x v = +axis
    for axis, sign in ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))[:5 if open_side else 6]:
        p = np.zeros((len(iu), 3), np.int64)
        p[:, (axis + 1) % 3], p[:, (axis + 2) % 3], p[:, axis] = iu, iv, (k if sign > 0 else 0)
        nrm = np.zeros((len(iu), 3), np.float32)
        nrm[:, axis] = sign
        fs.append((quad if sign > 0 else quad[:, ::-1]) + len(ids) * len(iu))
        ids.append((p[:, 2] * (k + 1) + p[:, 1]) * (k + 1) + p[:, 0])
        ns.append(nrm)
    ids, ns = np.concatenate(ids), np.concatenate(ns)
    uniq, first, inverse = np.unique(ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                    # welded vertices in order of first appearance
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    lattice = ids[first[order]]
    xyz = np.stack([lattice % (k + 1), lattice // (k + 1) % (k + 1), lattice // ((k + 1) * (k + 1))], axis=1).astype(np.float32)
    vertices = xyz / np.float32(max(k, 1)) * np.asarray(size, np.float32)
    return vertices.astype(np.float32), rank[inverse.reshape(-1)][np.concatenate(fs)].astype(np.uint32), ns[first[order]]


def icosphere(level, radius=1.0):
    """A closed unit icosahedron subdivided `level` times (every triangle into four, the new vertices pushed onto the sphere in f64 and
    rounded to f32 once), faces outward.  Level L has 10 * 4^L + 2 vertices and 20 * 4^L faces.  The midpoint of an edge is created once,
    in order of first use (face order, sides (a,b), (b,c), (c,a)), so the numbering is fixed.
    -> vertices (n, 3) float32, faces (m, 3) uint32."""
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.sqrt(1.0 + t * t) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(int(level)):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.sqrt((p * p).sum()))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return (np.asarray(v, np.float64) * float(radius)).astype(np.float32), np.asarray(f, np.uint32)


def bumpy_grid_mesh(nx, ny, amplitude=0.25, waves=3.0, spacing=None):
    """A smooth bumpy height field over an nx x ny lattice, triangulated as grid_mesh: x, y in [0, 1] (or `spacing` apart),
    z = amplitude * sin(2 pi waves x) * cos(2 pi waves y) + amplitude / 2 * sin(2 pi (x + 2 y)), computed in f64 and rounded to f32 once.
    Curved everywhere but on a set of measure zero: the quadric of an interior vertex is well conditioned.
    -> vertices (nx * ny, 3) float32, faces (2 (nx - 1) (ny - 1), 3) uint32."""
    _, faces = grid_mesh(nx, ny)
    iy, ix = np.divmod(np.arange(nx * ny), max(nx, 1))
    x = ix / float(max(nx - 1, 1)) if spacing is None else ix * float(spacing)
    y = iy / float(max(ny - 1, 1)) if spacing is None else iy * float(spacing)
    u, w = (x, y) if spacing is None else (x / (float(spacing) * max(nx - 1, 1)), y / (float(spacing) * max(ny - 1, 1)))
    z = amplitude * np.sin(2 * np.pi * waves * u) * np.cos(2 * np.pi * waves * w) + 0.5 * amplitude * np.sin(2 * np.pi * (u + 2 * w))
    return np.stack([x, y, z], axis=1).astype(np.float32), faces


def _volume_frame(center, resolution, size):
    """the frame of the reference's test volumes: the origin is the centre minus half the size, the voxel is size / (res - 1), in f32"""
    f = np.float32
    res = [int(r) for r in resolution]
    origin = [f(c) - f(s) / f(2.0) for c, s in zip(center, size)]
    voxel = [f(s) / f(r - 1) for s, r in zip(size, res)]
    axes = [o + np.arange(r, dtype=f) * v for o, r, v in zip(origin, res, voxel)]
    return res, [float(v) for v in voxel], [float(o) for o in origin], np.meshgrid(*axes, indexing="ij")


def sphere_volume(center=(0.0, 0.0, 0.0), radius=1.0, resolution=(33, 33, 33), size=(3.0, 3.0, 3.0)):
    """the signed distance to a sphere on a grid, f32 -> (values (nx, ny, nz), voxel_size, origin): |p - centre| - radius"""
    f = np.float32
    res, voxel, origin, (x, y, z) = _volume_frame(center, resolution, size)
    dx, dy, dz = x - f(center[0]), y - f(center[1]), z - f(center[2])
    return (np.sqrt(dx * dx + dy * dy + dz * dz) - f(radius)).astype(f), voxel, origin


def box_volume(center=(0.0, 0.0, 0.0), half_size=1.0, resolution=(33, 33, 33), size=(3.0, 3.0, 3.0)):
    """the signed distance to an axis-aligned cube of half edge half_size, f32 -> (values (nx, ny, nz), voxel_size, origin):
    |max(d, 0)| + min(max(dx, dy, dz), 0) with d = |p - centre| - half_size per axis"""
    f = np.float32
    res, voxel, origin, (x, y, z) = _volume_frame(center, resolution, size)
    dx, dy, dz = np.abs(x - f(center[0])) - f(half_size), np.abs(y - f(center[1])) - f(half_size), np.abs(z - f(center[2])) - f(half_size)
    mx, my, mz = np.maximum(dx, f(0)), np.maximum(dy, f(0)), np.maximum(dz, f(0))
    outside = np.sqrt(mx * mx + my * my + mz * mz)
    return (outside + np.minimum(np.maximum(np.maximum(dx, dy), dz), f(0))).astype(f), voxel, origin


def yaw_isometry(t, yaw):
    """7-float isometry (qx qy qz qw tx ty tz): rotation about z by `yaw`, translation t."""
    h = np.float32(yaw) / np.float32(2.0)
    return np.array([0.0, 0.0, np.sin(h), np.cos(h), t[0], t[1], t[2]], dtype=np.float32)


def isometry_matrix(T):
    """4x4 float64 homogeneous matrix of a 7-float isometry."""
    x, y, z, w = [float(v) for v in T[:4]]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = [float(v) for v in T[4:7]]
    return M


def apply_isometry(T, pts):
    """float64 application, rounded to f32 once (generates inputs, not a parity-critical op)."""
    M = isometry_matrix(T)
    return (pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def invert_isometry(T):
    M = np.linalg.inv(isometry_matrix(T))
    return M


def harness_transform():
    """examples/threecrate_dataset_bench.rs:281-287"""
    return yaw_isometry((0.05, -0.02, 0.01), 0.02)


def small_transform(n):
    """T_small of SURVEY 8(d): t = s*(0.3,-0.2,0.1), yaw 0.1*s rad, s = n^(-1/3)."""
    s = float(n) ** (-1.0 / 3.0)
    return yaw_isometry((0.3 * s, -0.2 * s, 0.1 * s), 0.1 * s)


def gaussian_noise(n, seed, sigma):
    """(n, 3) f32 normal deviates, counter based like the clouds (Box-Muller over splitmix_u01): same bits everywhere."""
    c = np.arange(6 * n, dtype=np.uint64)
    u = splitmix_u01(seed, c).astype(np.float64).reshape(n, 3, 2)
    r = np.sqrt(-2.0 * np.log(np.maximum(u[..., 0], 2.0 ** -25)))
    return (sigma * r * np.cos(2.0 * np.pi * u[..., 1])).astype(np.float32)


def registration_pair(n, seed=1, transform=None, scale=(1.0, 1.0, 1.0), noise_sigma=0.0):
    """target = cloud(seed); source = T^-1 * cloud, so that ICP(source -> target) recovers T.
    noise_sigma > 0: INDEPENDENT sensor noise on both clouds (two scans of one scene never hold the same points): the
    converged phase of a registration then has non-zero nearest-neighbour distances, like real scan pairs."""
    tgt = uniform_cloud(n, seed, scale)
    T = small_transform(n) if transform is None else transform
    Minv = invert_isometry(T)
    src = (tgt.astype(np.float64) @ Minv[:3, :3].T + Minv[:3, 3]).astype(np.float32)
    if noise_sigma > 0.0:
        src = (src + gaussian_noise(n, 1000003 + 2 * seed, noise_sigma)).astype(np.float32)
        tgt = (tgt + gaussian_noise(n, 1000004 + 2 * seed, noise_sigma)).astype(np.float32)
    return src, tgt, T


# ---- scan-shaped synthetic clouds (BASELINE configs [2] and [4]) ----------
def plane_clutter_cloud(n, seed=1, inlier_fraction=0.6, sigma=0.004):
    """A plane with clutter for plane segmentation: points uniform in the box [-1, 1)^3, of which `inlier_fraction` are moved onto the
    plane 0.3 x - 0.2 y + z = 0.5 with Gaussian noise `sigma` along z.  Same counter-based generators as the other workloads."""
    p = uniform_cloud(n, seed, (2.0, 2.0, 2.0)) - np.float32(1.0)
    on = splitmix_u01(seed + 7, np.arange(n, dtype=np.uint64)) < np.float32(inlier_fraction)
    z = np.float32(0.5) - np.float32(0.3) * p[:, 0] + np.float32(0.2) * p[:, 1] + gaussian_noise(n, seed + 11, sigma)[:, 2]
    p[on, 2] = z[on]
    return np.ascontiguousarray(p, np.float32)


def _smooth_noise(u, v, seed):
    """cheap smooth 2-D field in [-1, 1] (sum of a few seeded sinusoids)."""
    rng = np.random.default_rng(seed)
    out = np.zeros_like(u, dtype=np.float64)
    for _ in range(6):
        fu, fv, ph = rng.uniform(0.5, 4.0), rng.uniform(0.5, 4.0), rng.uniform(0, 2 * np.pi)
        out += np.sin(fu * u + fv * v + ph)
    return out / 6.0


def tum_shaped_cloud(width=1155, height=866, seed=0, step=1):
    """Pinhole back-projection of a synthetic depth map z(u,v) = 1.5 + 0.5*smooth_noise (metres);
    fx = fy = 525*width/640, principal point centred (the reference's TUM loader uses fx=fy=525,
    cx=319.5, cy=239.5: examples/threecrate_dataset_bench.rs:339-357)."""
    us, vs = np.meshgrid(np.arange(0, width, step, dtype=np.float64), np.arange(0, height, step, dtype=np.float64))
    fx = 525.0 * width / 640.0
    cx, cy = (width - 1) / 2.0, (height - 1) / 2.0
    z = 1.5 + 0.5 * _smooth_noise(us / width * 6.0, vs / height * 6.0, seed)
    x = (us - cx) / fx * z
    y = (vs - cy) / fx * z
    return np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)


def kitti_shaped_cloud(beams=64, azimuth_steps=1875, seed=0, noise=0.02):
    """64 beams (elevation -24.8..+2 deg) x azimuth steps ray-cast onto the ground plane z = -1.73 m and
    four walls at +-20 m, range noise sigma = 2 cm."""
    rng = np.random.default_rng(seed)
    el = np.deg2rad(np.linspace(-24.8, 2.0, beams))[:, None]
    az = np.linspace(0, 2 * np.pi, azimuth_steps, endpoint=False)[None, :]
    d = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el) * np.ones_like(az)], axis=-1).reshape(-1, 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ground = np.where(d[:, 2] < -1e-6, -1.73 / d[:, 2], np.inf)
        t_wx = np.where(np.abs(d[:, 0]) > 1e-9, 20.0 / np.abs(d[:, 0]), np.inf)
        t_wy = np.where(np.abs(d[:, 1]) > 1e-9, 20.0 / np.abs(d[:, 1]), np.inf)
    t = np.minimum(np.minimum(t_ground, t_wx), t_wy)
    t = t + rng.normal(0.0, noise, t.shape)
    return (d * t[:, None]).astype(np.float32)


def ground_scene(n_ground=8000, obstacles=True, sensor_height=1.8, seed=42):
    """The scene of the reference's ground segmentation tests: n_ground draws on a 60 x 60 m plane at z = -sensor_height with +-2 cm of
    uniform noise, those within 0.5 m of the sensor dropped; with obstacles a wall of 1500 points at x = 8 +- 0.4, |y| < 3, 0.5 to 3 m above
    the ground, and a pole of 400 points at (-5, -5) +- 0.1, 0 to 4 m above it.  (n, 3) float32, ground first."""
    rng = np.random.default_rng(seed)
    zg = -float(sensor_height)
    g = np.stack([rng.uniform(-30.0, 30.0, n_ground), rng.uniform(-30.0, 30.0, n_ground), zg + rng.uniform(-0.02, 0.02, n_ground)], axis=1)
    parts = [g[g[:, 0] ** 2 + g[:, 1] ** 2 >= 0.25]]
    if obstacles:
        parts.append(np.stack([8.0 + rng.uniform(-0.4, 0.4, 1500), rng.uniform(-3.0, 3.0, 1500), zg + rng.uniform(0.5, 3.0, 1500)], axis=1))
        parts.append(np.stack([-5.0 + rng.uniform(-0.1, 0.1, 400), -5.0 + rng.uniform(-0.1, 0.1, 400), zg + rng.uniform(0.0, 4.0, 400)], axis=1))
    return np.concatenate(parts).astype(np.float32)
