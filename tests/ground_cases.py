"""Named small cases of ground segmentation for tests/test_ground_cpu.py (which proves every one clean: margin >= 1e-6, every status and
every branch of the kernel reached) and tests/test_gpu_ground.py (which holds the device to tests/ground_checker.py on each of them).
A case is (points (n, 3) float32, config as ground_checker.default_config() makes it); expected(name) is the checker's result, computed once.
kStage / kWave are the kernel's two size thresholds (csrc/ground.hip: kGroundStage, kGroundWavePatch)."""
import functools

import numpy as np

from threecrate_amd import synth
from tests import ground_checker as GC

K_STAGE, K_WAVE = 4096, 64
H = 1.8                                                         # the sensor height of the built cases


def _quadrants(sectors=16, **over):
    """one zone, one ring: `sectors` patches out to 40 m"""
    return GC.default_config(H, zone_radii=[0.0, 40.0], num_rings=[1], num_sectors=[sectors], max_range=40.0, **over)


def _centre(sector, sectors, r=20.0):
    a = 2.0 * np.pi * (sector + 0.5) / sectors
    return np.array([r * np.cos(a), r * np.sin(a), 0.0])


def _flat(rng, m, centre, half=2.0, z0=-H, noise=0.02):
    """m points of a noisy horizontal square around `centre`"""
    return centre + np.stack([rng.uniform(-half, half, m), rng.uniform(-half, half, m), z0 + rng.uniform(-noise, noise, m)], axis=1)


def _sizes(counts, sectors, seed, **over):
    rng = np.random.default_rng(seed)
    pts = np.concatenate([_flat(rng, m, _centre(s, sectors)) for s, m in enumerate(counts)])
    return pts[rng.permutation(len(pts))].astype(np.float32), _quadrants(sectors, **over)


def _kitti16():
    """kitti_shaped_cloud(beams=16, azimuth_steps=360): its azimuth steps are whole degrees and fall on sector edges (22.5, 11.25 and 6.67 degree
    sectors) to the last bit, for every seed, so the frame is yawed by 0.37 degrees: a sensor that is not mounted square.  Nothing else changes."""
    p = synth.kitti_shaped_cloud(beams=16, azimuth_steps=360, seed=3).astype(np.float64)
    a = np.deg2rad(0.37)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return (p @ rot.T).astype(np.float32), GC.default_config(1.73)


def _statuses():
    """a patch per way of being turned down, 16 sectors"""
    rng = np.random.default_rng(11)
    n_sec, parts = 16, []
    c = lambda s: _centre(s, n_sec)
    parts.append(_flat(rng, 300, c(0)))                                                             # ground, early stop in the first iteration
    two = _flat(rng, 40, c(1))                                                                      # two seeds: two points far below the rest pull
    two[0, 2], two[1, 2] = -H - 6.5, -H - 5.5                                                       # the mean of the lowest 20 under everything else
    parts.append(two)
    parts.append(_flat(rng, 200, c(2), z0=-H + 3.0))                                                # a flat roof 3 m up: ELEVATION
    u = rng.normal(size=(400, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0, 1, (400, 1)) ** (1 / 3)
    parts.append(c(3) + u * np.array([0.11, 0.11, 0.08]) + np.array([0, 0, -H]))                      # a ball: NOT_FLAT
    t = rng.uniform(-3, 3, 500)                                                                     # a vertical wall: NOT_UPRIGHT
    wall_dir, wall_n = np.array([np.cos(0.4), np.sin(0.4), 0.0]), np.array([-np.sin(0.4), np.cos(0.4), 0.0])
    parts.append(c(4) + t[:, None] * wall_dir + rng.uniform(-0.02, 0.02, (500, 1)) * wall_n + np.array([0, 0, 1.0]) * (-H + rng.uniform(0, 3, (500, 1))))
    parts.append(_flat(rng, 9, c(5)))                                                               # below min_points_per_patch
    bowl = _flat(rng, 600, c(6), half=3.0, noise=0.0)                                               # a bowl: the inlier set grows with every plane
    bowl[:, 2] = -H + 0.06 * ((bowl[:, 0] - c(6)[0]) ** 2 + (bowl[:, 1] - c(6)[1]) ** 2) + rng.uniform(-0.01, 0.01, 600)
    parts.append(bowl)
    parts.append(_flat(rng, 15, c(7)))                                                              # num_seed_points larger than the patch
    pts = np.concatenate(parts)
    return pts[rng.permutation(len(pts))].astype(np.float32), _quadrants(n_sec)


def _few_inliers():
    """every point a seed (a threshold of 100 m), a plane that keeps almost nothing (1 mm): 12 points of a ball"""
    rng = np.random.default_rng(5)
    pts = _centre(0, 4) + rng.normal(size=(12, 3)) * 3.0
    more = _flat(rng, 50, _centre(1, 4), noise=0.0002)
    return np.concatenate([pts, more]).astype(np.float32), _quadrants(4, seed_selection_threshold=100.0, dist_threshold=1e-3)


def _bucket_edges():
    """zone_radii[0] > 0, max_range below the last radius, points just inside and just outside every edge (1e-4 relative, by construction),
    theta below 0, the last sector, the origin, and -0.0 in x where 90 degrees is no sector edge"""
    cfg = GC.default_config(H, zone_radii=[2.0, 10.0, 30.0], num_rings=[2, 3], num_sectors=[4, 6], max_range=25.0)
    rng = np.random.default_rng(21)
    pts = [np.array([[0.0, 0.0, -H]])]
    edges = [2.0, 6.0, 10.0, 10.0 + 20.0 / 3.0, 10.0 + 40.0 / 3.0, 25.0, 30.0]
    for ang in (0.3, -0.3, 2.0, -2.0, -0.01):
        for e in edges:
            for f in (1.0 - 1e-4, 1.0 + 1e-4):
                pts.append(np.array([[e * f * np.cos(ang), e * f * np.sin(ang), -H]]))
    pts.append(np.array([[-0.0, 15.0, -H], [5.0, -0.0, -H], [3.0, 0.0, -0.0]]))
    for zone_r, sectors in ((4.0, 4), (8.0, 4), (13.0, 6), (20.0, 6), (24.0, 6)):
        for s in range(sectors):
            pts.append(_flat(rng, 40, _centre(s, sectors, zone_r), half=0.5))
    pts.append(_flat(rng, 60, _centre(2, 6, 27.5), half=0.5))                                       # between max_range and the last radius: out
    pts = np.concatenate(pts)
    return pts[rng.permutation(len(pts))].astype(np.float32), cfg


def _data_edges(with_bad=True):
    """duplicated points, -0.0 coordinates, the origin, and NaN / +-inf in each coordinate among a small scene, default configuration"""
    rng = np.random.default_rng(8)
    scene = synth.ground_scene(3000, True, H, seed=7).astype(np.float64)
    dup = scene[rng.integers(0, len(scene), 60)]
    parts = [scene, dup, dup[:20], np.array([[0.0, 0.0, -H], [5.0, -0.0, -H], [7.0, 1.0, -0.0]])]
    if with_bad:
        bad = []
        for col in range(3):
            for v in (np.nan, np.inf, -np.inf):
                q = np.array([6.0, 2.0, -H])
                q[col] = v
                bad.append(q)
        parts.append(np.array(bad))
    pts = np.concatenate(parts)
    return pts[np.random.default_rng(9).permutation(len(pts))].astype(np.float32), GC.default_config(H)


def _max_patches():
    cfg = GC.default_config(H, zone_radii=[0.0, 45.0], num_rings=[256], num_sectors=[256], max_range=45.0, min_points_per_patch=3)
    rng = np.random.default_rng(31)
    dense = [_flat(rng, 30, np.array([r * np.cos(a), r * np.sin(a), 0.0]), half=0.02) for r, a in ((10.03, 0.5), (30.07, 2.2), (44.0, -1.0))]
    return np.concatenate([synth.ground_scene(3000, False, H, seed=32)] + dense).astype(np.float32), cfg


CASES = {
    "scene": lambda: (synth.ground_scene(8000, True, H, seed=47), GC.default_config(H)),
    "scene_flat": lambda: (synth.ground_scene(8000, False, H, seed=47), GC.default_config(H)),
    "kitti16": _kitti16,
    "sizes_small": lambda: _sizes([9, 10, K_WAVE - 1, K_WAVE, K_WAVE + 1, 255, 256, 257], 8, 2),
    "sizes_stage": lambda: _sizes([K_STAGE - 1, K_STAGE, K_STAGE + 1], 4, 3),
    "one_patch_20000": lambda: (_sizes([20000], 1, 4)[0], GC.default_config(H, zone_radii=[0.0, 40.0], num_rings=[1], num_sectors=[1], max_range=40.0)),
    "statuses": _statuses,
    "few_inliers": _few_inliers,
    "iterations_0": lambda: _sizes([100, 30], 4, 6, num_iterations=0),
    "iterations_1": lambda: _sizes([100, 30], 4, 6, num_iterations=1),
    "bucket_edges": _bucket_edges,
    "data_edges": _data_edges,
    "n1": lambda: (np.array([[5.0, 1.0, -H]], np.float32), GC.default_config(H)),
    "n2": lambda: (np.array([[5.0, 1.0, -H], [5.1, 1.0, -H]], np.float32), GC.default_config(H)),
    "max_patches": _max_patches,
}


@functools.lru_cache(maxsize=None)
def case(name):
    pts, cfg = CASES[name]()
    pts = np.ascontiguousarray(pts, np.float32)
    pts.setflags(write=False)
    return pts, cfg


@functools.lru_cache(maxsize=None)
def expected(name, arith="f64"):
    pts, cfg = case(name)
    return GC.segment(pts, cfg, arith)


def too_many_patches():
    """one patch past the limit"""
    return GC.default_config(H, zone_radii=[0.0, 45.0, 50.0], num_rings=[256, 1], num_sectors=[256, 1], max_range=50.0)
