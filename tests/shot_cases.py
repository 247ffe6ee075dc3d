"""Named small cases of the SHOT / USC descriptors for tests/test_shot_cpu.py (which proves on the checker alone that each reaches what it
is meant to and that at least 98 % of its compared rows are clean) and tests/test_gpu_shot.py (which holds the device to
tests/shot_checker.py on each of them).  A case is a dict: np6 (n, 6) float32 (position, normal), radius, k, rows (the compared rows, None =
all); expected(name, variant) is the checker's result, computed once.  K_WAVE, K_STAGE and K_KNN_ENTRIES are the kernel's constants, read
from csrc/shot.hip."""
import functools
import os
import re

import numpy as np

from tests import shot_checker as SC

_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "threecrate_amd", "csrc", "shot.hip")).read()
K_WAVE = int(re.search(r"constexpr uint32_t kShotWave = (\d+);", _SRC).group(1))
K_STAGE = int(re.search(r"constexpr uint32_t kShotStage = (\d+);", _SRC).group(1))
K_KNN_ENTRIES = 1 << int(re.search(r"constexpr size_t kShotKnnEntries = size_t\(1\) << (\d+);", _SRC).group(1))
K_MAX = 2048                                                    # kMaxK (tc_internal.h): k + 1 may reach it
VARIANTS = ("shot", "usc")
MIN_CLEAN = 0.98


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def bumpy(n, seed, noise=0.05, side=2.0):
    """n points of the surface z = 0.1 sin(3x) cos(2y) over a square of the given side, with its normals plus `noise` of isotropic error"""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, side, n), rng.uniform(0, side, n)
    z = 0.1 * np.sin(3 * x) * np.cos(2 * y)
    nrm = _unit(np.stack([-0.3 * np.cos(3 * x) * np.cos(2 * y), 0.2 * np.sin(3 * x) * np.sin(2 * y), np.ones(n)], 1))
    nrm = _unit(nrm + noise * rng.normal(size=(n, 3)))
    return np.concatenate([np.stack([x, y, z], 1), nrm], 1).astype(np.float32)


def volume(n, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.uniform(0, 1, (n, 3)), _unit(_unit(rng.normal(size=(n, 3))) + noise * rng.normal(size=(n, 3)))], 1).astype(np.float32)


def _ball(rng, m, radius):
    u = _unit(rng.normal(size=(m, 3))) * rng.uniform(0, 1, (m, 1)) ** (1 / 3)
    return u * radius


def _list_lengths():
    """clusters of m + 1 points inside a ball of diameter 0.8 r, 10 r apart: every point's ball is the other m points of its cluster"""
    rng = np.random.default_rng(1)
    r = 0.1
    ms = [K_WAVE - 1, K_WAVE, K_WAVE + 1, 2 * K_WAVE + 1, K_STAGE - 1, K_STAGE, K_STAGE + 1]
    pos = np.concatenate([_ball(rng, m + 1, 0.4 * r) + np.array([c, 0.3 * (c % 3), 0.0]) for c, m in enumerate(ms)])
    np6 = np.concatenate([pos, _unit(rng.normal(size=(len(pos), 3)))], 1).astype(np.float32)
    return dict(np6=np6, radius=r, k=10, rows=None, lengths=ms)


BLOCK_SEEDS = {64: 6}                                               # per n: the first seed (from 1) at which 98 % of the rows are clean, both variants


def _blocks(n, seed=None):
    """half dense (ball road), half sparse (fallback road); from 63 points on rows that are not finite at 0, n // 2, n - 1 and a zero and a
    NaN normal in either half"""
    rng = np.random.default_rng(BLOCK_SEEDS.get(n, 1) if seed is None else seed)
    r = 0.1
    dense = n - n // 2
    pos = np.concatenate([_ball(rng, dense, 0.45 * r), np.array([3.0, 0.0, 0.0]) + rng.uniform(0, 1, (n // 2, 3)) * r * (0.6 * max(n // 2, 4)) ** (1 / 3)])      # ~7 to a ball
    np6 = np.concatenate([pos, _unit(rng.normal(size=(n, 3)))], 1).astype(np.float32)
    if n >= 63:
        np6[0, 0], np6[n // 2, 1], np6[n - 1, 2] = np.nan, np.inf, -np.inf
        np6[1, 3:], np6[2, 3:] = 0.0, np.nan
        np6[n - 2, 3:], np6[n - 3, 3:] = 0.0, np.nan
    return dict(np6=np6, radius=r, k=10, rows=None)


def _fallback(k):
    """600 points of a cube whose balls hold fewer than 0.8 k points: every list is launch_knn's, a fifth of it or more beyond the radius"""
    return dict(np6=volume(600, 5), radius=0.15, k=k, rows=None)


EDGE_R = 0.25
EDGE_OFFSETS = ((EDGE_R, 0.0, 0.0), (0.0, EDGE_R / 2, 0.0), (-EDGE_R / 4, 0.0, 0.0), (0.0, -3 * EDGE_R / 4, 0.0))


def snapped(seed=1, n=3000):
    np6 = bumpy(n, seed)
    np6[:, :3] = np.round(np6[:, :3] * 1024.0) / 1024.0
    return np6


def _exact_edges():
    """the snapped cloud with partners planted at exactly (r, 0, 0), (0, r / 2, 0), (-r / 4, 0, 0), (0, -3 r / 4, 0) from 12 queries"""
    base = snapped()
    rng = np.random.default_rng(3)
    queries = rng.choice(len(base), 12, replace=False)
    extra = []
    for q in queries:
        for o in EDGE_OFFSETS:
            p = base[q].copy()
            p[:3] += np.array(o, np.float32)
            extra.append(p)
    np6 = np.concatenate([base, np.array(extra, np.float32)])
    rows = np.concatenate([queries, np.arange(len(base), len(np6)), rng.choice(len(base), 150, replace=False)])
    return dict(np6=np6, radius=EDGE_R, k=10, rows=np.unique(rows), queries=queries, n_base=len(base))


def _degenerate(kind):
    rng = np.random.default_rng(9)
    if kind == "identical":
        pos, nrm = np.tile([[0.5, 0.25, 0.125]], (500, 1)), _unit(rng.normal(size=(500, 3)))
    elif kind == "line":
        pos, nrm = np.stack([np.arange(400) / 256.0, np.zeros(400), np.zeros(400)], 1), np.tile([[0.0, 0.0, 1.0]], (400, 1))
    else:
        g = np.arange(20) / 16.0
        pos = np.stack([np.repeat(g, 20), np.tile(g, 20), np.zeros(400)], 1)
        nrm = np.tile([[0.0, 0.0, 1.0]], (400, 1))
    return dict(np6=np.concatenate([pos, nrm], 1).astype(np.float32), radius=0.2, k=10, rows=None, degenerate=True)


def chunk_lists(k):
    return K_KNN_ENTRIES // (k + 1)


def _chunked():
    """k + 1 = kMaxK and every ball below k: every point falls back, and n is the smallest that reaches a second chunk of lists, plus 16"""
    k = K_MAX - 1
    n = chunk_lists(k) + 16
    rng = np.random.default_rng(4)
    rows = np.sort(np.concatenate([rng.choice(chunk_lists(k), 284, replace=False), np.arange(chunk_lists(k), n)]))     # 300 rows, all of the second chunk's
    return dict(np6=volume(n, 6), radius=0.05, k=k, rows=rows)


CASES = {
    "bumpy": lambda: dict(np6=bumpy(3000, 1), radius=0.12, k=10, rows=None),
    "bumpy_mixed": lambda: dict(np6=bumpy(3000, 1), radius=0.06, k=10, rows=None),
    "volume": lambda: dict(np6=volume(3000, 1), radius=0.22, k=10, rows=np.arange(0, 3000, 3)),
    "list_lengths": _list_lengths,
    **{f"blocks_{n}": functools.partial(_blocks, n) for n in (1, 2, 63, 64, 65, 255, 256, 257)},
    **{f"fallback_k{k1 - 1}": functools.partial(_fallback, k1 - 1) for k1 in (34, 65, 66, 129, 130, 257)},
    "exact_edges": _exact_edges,
    **{f"degenerate_{kind}": functools.partial(_degenerate, kind) for kind in ("identical", "line", "plane")},
    "chunked": _chunked,
}
BOTH_ROADS = ("bumpy_mixed", "blocks_257", "fallback_k33", "exact_edges")    # the cases that also run through the _device entry point
SHIFTS = (2.0 ** 10, 2.0 ** 13)


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["np6"] = np.ascontiguousarray(c["np6"], np.float32)
    c["np6"].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name, variant, arith="f64"):
    c = case(name)
    return SC.describe(c["np6"], c["radius"], c["k"], variant, arith, c["rows"])


def shifted(shift):
    np6 = np.array(snapped())
    np6[:, :3] += np.float32(shift)
    return np6
