"""Inputs for tests/test_gpu_registration_variants.py and tests/test_gpu_icp_few_pairs.py, proven usable on the oracle alone (no GPU, no HIP library).

The converged transform of a noise-free isometric copy does not depend on how the pair terms were weighted (every residual
vanishes at the optimum), so the tests of GICP, KISS-ICP, multiscale ICP and the batch call compare ONE step (or a few) from a
non-trivial start on clouds that are independent samplings of one surface.  This module holds the generators and shows, per case:

  * the oracle's f32 run and its `exact_sums` run (the same f32 terms added in f64) differ by at most FROB_TOL / 3 x scale,
    so no case can miss the budget of h1.transform_budget on rounding alone;
  * the pair counts and error classes each case is built for;
  * the oracle's own share of exactly tied candidates is under the cap the GPU module allows for differing pairs (1e-3).

MUTATION EVIDENCE.  Measured once on a scratch copy of oracle/tc_oracle.c (not committed): the Frobenius distance between the
one-step transform of the unmutated oracle and of five mutants, for every successful GICP case of GICP_ONE_STEP, in units
of FROB_TOL x scale (scale = 1 for all of them).  A case kills a mutant at >= 10.

  (a) R^T C_s R in place of R C_s R^T           (b) the + 1e-4 I regulariser dropped
  (c) denominator n in place of n - 1           (d) k - 1 neighbours
  (e) source covariances rotated by one index (point j weighted with the covariance of point j + 1)

  case                (a)       (b)       (c)       (d)       (e)
  n20_k20               0      2.27     0.119  1.56e+03   0.00216
  refine_k20      2.6e+03  8.13e+03       106       199       936
  s257_t4_k4            0       393       119  7.13e+04  8.06e+03
  s65_t63_k20    1.94e+03      8.84     0.465  1.36e+03  4.39e+03
  sheet_k20           877  2.86e+03      48.3      62.7  1.14e+03
  sheet_k4            566   2.4e+03       133       286       410
  sheet_k5            641  2.85e+03       100       182       501
  sheet_k64      1.29e+03  1.57e+03      14.9      8.41  1.75e+03
  six_near_k4           0    0.0355    0.0113       127      62.9
  volume_k20     1.62e+03      97.4      4.77       172       706
  best case       2.6e+03  8.13e+03       133  7.13e+04  8.06e+03

Every mutant is more than 100 x over the budget in at least one case (last row); the cases that start from the identity
(n20, s257, six_near) cannot see (a), the sheet at k = 64 is the only one that barely sees (d).
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import h1
from threecrate_amd import synth

FROB_TOL = 1e-5                  # the value of tests/test_gpu_parity.py's FROB_TOL (the GPU module imports that one and checks they agree)
MAX_DIFFERING_SHARE = 1e-3       # the share of pairs that may differ from the oracle's, each one an exact f32 tie


IDENTITY7 = np.array([0, 0, 0, 1, 0, 0, 0], np.float32)


# ---- small tools -------------------------------------------------------------------------------------------------------------
def axis_isometry(axis, angle, t=(0.0, 0.0, 0.0)):
    """7-float isometry (qx qy qz qw tx ty tz): rotation by `angle` about `axis`, then translation t."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = 0.5 * float(angle)
    return np.array([*(np.sin(h) * a), np.cos(h), *t], np.float32)


def inverse_apply(T, pts):
    """T^-1 applied in f64, rounded once (input generation)"""
    M = synth.invert_isometry(T)
    return (np.asarray(pts, np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def frob(Ta, Tb):
    M = lambda T: O.isometry_to_matrix(np.asarray(T, np.float32)).astype(np.float64)
    return float(np.linalg.norm(M(Ta) - M(Tb)))


def scale_of(*clouds):
    """the `scale` of h1.transform_budget as the registration tests use it: max(1, max |coordinate| / 10)"""
    return max(1.0, max(float(np.abs(c).max()) for c in clouds if len(c)) / 10.0)


def pairs_equal_or_tied(src, tgt, T_a, T_b, corr_a, corr_b):
    """Two pair lists of the same iteration.  The sources must be the same; a row whose targets differ is accepted only if both
    targets are at the same f32 squared distance (nearest_neighbor.rs:162-167) from the source under side a's transform AND
    under side b's; at most MAX_DIFFERING_SHARE of the rows may differ.  -> number of differing rows."""
    assert len(corr_a) == len(corr_b), (len(corr_a), len(corr_b))
    assert np.array_equal(corr_a[:, 0], corr_b[:, 0])
    diff = np.nonzero(corr_a[:, 1] != corr_b[:, 1])[0]
    assert len(diff) <= MAX_DIFFERING_SHARE * max(len(corr_a), 1), f"{len(diff)} of {len(corr_a)} pairs differ"
    for row in diff:
        j, a, b = int(corr_a[row, 0]), int(corr_a[row, 1]), int(corr_b[row, 1])
        for T in (T_a, T_b):
            ts = O.isometry_apply(T, src[j:j + 1])[0]
            da, db = h1.d2_f32(tgt[a], ts), h1.d2_f32(tgt[b], ts)
            assert da == db, f"source {j}: targets {a} (d2 {da}) and {b} (d2 {db}) are not tied"
    return int(len(diff))


def tie_share(src, tgt, T, corr):
    """share of the pairs whose source has a second target at exactly the matched target's f32 squared distance"""
    if len(corr) == 0:
        return 0.0
    ts = O.isometry_apply(T, src[corr[:, 0]])
    tied = 0
    for b in range(0, len(corr), 256):
        d2 = h1.d2_f32(tgt[None, :, :], ts[b:b + 256, None, :])
        best = d2[np.arange(d2.shape[0]), corr[b:b + 256, 1]]
        tied += int(((d2 == best[:, None]).sum(1) > 1).sum())
    return tied / len(corr)


def outcome(fn, *a, **k):
    """-> (result, None) or (None, oracle error code)"""
    try:
        return fn(*a, **k), None
    except O.OracleError as e:
        return None, e.code


# ---- GICP -----------------------------------------------------------------------------------------------------------------------
SKEW_AXIS = (1.0, 2.0, -1.0)


def sheet(n, seed, amp=0.15, noise=0.004):
    """n points on a curved sheet centred on the origin: z = amp sin(3 x) cos(2.5 y) + small noise, extent about 2 x 1.5 x 0.3"""
    u = synth.uniform_cloud(n, seed).astype(np.float64)
    x, y = 2.0 * (u[:, 0] - 0.5), 1.5 * (u[:, 1] - 0.5)
    z = amp * np.sin(3.0 * x) * np.cos(2.5 * y) + noise * (2.0 * u[:, 2] - 1.0)
    return np.stack([x, y, z], axis=1).astype(np.float32)


SMALL_MOTION = axis_isometry((0.3, -1.0, 0.5), 0.04, (0.02, -0.015, 0.01))
ONE_STEP_INIT = axis_isometry(SKEW_AXIS, 0.3, (0.03, -0.02, 0.015))
LARGE_INIT = axis_isometry(SKEW_AXIS, 1.0, (0.5, -0.3, 0.2))


def gicp_sheet_pair():
    """target: 3 000 points of the sheet; source: an INDEPENDENT sampling of it, 2 963 points, moved by a small isometry"""
    return inverse_apply(SMALL_MOTION, sheet(2963, 12)), sheet(3000, 11)


def gicp_volume_pair():
    """a volumetric pair with independent noise on both sides (isotropic covariances)"""
    src, tgt, _ = synth.registration_pair(2963, seed=5, noise_sigma=0.01)
    return src, tgt


def gicp_refine_pair():
    """The sheet pair with a quarter of the source pushed out of the target's bounding box along +x by 0.2 ... 0.4, seen through
    LARGE_INIT: the queries LARGE_INIT * source are the pushed set (a small motion away from the target), so the out-of-box
    queries reach the refine pass's copy of the accumulation with a rotation far from the identity.
    -> (source, target, indices of the pushed points)"""
    tgt = sheet(3000, 11)
    s = sheet(2963, 12)
    pushed = np.arange(0, len(s), 4)
    u = synth.splitmix_u01(77, np.arange(len(pushed), dtype=np.uint64)).astype(np.float64)
    s[pushed, 0] = (float(tgt[:, 0].max()) + 0.2 + 0.2 * u).astype(np.float32)
    return inverse_apply(LARGE_INIT, inverse_apply(SMALL_MOTION, s)), tgt, pushed


def ball(n, seed, radius=1.0):
    """n points uniform in a ball (rejection from the cube, counter-based)"""
    u = synth.uniform_cloud(4 * n + 64, seed).astype(np.float64) * 2.0 - 1.0
    u = u[(u * u).sum(1) <= 1.0][:n]
    assert len(u) == n
    return (radius * u).astype(np.float32)


BOUNDARY_MOTION = axis_isometry((0.2, 1.0, 0.4), 0.05, (0.01, 0.012, -0.008))


def gicp_boundary_pair(n_near):
    """target: a 200-point ball; source: n_near points within max_correspondence_distance (0.1) of well spread target points
    -- the extreme points of the ball along +-x, +-y, +-z -- plus twenty points far away.  -> (source, target)"""
    tgt = ball(200, 31)
    picks = [int(np.argmax(tgt[:, 0])), int(np.argmin(tgt[:, 0])), int(np.argmax(tgt[:, 1])), int(np.argmin(tgt[:, 1])),
             int(np.argmax(tgt[:, 2])), int(np.argmin(tgt[:, 2]))]
    assert len(set(picks)) == 6 and n_near <= 6
    near = inverse_apply(BOUNDARY_MOTION, tgt[picks[:n_near]])
    far = (ball(20, 32) + np.float32(10.0)).astype(np.float32)
    return np.concatenate([near, far]).astype(np.float32), tgt


def _gicp_small(ns, nt, seed):
    tgt = ball(nt, seed)
    src = inverse_apply(SMALL_MOTION, ball(ns, seed + 1))
    return src, tgt


def _build_gicp_cases():
    """name -> (source, target, init, (max_iterations, max_correspondence_distance, convergence_threshold, k_correspondences))"""
    c = {}
    s, t = gicp_sheet_pair()
    for k in (20, 4, 5, 64):
        c[f"sheet_k{k}"] = (s, t, ONE_STEP_INIT, (1, 0.5, 0.0, k))
    vs, vt = gicp_volume_pair()
    c["volume_k20"] = (vs, vt, ONE_STEP_INIT, (1, 0.5, 0.0, 20))
    rs, rt, _ = gicp_refine_pair()
    c["refine_k20"] = (rs, rt, LARGE_INIT, (1, 1.0, 0.0, 20))
    c["n20_k20"] = (*_gicp_small(20, 20, 41), None, (1, 2.0, 0.0, 20))            # every covariance is the global one
    c["s257_t4_k4"] = (*_gicp_small(257, 4, 43), None, (1, 2.0, 0.0, 4))
    c["s4_t300_k20"] = (*_gicp_small(4, 300, 45), None, (1, 0.5, 0.0, 20))        # fewer source points than k
    c["s4_t300_k4"] = (*_gicp_small(4, 300, 45), None, (1, 0.5, 0.0, 4))          # four pairs at the most
    c["s65_t63_k20"] = (*_gicp_small(65, 63, 47), ONE_STEP_INIT, (1, 1.0, 0.0, 20))
    c["five_near_k4"] = (*gicp_boundary_pair(5), None, (1, 0.1, 0.0, 4))
    c["six_near_k4"] = (*gicp_boundary_pair(6), None, (1, 0.1, 0.0, 4))
    return c


GICP_ONE_STEP = _build_gicp_cases()
# what the oracle makes of each case: None = a transform, else its error code (asserted below)
GICP_EXPECTED_ERROR = {"s4_t300_k20": O.INVALID_DATA, "s4_t300_k4": O.ALGORITHM, "five_near_k4": O.ALGORITHM}
# pairs of the successful cases (asserted below): all of the source but what max_correspondence_distance rejects
GICP_EXPECTED_PAIRS = {"n20_k20": 20, "six_near_k4": 6}


def run_gicp(case, exact_sums=False, max_iterations=None):
    s, t, init, (it, md, thr, k) = GICP_ONE_STEP[case]
    return O.gicp(s, t, init, it if max_iterations is None else max_iterations, md, thr, k, exact_sums=exact_sums)


@pytest.mark.parametrize("case", sorted(GICP_ONE_STEP))
def test_gicp_one_step_cases_are_usable(case):
    s, t, init, (it, md, thr, k) = GICP_ONE_STEP[case]
    r, err = outcome(run_gicp, case)
    assert err == GICP_EXPECTED_ERROR.get(case), (case, err)
    if err is not None:
        return
    e = run_gicp(case, exact_sums=True)
    assert r.iterations == 1 and not r.converged
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(s, t), frob(r.transformation, e.transformation)
    assert np.array_equal(r.correspondences, e.correspondences) and abs(r.mse - e.mse) <= 1e-5 / 3 * e.mse
    if case in GICP_EXPECTED_PAIRS:
        assert len(r.correspondences) == GICP_EXPECTED_PAIRS[case]
    assert len(r.correspondences) >= 6
    T0 = O.IDENTITY if init is None else init
    assert tie_share(s, t, T0, r.correspondences) < MAX_DIFFERING_SHARE
    # the step is a real one: the case would notice a library that returned its start
    assert frob(r.transformation, T0) > 100 * FROB_TOL


def test_gicp_one_step_depends_on_the_covariances():
    """k = 10 instead of 20 moves the sheet's step by far more than the budget, and so does k = 19; the sheet's covariances are
    surface-like, the volume's isotropic."""
    s, t, init, (it, md, thr, k) = GICP_ONE_STEP["sheet_k20"]
    r = run_gicp("sheet_k20")
    assert frob(r.transformation, O.gicp(s, t, init, 1, md, thr, 10).transformation) > 100 * FROB_TOL
    assert frob(r.transformation, O.gicp(s, t, init, 1, md, thr, 19).transformation) > 10 * FROB_TOL
    cov = O.gicp_covariances(t, 20)
    ev = np.linalg.eigvalsh(cov.astype(np.float64))
    assert np.median(ev[:, 0] / ev[:, 2]) < 0.1                     # surface-like on the sheet ...
    cov = O.gicp_covariances(GICP_ONE_STEP["volume_k20"][1], 20)
    ev = np.linalg.eigvalsh(cov.astype(np.float64))
    assert np.median(ev[:, 0] / ev[:, 2]) > 0.15                     # ... and isotropic in the volume


def test_gicp_refine_pair_reaches_out_of_the_box():
    s, t, pushed = gicp_refine_pair()
    q = O.isometry_apply(LARGE_INIT, s)
    assert (q[pushed, 0] > t[:, 0].max() + 0.1).all()                 # the pushed queries lie outside the target's box ...
    r = run_gicp("refine_k20")
    assert np.isin(pushed, r.correspondences[:, 0]).all()             # ... and are paired all the same (max distance 1.0)
    assert len(pushed) * 4 >= len(s) - 3


@pytest.mark.parametrize("steps", [2, 3])
def test_gicp_last_two_steps_have_different_pairs(steps):
    """A run that does not converge returns the mse and the pairs its LAST executed step measured (before that step's update):
    the pairs and mse of steps - 1 differ, so a library that returned the step before (or searched again after) is seen."""
    s, t, init, _ = GICP_ONE_STEP["sheet_k20"]
    a, b = run_gicp("sheet_k20", max_iterations=steps - 1), run_gicp("sheet_k20", max_iterations=steps)
    e = run_gicp("sheet_k20", exact_sums=True, max_iterations=steps)
    assert b.iterations == steps and not b.converged
    assert frob(b.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(s, t) and abs(b.mse - e.mse) <= 1e-5 / 3 * e.mse
    assert not (len(a.correspondences) == len(b.correspondences) and np.array_equal(a.correspondences, b.correspondences))
    assert abs(a.mse - b.mse) > 1e-3 * b.mse
    assert tie_share(s, t, a.transformation, b.correspondences) < MAX_DIFFERING_SHARE


# ---- KISS-ICP ------------------------------------------------------------------------------------------------------------------
KISS_VOXEL = 0.2
KISS_MIN_RANGE, KISS_MAX_RANGE = 0.625, 5.0          # 0.625^2 = 0.390625 and 5^2 = 25 are exact in f32


def kiss_down(src, voxel, min_range, max_range):
    """the down-sampled source the pairs index: range filter (kiss_icp.rs:56-70, f32, inclusive ends) + voxel filter"""
    p = np.asarray(src, np.float32)
    r2 = ((p[:, 0] * p[:, 0]).astype(np.float32) + (p[:, 1] * p[:, 1]).astype(np.float32)).astype(np.float32)
    r2 = (r2 + (p[:, 2] * p[:, 2]).astype(np.float32)).astype(np.float32)
    keep = (r2 >= np.float32(min_range) * np.float32(min_range)) & (r2 <= np.float32(max_range) * np.float32(max_range))
    return O.voxel_grid_filter(p[keep], voxel), r2


def lattice(n, seed, spacing=0.5, jitter=0.1, origin=(-2.0, -2.0, -1.0), side=8):
    """n points of a jittered lattice: neighbours are at least spacing - 2 jitter apart along a lattice axis, so with a voxel
    below that every point keeps a voxel of its own"""
    i = np.arange(n)
    g = np.stack([i % side, (i // side) % side, i // (side * side)], axis=1).astype(np.float64)
    u = synth.uniform_cloud(n, seed).astype(np.float64) * 2.0 - 1.0
    return (np.asarray(origin) + spacing * g + jitter * u).astype(np.float32)


def kiss_range_case():
    """A few hundred points with six special ones, each in a voxel of its own, far from the bulk:
    |p|^2 == max_range^2 exactly ((3, 4, 0): kept), one ulp of |p|^2 inside (kept) and one ulp outside (dropped), and the same
    three at min_range^2 ((0.375, 0.5, 0) = (3, 4, 0) / 8).  The target holds a partner for every special point, dropped ones included.
    -> (source, target, specials (6, 3), kept flags of the specials)"""
    f = np.float32
    dn = lambda v: np.nextafter(f(v), f(0.0))
    specials = np.array([[3.0, 4.0, 0.0], [-3.0, dn(4.0), 0.0], [3.0, -4.0, 0.00125],
                         [0.375, 0.5, 0.0], [-0.375, 0.5, 0.00017], [0.375, -dn(0.5), 0.0]], np.float32)
    kept = np.array([True, True, False, True, True, False])
    bulk_t = lattice(300, 51, origin=(-1.75, -1.75, 0.9), side=8)              # z >= 0.8: clear of the specials (z = 0)
    bulk_s = inverse_apply(SMALL_MOTION, bulk_t[:240])
    tgt = np.concatenate([bulk_t, specials + f(0.01)]).astype(np.float32)
    src = np.concatenate([bulk_s[:100], specials[:3], bulk_s[100:], specials[3:]]).astype(np.float32)
    return src, tgt, specials, kept


KISS_PRIORS = {"identity": np.array([0, 0, 0, 1, 0, 0, 0], np.float32),                       # 3 voxels
               "between": axis_isometry(SKEW_AXIS, 0.4, (0.3, 0.0, 0.0)),                     # 3 * motion, strictly between
               "five_metres": np.array([0, 0, 0, 1, 5.0, 0, 0], np.float32)}                  # 10 voxels


def kiss_prior_case(name):
    """target: a jittered lattice; the queries prior * source are target points pushed away from the lattice by 0 ... 2.4 (well
    past 10 voxels), so the number of pairs tells the three adaptive thresholds apart.  -> (source, target, prior)"""
    tgt = lattice(400, 53, spacing=0.25, jitter=0.05, origin=(-1.0, -1.0, -1.0), side=8)
    base = tgt[:300].astype(np.float64)
    u = synth.splitmix_u01(91, np.arange(len(base), dtype=np.uint64)).astype(np.float64)
    base[:, 2] = float(tgt[:, 2].min()) - 2.4 * u                              # below the lowest layer: NN distance ~ the push
    prior = KISS_PRIORS[name]
    return inverse_apply(prior, base.astype(np.float32)), tgt, prior


def kiss_size_case(n_down):
    """a source whose voxel filter leaves exactly n_down points (n_down >= 3: lattice points; 1 or 2: fifty points in one / two voxels;
    "row5": five nearly collinear points far from the target's box centre)"""
    tgt = lattice(300, 55)
    if n_down == "row5":
        # The lattice's first five points: a row 1.7 from the target's box centre with 0.1 of scatter across it.  The rotation about
        # the row is settled by products of a few 1e-2; the oracle, which centres on the centroids before it multiplies, is 5e-7 from
        # the same step in f64, and one-ulp moves of the input move it by 1.8e-6.  (Sums of f32 products of coordinates taken from
        # the box centre end 3.0e-5 away: what icp_exact_p2p_sums_kernel is there for.)
        return inverse_apply(SMALL_MOTION, tgt[:5]), tgt
    if n_down >= 3:
        # spread over the lattice, with noise of their own (an exact copy ends at a residual of zero, where the mse is rounding)
        src = inverse_apply(SMALL_MOTION, tgt[(np.arange(n_down) * 37) % len(tgt)])
        return (src + synth.gaussian_noise(n_down, 59, 0.01)).astype(np.float32), tgt
    u = synth.uniform_cloud(50, 57).astype(np.float64) * 0.15
    u[:, 0] += 1.01 + 0.2 * (np.arange(50) % n_down)                           # inside the voxel(s) [1.0, 1.2) (, [1.2, 1.4)) x [0, 0.2)^2
    return u.astype(np.float32), tgt


def kiss_step_f64(down, tgt, prior, corr):
    """svd_transform (kiss_icp.rs:102-162) on the given pairs in f64, composed with the prior: the 4 x 4 matrix one iteration
    of kiss_icp would return in exact arithmetic (the queries are the oracle's f32 prior * source)"""
    start = IDENTITY7 if prior is None else prior
    vs = O.isometry_apply(start, down[corr[:, 0]]).astype(np.float64)
    vq = tgt[corr[:, 1]].astype(np.float64)
    cs, cq = vs.mean(0), vq.mean(0)
    U, _, Vt = np.linalg.svd((vs - cs).T @ (vq - cq))
    Rm = Vt.T @ U.T
    if np.linalg.det(Rm) < 0:
        Vt[2] = -Vt[2]
        Rm = Vt.T @ U.T
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = Rm, cq - Rm @ cs
    return D @ O.isometry_to_matrix(start).astype(np.float64)


def kiss_f32_error(src, tgt, prior, r, min_range=0.0, max_range=100.0):
    """how far the oracle's f32 step is from the same step in f64 (f32 centroids, products and SVD: conditioning shows here)"""
    down, _ = kiss_down(src, KISS_VOXEL, min_range, max_range)
    return float(np.linalg.norm(O.isometry_to_matrix(r.transformation).astype(np.float64) - kiss_step_f64(down, tgt, prior, r.correspondences)))


def run_kiss(src, tgt, prior, exact_sums=False, voxel_order_seed=0, min_range=0.0, max_range=100.0, max_iterations=1):
    return O.kiss_icp(src, tgt, prior, KISS_VOXEL, max_range, min_range, max_iterations, exact_sums=exact_sums,
                      voxel_order_seed=voxel_order_seed)


def test_kiss_range_filter_ends_are_visible_in_the_oracle():
    src, tgt, specials, kept = kiss_range_case()
    down, r2 = kiss_down(src, KISS_VOXEL, KISS_MIN_RANGE, KISS_MAX_RANGE)
    sp = np.concatenate([np.arange(100, 103), np.arange(len(src) - 3, len(src))])
    assert np.array_equal(src[sp], specials)
    lo, hi = np.float32(KISS_MIN_RANGE) ** 2, np.float32(KISS_MAX_RANGE) ** 2
    assert r2[sp[0]] == hi and r2[sp[1]] == np.nextafter(hi, np.float32(0)) and r2[sp[2]] == np.nextafter(hi, np.float32(np.inf))
    assert r2[sp[3]] == lo and r2[sp[4]] == np.nextafter(lo, np.float32(np.inf)) and r2[sp[5]] == np.nextafter(lo, np.float32(0))
    (r, nd), err = outcome(run_kiss, src, tgt, None, min_range=KISS_MIN_RANGE, max_range=KISS_MAX_RANGE)
    assert err is None and nd == len(down)
    # every special point has a voxel of its own: exclusive ends would lose two of them, ends one ulp wider would gain two
    bulk = np.delete(np.arange(len(src)), sp)
    n_bulk = len(kiss_down(src[bulk], KISS_VOXEL, KISS_MIN_RANGE, KISS_MAX_RANGE)[0])
    assert nd == n_bulk + int(kept.sum()) and n_bulk == len(bulk)
    # the kept specials are paired with their partners (the last six target points), the dropped ones are not in the list
    for p, k in zip(range(6), kept):
        hit = np.nonzero((down == specials[p]).all(1))[0]
        assert len(hit) == (1 if k else 0)
        if k:
            row = np.nonzero(r.correspondences[:, 0] == hit[0])[0]
            assert len(row) == 1 and r.correspondences[row[0], 1] == len(tgt) - 6 + p
    e, _ = run_kiss(src, tgt, None, exact_sums=True, min_range=KISS_MIN_RANGE, max_range=KISS_MAX_RANGE)
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(src, tgt)
    assert kiss_f32_error(src, tgt, None, r, KISS_MIN_RANGE, KISS_MAX_RANGE) <= FROB_TOL / 3 * scale_of(src, tgt)
    assert tie_share(down, tgt, O.IDENTITY, r.correspondences) < MAX_DIFFERING_SHARE


def test_kiss_three_priors_give_three_thresholds_and_three_pair_counts():
    want = {"identity": 3 * KISS_VOXEL, "five_metres": 10 * KISS_VOXEL}
    counts = {}
    for name, prior in KISS_PRIORS.items():
        sigma = O.kiss_adaptive_threshold(prior, KISS_VOXEL)
        if name in want:
            assert sigma == pytest.approx(want[name], rel=1e-6)
        else:
            assert 3 * KISS_VOXEL * 1.2 < sigma < 10 * KISS_VOXEL / 1.2
        src, tgt, _ = kiss_prior_case(name)
        r, nd = run_kiss(src, tgt, prior)
        e, _ = run_kiss(src, tgt, prior, exact_sums=True)
        assert r.iterations == 1 and not r.converged
        assert frob(r.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(src, tgt), name
        assert kiss_f32_error(src, tgt, prior, r) <= FROB_TOL / 3 * scale_of(src, tgt), name
        down, _ = kiss_down(src, KISS_VOXEL, 0.0, 100.0)
        assert nd == len(down)
        assert tie_share(down, tgt, prior, r.correspondences) < MAX_DIFFERING_SHARE
        counts[name] = len(r.correspondences)
    assert 3 <= counts["identity"] < counts["between"] < counts["five_metres"] < 300, counts


KISS_SIZES = [1, 2, 5, 64, 257, "row5"]


def ulp_moved(a, seed):
    """every coordinate moved by -1, 0 or +1 ulp"""
    d = np.random.default_rng(seed).integers(-1, 2, a.shape)
    up, dn = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))
    return np.where(d > 0, up, np.where(d < 0, dn, a)).astype(np.float32)


@pytest.mark.parametrize("n_down", KISS_SIZES)
def test_kiss_size_cases_have_the_size_they_claim(n_down):
    src, tgt = kiss_size_case(n_down)
    want = 5 if n_down == "row5" else n_down
    assert len(kiss_down(src, KISS_VOXEL, 0.0, 100.0)[0]) == want
    res, err = outcome(run_kiss, src, tgt, None)
    if want < 3:
        assert err == O.ALGORITHM              # fewer than three pairs (kiss_icp.rs:256-262)
        return
    r, nd = res
    assert nd == want and len(r.correspondences) == want
    e, _ = run_kiss(src, tgt, None, exact_sums=True)
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(src, tgt)
    assert kiss_f32_error(src, tgt, None, r) <= FROB_TOL / 3 * scale_of(src, tgt)
    # the case is no harder than that for the reference: one-ulp moves of the input move its step by less than a third of the budget
    assert max(frob(r.transformation, run_kiss(ulp_moved(src, sd), tgt, None)[0].transformation) for sd in range(5)) <= FROB_TOL / 3
    if n_down != "row5":
        assert r.mse > 1e-5                   # a residual the mse can be compared at


# ---- few pairs out of a large source ------------------------------------------------------------------------------------------------
# A source of 4 096 ... 20 000 points of which max_correspondence_distance keeps a handful: the pairs' terms are all that decides the
# step, and the size of the source decides which kernels of the library form them (tests/test_gpu_icp_few_pairs.py).
FEW_KINDS = ["row5", 3, 64, 257]
FEW_SIZES = [4096, 4097, 20000]          # the last source size the exact sums served by size alone, the first they did not, several main-pass blocks
FEW_PLACEMENTS = ["spread", "block"]
FEW_MAX_DIST = 0.6
FEW_CASES = [(k, n, p) for k in FEW_KINDS for n in FEW_SIZES for p in FEW_PLACEMENTS]
FEW_THREE = (0, 2, 7)                    # the lattice points of kind 3 (see few_pairs_case)


def few_id(case):
    return "-".join(str(c) for c in case)


def far_filler(n, seed):
    """n points of uniform_cloud * 4 + 6: every coordinate in [6, 10), more than 4 from every point of lattice() and sheet()"""
    return (synth.uniform_cloud(n, seed).astype(np.float64) * 4.0 + 6.0).astype(np.float32)


def place_rows(filler, rows, placement):
    """`rows` written over len(rows) points of `filler`: "spread" at (i * (ns // m) + ns // 11) % ns (pairs that meet only when
    blocks are folded), "block" in one contiguous run from ns // 3 (pairs that meet in one wave).  -> (cloud, indices of the rows)"""
    ns, m = len(filler), len(rows)
    at = (np.arange(m) * (ns // m) + ns // 11) % ns if placement == "spread" else ns // 3 + np.arange(m)
    assert len(set(at.tolist())) == m and at.max() < ns
    out = filler.copy()
    out[at] = rows
    return out, at


def few_pairs_rows(kind, tgt):
    if kind == "row5":
        return inverse_apply(SMALL_MOTION, tgt[:5])                   # kiss_size_case("row5")'s rows
    if kind == 3:
        return inverse_apply(SMALL_MOTION, tgt[list(FEW_THREE)])
    src = inverse_apply(SMALL_MOTION, tgt[(np.arange(kind) * 37) % len(tgt)])      # as kiss_size_case builds them: the mse is comparable
    return (src + synth.gaussian_noise(kind, 59, 0.01)).astype(np.float32)


def few_pairs_case(kind, ns, placement):
    """Point-to-point: `ns` source points of which FEW_MAX_DIST pairs only the rows of `kind` with lattice(300, 55); the rest is
    far_filler.  "row5": the five nearly collinear rows of kiss_size_case("row5"), 1.7 from the target's box centre.  64 / 257: noisy
    copies of spread lattice points.  3: the minimum pair count, lattice points 0, 2 and 7 of the first row.  (The first three points
    of that row are NOT usable: the oracle's own f32 step is 4.2e-6 from the same step in f64 and one-ulp moves of the input move it
    by up to 1.5e-5, both over a third of the budget -- test_the_first_three_lattice_points_are_no_usable_case; of the 56 triples of
    the row's eight points, (0, 2, 7) is the one with the smallest sensitivity to one-ulp moves, 2.4e-6, that still sees the
    uncentred f32 sums, 3.4e-5.)  Every coordinate of both clouds lies within +-10.  -> (source, target, max_dist)"""
    tgt = lattice(300, 55)
    src, _ = place_rows(far_filler(ns, 63), few_pairs_rows(kind, tgt), placement)
    return src, tgt, FEW_MAX_DIST


def few_pairs_count(kind):
    return 5 if kind == "row5" else kind


def run_few(src, tgt, max_dist, exact_sums=False, max_iters=1):
    return O.icp_detailed(src, tgt, None, max_iters, max_dist, 0.0, exact_sums=exact_sums)


def matrix64(T):
    return O.isometry_to_matrix(np.asarray(T, np.float32)).astype(np.float64)


def uncentred_f32_step(src, tgt, start, corr):
    """The device's point-to-point arithmetic WITHOUT the exact sums, restated: coordinates taken from the f32 centre of the target's
    box, every product rounded to f32, the sums folded in f32 (in pair order); H = S - n ms mq^T and the Kabsch solve in f64.
    -> the 4 x 4 matrix of one step"""
    f = np.float32
    start = IDENTITY7 if start is None else start
    c = ((tgt.min(0) + tgt.max(0)) * f(0.5)).astype(f)
    sv = (O.isometry_apply(start, src[corr[:, 0]]) - c).astype(f)
    tv = (tgt[corr[:, 1]] - c).astype(f)
    n = len(corr)
    fold = lambda a: np.add.accumulate(a, axis=0, dtype=f)[-1].astype(np.float64)
    ms, mq = fold(sv) / n, fold(tv) / n
    S = fold((sv[:, :, None] * tv[:, None, :]).astype(f).reshape(n, 9)).reshape(3, 3)
    U, _, Vt = np.linalg.svd(S - n * np.outer(ms, mq))
    Rm = Vt.T @ U.T
    if np.linalg.det(Rm) < 0:
        Vt[2] = -Vt[2]
        Rm = Vt.T @ U.T
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = Rm, (mq + c) - Rm @ (ms + c)
    return D @ matrix64(start)


def _usable(run, src, step_f64, down=None, tgt=None, start=None):
    """the usability rules of a one-step case; run(source, exact_sums) -> result, step_f64(result) -> 4 x 4 in f64"""
    r, e = run(src, False), run(src, True)
    assert r.iterations == 1 and not r.converged
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3
    assert float(np.linalg.norm(matrix64(r.transformation) - step_f64(r))) <= FROB_TOL / 3
    assert max(frob(r.transformation, run(ulp_moved(src, sd), False).transformation) for sd in range(5)) < FROB_TOL / 3
    assert tie_share(src if down is None else down, tgt, O.IDENTITY if start is None else start, r.correspondences) < MAX_DIFFERING_SHARE
    return r


@pytest.mark.parametrize("case", FEW_CASES, ids=few_id)
def test_few_pairs_cases_are_usable(case):
    src, tgt, md = few_pairs_case(*case)
    assert len(src) == case[1] and scale_of(src, tgt) == 1.0
    r = _usable(lambda s, ex: run_few(s, tgt, md, ex), src, lambda r: kiss_step_f64(src, tgt, None, r.correspondences), tgt=tgt)
    assert len(r.correspondences) == few_pairs_count(case[0])
    # the pairs are the placed rows, and the filler is farther than max_dist from every target point
    _, at = place_rows(far_filler(case[1], 63), few_pairs_rows(case[0], tgt), case[2])
    assert np.array_equal(r.correspondences[:, 0], np.sort(at))
    assert float(np.abs(np.delete(src, at, axis=0)).min()) >= 6.0 > float(np.abs(tgt).max()) + md
    if case[0] in (64, 257):
        assert r.mse > 1e-5


def test_the_first_three_lattice_points_are_no_usable_case():
    """why kind 3 is not tgt[:3]: the reference itself is not good to a third of the budget there"""
    tgt = lattice(300, 55)
    src, _ = place_rows(far_filler(4097, 63), inverse_apply(SMALL_MOTION, tgt[:3]), "spread")
    r = run_few(src, tgt, FEW_MAX_DIST)
    assert len(r.correspondences) == 3
    assert float(np.linalg.norm(matrix64(r.transformation) - kiss_step_f64(src, tgt, None, r.correspondences))) > FROB_TOL / 3
    assert max(frob(r.transformation, run_few(ulp_moved(src, sd), tgt, FEW_MAX_DIST).transformation) for sd in range(5)) > FROB_TOL / 3


@pytest.mark.parametrize("case", [c for c in FEW_CASES if c[0] in ("row5", 3)], ids=few_id)
def test_few_pairs_cases_see_uncentred_f32_sums(case):
    """MUTATION EVIDENCE: the device's arithmetic without the exact sums (uncentred_f32_step) is more than three budgets from the
    oracle on every "row5" and 3 case (the pairs, and so the figure, do not depend on the size of the source: 3.1e-5 and 3.4e-5),
    while the oracle is within a third of a budget of the f64 step (test_few_pairs_cases_are_usable)."""
    src, tgt, md = few_pairs_case(*case)
    r = run_few(src, tgt, md)
    assert float(np.linalg.norm(uncentred_f32_step(src, tgt, None, r.correspondences) - matrix64(r.transformation))) > 3 * FROB_TOL
    if case[1] >= 4097:
        assert len(src) > 4096 >= len(r.correspondences)


def test_uncentred_f32_sums_do_not_hurt_well_spread_pairs():
    """the restatement is not a wrong solve: on 64 and 257 spread pairs it is within a tenth of a budget of the f64 step"""
    for kind in (64, 257):
        src, tgt, md = few_pairs_case(kind, 4097, "spread")
        r = run_few(src, tgt, md)
        f64 = kiss_step_f64(src, tgt, None, r.correspondences)
        assert float(np.linalg.norm(uncentred_f32_step(src, tgt, None, r.correspondences) - f64)) < FROB_TOL / 10


def test_few_pairs_three_steps_keep_the_five_pairs():
    """three steps at threshold 0 on the row5 case: every step pairs the five rows, and the run is usable as a whole"""
    src, tgt, md = few_pairs_case("row5", 4097, "spread")
    r, e = run_few(src, tgt, md, max_iters=3), run_few(src, tgt, md, True, max_iters=3)
    assert r.iterations == 3 and not r.converged and len(r.correspondences) == 5
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3
    for k in (1, 2):
        assert np.array_equal(run_few(src, tgt, md, max_iters=k).correspondences, r.correspondences)
    assert max(frob(r.transformation, run_few(ulp_moved(src, sd), tgt, md, max_iters=3).transformation) for sd in range(5)) < FROB_TOL / 3


def kiss_few_pairs_case():
    """KISS-ICP: a source whose voxel filter leaves 4 205 points -- 4 200 of a jittered lattice with a voxel each, x >= 2.5, and the
    five "row5" rows in the middle of the array -- of which sigma (3 voxels = 0.6 at the identity prior) pairs the five rows only
    -> (source, target)"""
    tgt = lattice(300, 55)
    fill = lattice(4200, 67, spacing=0.45, jitter=0.1, origin=(2.6, -3.5, -3.5), side=16)
    return np.concatenate([fill[:2000], inverse_apply(SMALL_MOTION, tgt[:5]), fill[2000:]]).astype(np.float32), tgt


def test_kiss_few_pairs_case_is_usable():
    src, tgt = kiss_few_pairs_case()
    assert scale_of(src, tgt) == 1.0
    down, _ = kiss_down(src, KISS_VOXEL, 0.0, 100.0)
    assert len(down) == len(src) == 4205 > 4096
    assert O.kiss_adaptive_threshold(IDENTITY7, KISS_VOXEL) == pytest.approx(3 * KISS_VOXEL, rel=1e-6)
    run = lambda s, ex: run_kiss(s, tgt, None, exact_sums=ex)[0]
    r = _usable(run, src, lambda r: kiss_step_f64(down, tgt, None, r.correspondences), down=down, tgt=tgt)
    assert len(r.correspondences) == 5 and run_kiss(src, tgt, None)[1] == 4205
    assert float(np.linalg.norm(uncentred_f32_step(down, tgt, None, r.correspondences) - matrix64(r.transformation))) > 3 * FROB_TOL


# ---- point-to-plane, few pairs ------------------------------------------------------------------------------------------------------
P2PLANE_FEW_PAIRS = [7, 12, 64]
P2PLANE_FEW_MAX_DIST = 0.3
_P2PLANE_TARGET = []


def p2plane_few_target():
    """sheet(3000, 11) and the oracle's k = 16 normals of it (computed once)"""
    if not _P2PLANE_TARGET:
        tgt = sheet(3000, 11)
        _P2PLANE_TARGET.append((tgt, np.ascontiguousarray(O.estimate_normals(tgt, 16)[:, 3:6])))
    return _P2PLANE_TARGET[0]


def p2plane_few_case(m):
    """Point-to-plane: 4 097 source points of which P2PLANE_FEW_MAX_DIST pairs m noisy copies of spread sheet points (spread over the
    array); the rest is far_filler.  m = 7, 12, 64.  Six pairs, the minimum, are NOT usable: the 6 x 6 system is just determined,
    the oracle's f32 step is 8.5e-6 from the same step in f64 and one-ulp moves of the input move it by 1.8e-5
    (test_six_point_to_plane_pairs_are_no_usable_case); seven is the next count that passes.  -> (source, target, normals, max_dist)"""
    tgt, nrm = p2plane_few_target()
    rows = inverse_apply(SMALL_MOTION, tgt[(np.arange(m) * 296 + 5) % len(tgt)])
    rows = (rows + synth.gaussian_noise(m, 59, 0.01)).astype(np.float32)
    src, _ = place_rows(far_filler(4097, 65), rows, "spread")
    return src, tgt, nrm, P2PLANE_FEW_MAX_DIST


def p2plane_step_f64(src, tgt, nrm, start, corr, b_sign=1.0, swapped_cross=False):
    """compute_transformation_point_to_plane (registration.rs:395-450) on the given pairs in f64, composed with the start: rows
    a = [s x n, n], b = n . (q - s), the 6 x 6 normal equations, Rz Ry Rx of the first three unknowns.  b_sign = -1 and
    swapped_cross (n x s) are the mutants of the mutation test.  -> 4 x 4"""
    start = IDENTITY7 if start is None else start
    s = O.isometry_apply(start, src[corr[:, 0]]).astype(np.float64)
    q, n = tgt[corr[:, 1]].astype(np.float64), nrm[corr[:, 1]].astype(np.float64)
    A = np.concatenate([np.cross(n, s) if swapped_cross else np.cross(s, n), n], axis=1)
    x = np.linalg.solve(A.T @ A, A.T @ (b_sign * (n * (q - s)).sum(1)))
    (cx, cy, cz), (sx, sy, sz) = np.cos(x[:3]), np.sin(x[:3])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    D = np.eye(4)
    D[:3, :3], D[:3, 3] = Rz @ Ry @ Rx, x[3:]
    return D @ matrix64(start)


def run_p2plane_few(src, tgt, nrm, md, exact_sums=False):
    return O.icp_point_to_plane_detailed(src, tgt, nrm, None, 1, md, 0.0, exact_sums=exact_sums)


@pytest.mark.parametrize("m", P2PLANE_FEW_PAIRS)
def test_p2plane_few_pairs_cases_are_usable(m):
    src, tgt, nrm, md = p2plane_few_case(m)
    assert len(src) == 4097 and scale_of(src, tgt) == 1.0
    r = _usable(lambda s, ex: run_p2plane_few(s, tgt, nrm, md, ex), src, lambda r: p2plane_step_f64(src, tgt, nrm, None, r.correspondences), tgt=tgt)
    assert len(r.correspondences) == m and r.mse > 1e-5


def test_six_point_to_plane_pairs_are_no_usable_case():
    src, tgt, nrm, md = p2plane_few_case(6)
    r = run_p2plane_few(src, tgt, nrm, md)
    assert len(r.correspondences) == 6
    assert float(np.linalg.norm(matrix64(r.transformation) - p2plane_step_f64(src, tgt, nrm, None, r.correspondences))) > FROB_TOL / 3
    assert max(frob(r.transformation, run_p2plane_few(ulp_moved(src, sd), tgt, nrm, md).transformation) for sd in range(5)) > FROB_TOL / 3


def test_p2plane_few_pairs_cases_see_the_sign_of_b_and_the_order_of_the_cross_product():
    """MUTATION EVIDENCE: b = n . (s - q) in place of n . (q - s), and n x s in place of s x n, each move the f64 step by more than
    100 budgets in some case (measured: 1.8e-1 ... 2.8e-1 and 1.3e-1 ... 2.5e-1, over 10^4 budgets in every case)"""
    worst = {"b": 0.0, "cross": 0.0}
    for m in P2PLANE_FEW_PAIRS:
        src, tgt, nrm, md = p2plane_few_case(m)
        corr = run_p2plane_few(src, tgt, nrm, md).correspondences
        good = p2plane_step_f64(src, tgt, nrm, None, corr)
        worst["b"] = max(worst["b"], float(np.linalg.norm(p2plane_step_f64(src, tgt, nrm, None, corr, b_sign=-1.0) - good)))
        worst["cross"] = max(worst["cross"], float(np.linalg.norm(p2plane_step_f64(src, tgt, nrm, None, corr, swapped_cross=True) - good)))
    assert worst["b"] > 100 * FROB_TOL and worst["cross"] > 100 * FROB_TOL, worst


# ---- multiscale ICP -----------------------------------------------------------------------------------------------------------
MULTISCALE_LEVELS = [(2.0, 5, 1.0), (0.5, 5, 0.5), (0.1, 10, 0.2)]
MULTISCALE_ALL_COARSE = [(2.0, 5, 1.0), (4.0, 5, None)]
MULTISCALE_TAIL = (10, 0.10, 1e-5)          # final_refinement_iterations, final_max_correspondence_distance, convergence_threshold
MULTISCALE_INIT = axis_isometry(SKEW_AXIS, 0.5, (0.4, -0.2, 0.1))


def multiscale_pair(init=None):
    """a 400-point pair spanning about 1 m; with `init` the source is moved so that init roughly aligns it"""
    src, tgt, _ = synth.registration_pair(400, seed=61, noise_sigma=0.002)
    return (src if init is None else inverse_apply(init, src)), tgt


def multiscale_biting_pair():
    """the pair with 40 % of the source lifted 1.6 above the scene: both levels' distances (0.5, 0.15) drop those pairs"""
    src, tgt = multiscale_pair()
    src = src.copy()
    src[np.arange(len(src)) % 5 < 2, 2] += np.float32(1.6)
    return src, tgt


MULTISCALE_BITING_LEVELS = [(0.3, 5, 0.5), (0.02, 10, 0.15)]


def run_multiscale(src, tgt, init, levels, exact_sums=False):
    """exact_sums: every level's Kabsch sums with their f32 terms added in f64 (the oracle's diagnostic switch, as icp_detailed sets it)"""
    O.lib().tco_set_exact_sums(1 if exact_sums else 0)
    try:
        return O.multiscale_icp_point_to_point(src, tgt, init, levels, *MULTISCALE_TAIL)
    finally:
        O.lib().tco_set_exact_sums(0)


def multiscale_cases():
    """name -> (source, target, init, levels) of the runs that succeed"""
    return {"skipped_level": (*multiscale_pair(), None, MULTISCALE_LEVELS),
            "init": (*multiscale_pair(MULTISCALE_INIT), MULTISCALE_INIT, MULTISCALE_LEVELS),
            "biting": (*multiscale_biting_pair(), None, MULTISCALE_BITING_LEVELS)}


MULTISCALE_FEW_LEVELS = [(0.6, 4, 0.8), (0.25, 6, 0.6)]


MULTISCALE_FEW_KINDS = {"twenty": (MULTISCALE_FEW_LEVELS, 20), "row5": ([(0.3, 4, 0.8), (0.25, 6, 0.6)], 5)}


def multiscale_few_pairs_case(kind="twenty"):
    """4 320 / 4 305 source points -- 4 300 of a jittered lattice at x >= 2.7, a voxel each at every level that runs, and, in the
    middle of the array, "twenty": twenty noisy copies of spread target lattice points; "row5": the five nearly collinear rows of
    kiss_size_case("row5"), which see uncentred f32 sums -- of which every level's distance (and the final 0.10) pairs those rows
    only.  Every step's mse changes by 1e-4 or more, or by 1e-13 or less: no stop decision is near the threshold (1e-5).
    -> (source, target, init, levels)"""
    tgt = lattice(300, 55)
    levels, m = MULTISCALE_FEW_KINDS[kind]
    if kind == "row5":
        rows = inverse_apply(SMALL_MOTION, tgt[:5])
    else:
        rows = (inverse_apply(SMALL_MOTION, tgt[(np.arange(m) * 37) % len(tgt)]) + synth.gaussian_noise(m, 59, 0.01)).astype(np.float32)
    fill = lattice(4300, 69, spacing=0.45, jitter=0.08, origin=(2.8, -3.5, -3.5), side=16)
    return np.concatenate([fill[:1500], rows, fill[1500:]]).astype(np.float32), tgt, None, levels


def _multiscale_few_pairs_usable(kind):
    src, tgt, init, levels = multiscale_few_pairs_case(kind)
    m = MULTISCALE_FEW_KINDS[kind][1]
    assert scale_of(src, tgt) == 1.0
    (v0, it0, md0), (v1, it1, md1) = levels
    sd0 = O.voxel_grid_filter(src, v0)
    first = O.icp_point_to_point(sd0, O.voxel_grid_filter(tgt, v0), None, it0, MULTISCALE_TAIL[2], md0)
    sd, td = O.voxel_grid_filter(src, v1), O.voxel_grid_filter(tgt, v1)
    assert len(sd) == len(src) > 4096                               # the finest level's source ...
    finest = O.icp_point_to_point(sd, td, first.transformation, 1, MULTISCALE_TAIL[2], md1)
    assert 3 <= len(finest.correspondences) == m < 64               # ... of which the level's distance keeps m
    if kind == "row5":
        assert len(sd0) > 4096 and len(first.correspondences) == 5  # the coarser level is of the same kind
    r, e = run_multiscale(src, tgt, init, levels), run_multiscale(src, tgt, init, levels, exact_sums=True)
    assert (r.iterations, r.converged) == (e.iterations, e.converged) and len(r.correspondences) == m
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3
    for sdd in range(5):
        u = run_multiscale(ulp_moved(src, sdd), tgt, init, levels)
        assert (u.iterations, u.converged) == (r.iterations, r.converged) and frob(r.transformation, u.transformation) < FROB_TOL / 3


def test_multiscale_few_pairs_case_is_usable():
    _multiscale_few_pairs_usable("twenty")


def test_multiscale_row5_pairs_case_is_usable():
    _multiscale_few_pairs_usable("row5")


@pytest.mark.parametrize("name", ["skipped_level", "init", "biting"])
def test_multiscale_cases_do_not_hang_on_rounding(name):
    src, tgt, init, levels = multiscale_cases()[name]
    r, e = run_multiscale(src, tgt, init, levels), run_multiscale(src, tgt, init, levels, exact_sums=True)
    assert (r.iterations, r.converged) == (e.iterations, e.converged)
    assert frob(r.transformation, e.transformation) <= FROB_TOL / 3 * scale_of(src, tgt)


def test_multiscale_level_zero_is_skipped_and_the_others_run():
    src, tgt = multiscale_pair()
    assert len(O.voxel_grid_filter(tgt, 2.0)) < 3                                  # level 0: `continue` (registration.rs:749-751)
    for v in (0.5, 0.1):
        assert len(O.voxel_grid_filter(tgt, v)) >= 3 and len(O.voxel_grid_filter(src, v)) >= 3
    r = run_multiscale(src, tgt, None, MULTISCALE_LEVELS)
    assert r.iterations >= 3
    # the skipped level leaves no trace: the same run without it
    r2 = run_multiscale(src, tgt, None, MULTISCALE_LEVELS[1:])
    assert np.array_equal(r.transformation, r2.transformation) and r.iterations == r2.iterations


def test_multiscale_all_levels_skipped_is_an_algorithm_error():
    src, tgt = multiscale_pair()
    for v, _, _ in MULTISCALE_ALL_COARSE:
        assert len(O.voxel_grid_filter(tgt, v)) < 3
    assert outcome(run_multiscale, src, tgt, None, MULTISCALE_ALL_COARSE)[1] == O.ALGORITHM      # registration.rs:767-771


def test_multiscale_init_matters():
    src, tgt = multiscale_pair(MULTISCALE_INIT)
    r = run_multiscale(src, tgt, MULTISCALE_INIT, MULTISCALE_LEVELS)
    res0, err0 = outcome(run_multiscale, src, tgt, None, MULTISCALE_LEVELS)
    assert err0 is not None or frob(r.transformation, res0.transformation) > 1000 * FROB_TOL


def test_multiscale_level_distance_removes_a_third_of_the_pairs():
    src, tgt = multiscale_biting_pair()
    (v0, it0, md0), (v1, it1, md1) = MULTISCALE_BITING_LEVELS
    first = O.icp_point_to_point(O.voxel_grid_filter(src, v0), O.voxel_grid_filter(tgt, v0), None, it0, MULTISCALE_TAIL[2], md0)
    sd, td = O.voxel_grid_filter(src, v1), O.voxel_grid_filter(tgt, v1)
    with_md = O.icp_point_to_point(sd, td, first.transformation, 1, MULTISCALE_TAIL[2], md1)
    without = O.icp_point_to_point(sd, td, first.transformation, 1, MULTISCALE_TAIL[2], None)
    assert len(without.correspondences) == len(sd)
    assert len(with_md.correspondences) <= 2 * len(sd) // 3, (len(with_md.correspondences), len(sd))
    assert len(with_md.correspondences) >= len(sd) // 2
    run_multiscale(src, tgt, None, MULTISCALE_BITING_LEVELS)


# ---- batch ---------------------------------------------------------------------------------------------------------------------
def batch_jobs():
    """five point-to-point jobs of 300 ... 2 000 points with different motions, iteration caps, thresholds and distances
    -> [(source, target, max_iterations, convergence_threshold, max_correspondence_distance)]"""
    spec = [(300, 71, 5, 1e-6, 0.5, 0.02), (2000, 72, 12, 1e-7, 0.06, 0.05), (777, 73, 1, 1e-6, 1.0, 0.05),
            (1025, 74, 30, 1e-5, 0.3, 0.12), (1500, 75, 4, 1e-9, 0.08, 0.08)]
    jobs = []
    for n, seed, iters, thr, md, motion in spec:
        T = synth.yaw_isometry((motion, -0.5 * motion, 0.3 * motion), motion)
        _, tgt, _ = synth.registration_pair(n, seed=seed, noise_sigma=0.003, transform=T)
        scene = synth.uniform_cloud(n, seed).astype(np.float64)
        m = n // 10                            # the last tenth of the scene is seen 0.02 ... 0.42 above it: the distance drops some of it
        scene[n - m:, 2] = 1.02 + 0.4 * synth.splitmix_u01(seed + 100, np.arange(m, dtype=np.uint64)).astype(np.float64)
        src = (inverse_apply(T, scene) + synth.gaussian_noise(n, seed + 200, 0.003)).astype(np.float32)
        jobs.append((src, tgt, iters, thr, md))
    return jobs


def test_batch_jobs_run_in_the_oracle_and_end_differently():
    ends = set()
    for src, tgt, iters, thr, md in batch_jobs():
        r = O.icp_point_to_point(src, tgt, None, iters, thr, md)
        assert 1 <= r.iterations <= iters and 0.9 * len(src) <= len(r.correspondences) <= len(src)
        ends.add((r.iterations, r.converged, len(r.correspondences) < len(src)))
    # the jobs do not all stop the same way: some converge, some hit their cap; the distance drops pairs in some
    assert len(ends) >= 4 and len({e[1] for e in ends}) == 2 and len({e[2] for e in ends}) == 2
