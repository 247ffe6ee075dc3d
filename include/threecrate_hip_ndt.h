/* threecrate_hip_ndt.h -- extension surface of libthreecrate_hip.so: NDT (Normal Distributions Transform) registration.
 *
 * The symbols live in the same shared library as those of threecrate_hip.h and use its status and context types;
 * tc_abi_version() is unchanged.  They are declared apart so that the main header and the other extension headers keep the sets
 * of names they have. */
#ifndef THREECRATE_HIP_NDT_H
#define THREECRATE_HIP_NDT_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ndt_registration ----
 * ndt_registration(&source, &target, initial_transform, &NdtConfig) -> Result<NdtResult> and ndt_registration_default
 * (threecrate-algorithms/src/ndt_registration.rs:188-269), the wheel's ndt_registration (threecrate-python/src/lib.rs:1165-1201).
 * The reference computes everything in f32.
 *
 * Voxel key (:61-67): (floor(x / res), floor(y / res), floor(z / res)) as i32 -- true division and floor, so a coordinate in
 *   (-res, 0) has key -1; keys are absolute, not taken from the cloud's minimum.
 * Voxel build (:70-111): the target's points grouped by key in input order; a voxel with fewer than min_points_per_voxel points is
 *   dropped; mean = (sum p) / n; cov = (sum (p - mean)(p - mean)^T) / n + 1e-4 I; inv_cov = cov^-1.
 * One evaluation at the pose T = (R, t) (:117-176), for every source point s: rs = R s, p = T s, key(p); a point whose key has
 *   no voxel is skipped; d = p - mean, c = inv_cov d, e = exp(-0.5 d.c); score += e; with J = [I | K],
 *   K = ((0, -rs.z, rs.y), (rs.z, 0, -rs.x), (-rs.y, rs.x, 0)) by columns: g += e J^T c, H += e J^T inv_cov J.
 * Loop (:216-252), for iter in 0..max_iterations: iterations = iter + 1; evaluate (score = this evaluation's); solve
 *   (H + 1e-6 I) delta = -g by LU with partial pivoting (failure: stop, not converged); |delta| > step_size: delta is scaled to that
 *   length; |delta| < epsilon: converged, stop, the pose is NOT updated; else T <- (Translation(delta[0..3]),
 *   from_euler_angles(roll = delta[3], pitch = delta[4], yaw = delta[5]) = Rz(yaw) Ry(pitch) Rx(roll)) o T.
 *   max_iterations == 0 returns the initial pose, score 0, 0 iterations, not converged.  The reported score belongs to the last
 *   pose that was EVALUATED, which after an update is not the returned one.
 *
 * Errors, in the reference's order (:194-209), TC_ALGORITHM: ns == 0 ("Source point cloud is empty"); nt < min_points_per_voxel
 *   ("Target point cloud has too few points for NDT voxel grid"); no voxel survives ("NDT voxel grid is empty — try a larger
 *   resolution or lower min_points_per_voxel").  Before them, TC_INVALID_DATA: a NULL context, cloud, config or result; a
 *   resolution that is not finite or <= 0 ("Resolution must be positive and finite").  TC_UNSUPPORTED: 2^32 - 16 points or more; a
 *   target whose key box needs more than 64 bits (the per-axis key ranges, each rounded up to a power of two).
 * Deviations:
 *   - non-finite points: the reference's saturating cast puts a NaN point into voxel (0, 0, 0) and poisons it.  Here a target point
 *     with a non-finite coordinate takes no part in the build, and a source point whose transformed position is non-finite scores
 *     nothing.
 *   - resolution: the reference divides by whatever it is given; here it is checked (above).
 *   - the voxel sums (mean, centred covariance, the 3 x 3 inverse), the 28 sums of an evaluation and the 6 x 6 solve are carried in
 *     f64 and rounded to f32 where the reference holds an f32 (the voxel records, the score, delta).  The per-point terms of g and H
 *     are f64 products of f32 values (the transformed point, R s, the record; exp is the f32 function): every point's H has rank 3,
 *     and f32 rounding of the terms leaves g a component outside H's range that the solve amplifies by up to 1e6 when few points
 *     hit.  The transform, the clamp, the convergence test and the pose update are f32 as in the reference.  The result is nearer
 *     to exact arithmetic than the reference's own.
 *   - the LU failure branch (a pivot that is exactly zero or not finite ends the loop with converged = 0) is kept, but the matrix is
 *     positive semi-definite plus 1e-6 I: for finite sums it cannot be reached, and no test reaches it.
 * The result has the same bits on every run: every sum has a fixed order, there are no floating-point atomics.
 *
 *   init     NULL (identity) or 7 floats: rotation i j k w, translation -- the pose of the ICP entry points.
 *   result   n_voxels: voxels of the map; n_hits: source points of the last evaluation that fell into one.
 *            A call that fails writes iterations = 0 and nothing else; without a context or a result it writes nothing at all.
 * The _device variants take device pointers for the clouds; init, config and result are host pointers in both. */
typedef struct tc_ndt_config {      /* NdtConfig, ndt_registration.rs:15-38 (defaults 1.0, 0.1, 35, 1e-4, 5) */
    float  resolution;
    float  step_size;
    size_t max_iterations;
    float  epsilon;
    size_t min_points_per_voxel;
} tc_ndt_config;

typedef struct tc_ndt_result {      /* NdtResult, ndt_registration.rs:42-51 */
    float  transformation[7];       /* Isometry3<f32>: qi qj qk qw tx ty tz */
    float  score;
    size_t iterations;
    int    converged;
    size_t n_voxels;
    size_t n_hits;
} tc_ndt_result;

tc_status tc_ndt_registration(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt, const float *init,
                              const tc_ndt_config *cfg, tc_ndt_result *result);
tc_status tc_ndt_registration_device(tc_context *ctx, const float *d_source, size_t ns, const float *d_target, size_t nt, const float *init,
                                     const tc_ndt_config *cfg, tc_ndt_result *result);

/* ---- the voxel map itself ----
 * The map ndt_registration builds from `target`: V voxels in ascending (kx, ky, kz) order.
 *   keys     V x 3 int32;  counts  V uint32 (points of the voxel);  mean  V x 3;  inv_cov  V x 6: xx xy xz yy yz zz.
 *   Any of the four may be NULL.  capacity: rows each non-NULL array has room for.  capacity < V writes *n_voxels and returns
 *   TC_INVALID_DATA ("capacity is smaller than the number of voxels") without writing an array.
 *   A target without a surviving voxel (nt == 0 included) is V = 0, not an error.
 * NULL context, n_voxels, or target with nt > 0: TC_INVALID_DATA; the resolution check and the limits as above.
 * The _device variant takes device pointers for target and the four arrays; n_voxels is a host pointer. */
tc_status tc_ndt_voxels(tc_context *ctx, const float *target, size_t nt, float resolution, size_t min_points_per_voxel, int32_t *keys,
                        uint32_t *counts, float *mean, float *inv_cov, size_t capacity, size_t *n_voxels);
tc_status tc_ndt_voxels_device(tc_context *ctx, const float *d_target, size_t nt, float resolution, size_t min_points_per_voxel, int32_t *d_keys,
                               uint32_t *d_counts, float *d_mean, float *d_inv_cov, size_t capacity, size_t *n_voxels);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_NDT_H */
