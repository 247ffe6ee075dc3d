/* threecrate_hip_segmentation.h -- extension surface of libthreecrate_hip.so: RANSAC plane segmentation.
 *
 * The symbols live in the same shared library as those of threecrate_hip.h and use its status and context types;
 * tc_abi_version() is unchanged.  They are declared apart so that the main header and the filters header keep the sets of
 * names they have. */
#ifndef THREECRATE_HIP_SEGMENTATION_H
#define THREECRATE_HIP_SEGMENTATION_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- segment_plane ----
 * segment_plane(&PointCloud<Point3f>, threshold, max_iters) -> Result<PlaneSegmentationResult>, segment_plane_ransac and
 * plane_segmentation_ransac (threecrate-algorithms/src/segmentation.rs:28-91, :117-180, :297-324), the wheel's segment_plane
 * (threecrate-python/src/lib.rs:1251-1277) and the facade's gpu_segment_plane / gpu_segment_plane_ransac
 * (threecrate-gpu/src/segmentation.rs:304-452, :813-831).  Every operation is f32, left to right, no FMA.
 *
 * Model from a triple (i0, i1, i2) of point indices (:28-47):
 *   v1 = p[i1] - p[i0], v2 = p[i2] - p[i0];
 *   c = (v1.y*v2.z - v1.z*v2.y, v1.z*v2.x - v1.x*v2.z, v1.x*v2.y - v1.y*v2.x);
 *   len = sqrt(c.x*c.x + c.y*c.y + c.z*c.z);  len < 1e-8 -> no model (collinear or repeated points);
 *   (a, b, c) = c / len, component by component;  d = -(a*p0.x + b*p0.y + c*p0.z).
 * Distance of a point (:59-73): m = sqrt(a*a + b*b + c*c) of the STORED coefficients (close to 1, not exactly 1);
 *   m < 1e-8 -> +inf, else |a*x + b*y + c*z + d| / m.  A point is an inlier when distance <= threshold.
 * A candidate's score is its inlier count over all n points; the returned inliers pass the same test, so *n_inliers is the
 * winner's score.  The winner is the candidate with the greatest score and, among equal scores, the LOWEST iteration index
 * (:162, a strict `>` in a sequential loop).  A candidate without a model or with score 0 never wins; when none wins the call
 * returns TC_ALGORITHM, "Failed to find valid plane model".
 * Non-finite points get no special case: a NaN distance is not <= threshold, so such a point is never an inlier, and a model
 * built from one has NaN coefficients and scores 0.
 *
 *   coefficients    4 floats: a, b, c, d of the winner.
 *   inlier_index    capacity n, or NULL: the winner's inliers, ascending original indices.  NULL skips that pass.
 *   n_inliers       the winner's score.
 *   best_iteration  or NULL: the winner's iteration (row of `samples`).
 *   coefficients, n_inliers and best_iteration are host pointers in both variants.  A call that fails leaves *n_inliers 0
 *   and writes nothing else; without a context, coefficients or n_inliers it writes nothing at all.
 *
 * tc_segment_plane draws its triples like the facade (threecrate-gpu/src/segmentation.rs:979-1011), which is deterministic
 * (the CPU path draws from the thread's RNG and cannot be reproduced): a 64-bit LCG,
 *   state0 = ((n << 32) ^ max_iters ^ 0x9E3779B97F4A7C15) ^ seed;
 *   draw:    state = state * 6364136223846793005 + 1442695040888963407 (mod 2^64); index = (state >> 32) % n;
 * three draws per iteration.  When two of them are equal the iteration's triple is the closed form of :988-998:
 *   a = it % n, b = (it*37 + 1) % n, c = (it*101 + 2) % n, then b = (b + 1) % n while b == a, c = (c + 1) % n while
 *   c == a or c == b.
 * seed == 0 is the facade's own sequence.  The triples are generated on the device (every iteration jumps the LCG ahead to
 * its own three draws): no sample list crosses the bus.
 * tc_segment_plane_samples takes the triples from the caller: n_samples rows of three indices.  A row with an index >= n is
 * a candidate without a model; it is never dereferenced.
 *
 * Errors, in the reference's order (:122-136, gpu :863-883), TC_INVALID_DATA: n < 3 ("Need at least 3 points for plane
 * segmentation"), threshold <= 0 ("Threshold must be positive"; NaN passes as it does in Rust, every test is then false and
 * the call ends in TC_ALGORITHM), max_iters == 0 / n_samples == 0 ("Max iterations must be positive").  A NULL context,
 * coefficients, n_inliers, or samples is TC_INVALID_DATA.
 * Limits, TC_UNSUPPORTED: n >= 2^32 - 16; max_iters / n_samples > 2^20 (TC_SEGMENT_PLANE_MAX_ITERS; a candidate takes 28
 * bytes of device memory for the duration of the call).
 * Deviations:
 *   - the facade picks its winner with max_by_key, which returns the LAST of equal scores; this backend returns the first, as
 *     the CPU path does.
 *   - the facade's score shader compares |a*x + b*y + c*z + d| with the threshold without dividing by m; this backend divides
 *     (the CPU path's distance) in the score and in the inlier list alike.
 *   - the facade's min_inliers check belongs to the callers of this header (the Python and Rust facades).
 * The result has the same bits on every run: the scores are integer sums.
 * The _device variants take device pointers (xyz, samples, inlier_index). */
#define TC_SEGMENT_PLANE_MAX_ITERS ((size_t)1 << 20)

tc_status tc_segment_plane(tc_context *ctx, const float *xyz, size_t n, float threshold, size_t max_iters, uint64_t seed,
                           float *coefficients, uint32_t *inlier_index, size_t *n_inliers, uint32_t *best_iteration);
tc_status tc_segment_plane_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, size_t max_iters, uint64_t seed,
                                  float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers, uint32_t *best_iteration);
tc_status tc_segment_plane_samples(tc_context *ctx, const float *xyz, size_t n, float threshold, const uint32_t *samples,
                                   size_t n_samples, float *coefficients, uint32_t *inlier_index, size_t *n_inliers,
                                   uint32_t *best_iteration);
tc_status tc_segment_plane_samples_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, const uint32_t *d_samples,
                                          size_t n_samples, float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers,
                                          uint32_t *best_iteration);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_SEGMENTATION_H */
