/* threecrate_hip_ground.h -- companion surface: ground segmentation of an outdoor LiDAR frame on the device, a Patchwork++-style split
 * of a cloud into ground and non-ground points (patchwork_plus_plus and segment_ground, threecrate-algorithms/src/ground_segmentation.rs).
 * The plane around the sensor is cut into concentric zones, each zone into rings and sectors: the patches.  Every patch is an independent
 * small problem: seeds near its lowest points, a plane through them by PCA, the plane's inliers, the plane through those, a few times over
 * (R-GPF); then three tests of the last plane (upright, at the expected height, flat).  The inliers of a patch that passes are ground.
 *
 * The symbols live in a library of their own, libthreecrate_hip_ground.so, which is linked against libthreecrate_hip.so (it sits in the same
 * directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by tc_context_create serves both.
 * tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * ---- the contract, in the order of operations
 *    1. BUCKETING, per point, in f32, one rounding per operation, no contraction; sqrtf and / correctly rounded:
 *         r = sqrtf(x*x + y*y).  r > max_range, or no zone z with zone_radii[z] <= r < zone_radii[z+1]: OUT OF RANGE, label 0, in no patch
 *         ring_width = (zone_radii[z+1] - zone_radii[z]) / (float)num_rings[z]
 *         ring = min((uint)((r - zone_radii[z]) / ring_width), num_rings[z] - 1)           (a quotient that is NaN gives ring 0)
 *         theta = atan2f(y, x); theta += 2.0f * PI when theta < 0
 *         sector = min((uint)(theta / (2.0f * PI / (float)num_sectors[z])), num_sectors[z] - 1)
 *       atan2f(y, x) is the f64 atan2 of the two floats, rounded once to f32.  The patches are numbered in (zone, ring, sector) order
 *    2. SEEDS of a patch of `count` points.  count == 0: TC_GROUND_PATCH_EMPTY.  count < min_points_per_patch: _TOO_FEW_POINTS.  Else
 *       z_min_mean = the mean of the min(num_seed_points, count) smallest z of the patch, cutoff = z_min_mean + seed_selection_threshold,
 *       and the seed set is every point of the patch with z <= cutoff.  Fewer than 3 seeds: _TOO_FEW_SEEDS.  The set does not depend on
 *       how equal z are ordered
 *    3. R-GPF, at most num_iterations times (num_iterations == 0: _NO_ITERATION).  PCA of the current set: its mean, its covariance
 *       divided by the count, the unit eigenvector of the smallest eigenvalue as the normal, negated when its z is negative;
 *       d = -normal . mean.  The new set is every point p of the WHOLE patch with |normal . p + d| <= dist_threshold.  Fewer than 3:
 *       _TOO_FEW_INLIERS.  The loop ends early when the new set has as many members as the current one (the counts are compared, not
 *       the sets, as in the reference).  The new set is the next current set
 *    4. VALIDATION of the last plane and its inlier set, the first test that holds gives the status:
 *         _NOT_UPRIGHT   |normal.z| < uprightness_threshold
 *         _ELEVATION     |mean_z(inliers) + sensor_height| > elevation_threshold
 *         _NOT_FLAT      flatness = l0 / (l0 + l1 + l2) of the inliers' covariance (eigenvalues ascending) > flatness_threshold; only when
 *                        the sum is > 0 (otherwise flatness is reported as 0 and the test does not hold)
 *         _GROUND        otherwise: the inliers get label 1
 *    5. OUTPUTS: the labels; the indices of the ground points and of all other points, each in ascending input order; *n_ground; one
 *       tc_ground_patch per patch of the configuration, empty ones included.  n_inliers, normal, d, mean_z and flatness of a record are
 *       those of the last plane and its inliers for the four statuses of (4) and zero for every other
 * ARITHMETIC.  Every sum of (2) to (4) (the seed mean, the means, the second moments, mean z), the eigen-problem (cyclic Jacobi,
 * csrc/sym3_eigen.h) and the point-to-plane distance of (3) are f64.  Their inputs are the f32 coordinates widened to f64 and taken
 * relative to a pivot per patch, the patch's point of smallest z (of several, the one of lowest index; -0.0 sorts below 0.0): the sums are the
 * count, the three first and the six second raw moments about the pivot, cov_ab = S_ab / count - mean_a mean_b; the cutoff of (2) and
 * the distance of (3) are compared in f64, in the pivot's frame, ((nx qx + ny qy) + nz qz) + d'.  f32 returns at the three comparisons
 * of (4): normal.z, mean_z and flatness are rounded to f32 and compared with the f32 thresholds (mean_z + sensor_height is an f32 sum);
 * normal, d, mean_z and flatness of a patch record are those rounded values, in the cloud's frame.  The order of every reduction is
 * fixed (a lane's points in ascending position, then the lanes of a wave, then the waves of a block): two calls give identical bits.
 * No floating-point atomics.
 * Deviations from ground_segmentation.rs:
 *   - the f64 sums above.  The reference adds up f32 values point after point, an order a parallel reduction cannot keep; in f32 the
 *     plane then moves by enough to flip points near dist_threshold, and the flips cascade through the iterations
 *   - a point with a coordinate that is not finite is out of range: label 0, in no patch.  The reference panics on a NaN z inside its sort
 *   - the result does not depend on a thread count (the reference's rayon pool)
 *   - the configuration is a fixed-size struct: at most TC_GROUND_MAX_ZONES zones, every zone with at least one ring and one sector
 *     (the reference would underflow num_rings - 1) */
#ifndef THREECRATE_HIP_GROUND_H
#define THREECRATE_HIP_GROUND_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_GROUND_MAX_ZONES 8

#define TC_GROUND_PATCH_EMPTY           0u      /* no point */
#define TC_GROUND_PATCH_TOO_FEW_POINTS  1u      /* fewer than min_points_per_patch */
#define TC_GROUND_PATCH_TOO_FEW_SEEDS   2u      /* fewer than 3 points up to the cutoff */
#define TC_GROUND_PATCH_TOO_FEW_INLIERS 3u      /* a plane kept fewer than 3 points */
#define TC_GROUND_PATCH_NO_ITERATION    4u      /* num_iterations == 0: no plane */
#define TC_GROUND_PATCH_NOT_UPRIGHT     5u
#define TC_GROUND_PATCH_ELEVATION       6u
#define TC_GROUND_PATCH_NOT_FLAT        7u
#define TC_GROUND_PATCH_GROUND          8u

typedef struct tc_ground_config {       /* PatchworkConfig with its vectors at a fixed size */
    float    sensor_height;
    uint32_t n_zones;                   /* 1 .. TC_GROUND_MAX_ZONES */
    float    zone_radii[9];             /* TC_GROUND_MAX_ZONES + 1; the first n_zones + 1 are read, strictly increasing */
    uint32_t num_rings[8];              /* TC_GROUND_MAX_ZONES; the first n_zones are read, each >= 1 */
    uint32_t num_sectors[8];            /* the same */
    float    max_range;
    uint32_t min_points_per_patch;
    uint32_t num_seed_points;           /* >= 1 */
    float    seed_selection_threshold;
    float    dist_threshold;            /* > 0 */
    uint32_t num_iterations;
    float    uprightness_threshold;     /* in (0, 1] */
    float    flatness_threshold;
    float    elevation_threshold;
} tc_ground_config;

typedef struct tc_ground_patch {
    uint32_t count;                     /* points of the patch */
    uint32_t n_inliers;                 /* of the last plane */
    uint32_t status;                    /* TC_GROUND_PATCH_* */
    float    normal[3];
    float    d;
    float    mean_z;
    float    flatness;
} tc_ground_patch;

/* PatchworkConfig::default() with the given sensor height: 4 zones with radii 0, 2.7, 12.3625, 22.025, 80; 2, 4, 4, 4 rings and 16, 32, 54,
 * 32 sectors (504 patches); max_range 80, 10 points per patch, 20 seed points, 0.5, 0.125, 3 iterations, 0.707, 0.05, 1.0.  NULL is allowed. */
void tc_ground_config_default(float sensor_height, tc_ground_config *cfg);

/* The number of patches, the sum of num_rings[z] * num_sectors[z] over the zones; 0 for a NULL config and for one that fails check (2) or
 * (3) below (a count above 65 536 is returned as it is). */
size_t tc_ground_patch_count(const tc_ground_config *cfg);

/* Segment n points (n x 3 floats).
 *   out_labels            n bytes, 1 = ground
 *   out_ground_index      room for n uint32, or NULL: the ground points' indices, ascending; *n_ground of them are written
 *   out_nonground_index   room for n uint32, or NULL: all other indices, ascending; n - *n_ground of them are written
 *   out_patches           room for tc_ground_patch_count(cfg) records, or NULL
 *   n_ground              the number of ground points
 * No output may overlap the input or another output.
 * Checks, in this order:
 *   1. a NULL context, cfg, out_labels or n_ground: TC_INVALID_DATA; points may be NULL only with n == 0
 *   2. the reference's validate_config, in its order and with its messages: n_zones == 0 ("num_rings_per_zone must be non-empty");
 *      zone_radii not strictly increasing, which a NaN radius fails ("zone_radii must be strictly increasing"); dist_threshold <= 0
 *      ("dist_threshold must be positive"); num_seed_points == 0 ("num_seed_points must be at least 1"); uprightness_threshold outside
 *      (0, 1] ("uprightness_threshold must be in (0, 1]"): TC_INVALID_DATA.  With n_zones above TC_GROUND_MAX_ZONES the first
 *      TC_GROUND_MAX_ZONES + 1 radii are the ones looked at
 *   3. n_zones > TC_GROUND_MAX_ZONES: TC_INVALID_DATA; then a zone with 0 rings or 0 sectors: TC_INVALID_DATA
 *   4. more than 65 536 patches: TC_UNSUPPORTED; then n >= 2^32 - 16: TC_UNSUPPORTED
 *   5. n == 0: TC_OK with *n_ground = 0, every patch TC_GROUND_PATCH_EMPTY, and no device work (the host variant writes the records; the
 *      _device variant clears them on the stream)
 * A call that fails a check writes nothing.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for points, out_labels, the two
 * index lists and out_patches (cfg and n_ground are host pointers in both) and works on the context's stream.  Host waits of a call:
 * the ground count; the final drain.  Nothing else waits: the number of patches is known from the configuration, and the list of patches
 * to fit is made and consumed on the device.  The call's scratch is released on return. */
tc_status tc_segment_ground(tc_context *ctx, const float *points, size_t n, const tc_ground_config *cfg, uint8_t *out_labels,
                            uint32_t *out_ground_index, uint32_t *out_nonground_index, tc_ground_patch *out_patches, size_t *n_ground);
tc_status tc_segment_ground_device(tc_context *ctx, const float *points, size_t n, const tc_ground_config *cfg, uint8_t *out_labels,
                                   uint32_t *out_ground_index, uint32_t *out_nonground_index, tc_ground_patch *out_patches, size_t *n_ground);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_GROUND_H */
