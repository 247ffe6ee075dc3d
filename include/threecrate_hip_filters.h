/* threecrate_hip_filters.h -- extension surface of libthreecrate_hip.so: the outlier removal filters.
 *
 * The symbols live in the same shared library as those of threecrate_hip.h and use its status and context types;
 * tc_abi_version() is unchanged.  They are declared apart so that the main header keeps the set of names it has. */
#ifndef THREECRATE_HIP_FILTERS_H
#define THREECRATE_HIP_FILTERS_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- statistical_outlier_removal ----
 * statistical_outlier_removal(&PointCloud<Point3f>, k_neighbors, std_dev_multiplier) -> Result<PointCloud<Point3f>> and
 * statistical_outlier_removal_with_threshold(&PointCloud<Point3f>, k_neighbors, threshold)
 * (threecrate-algorithms/src/filtering.rs:249-395), the wheel's remove_statistical_outliers (threecrate-python/src/lib.rs:789-803)
 * and the facade gpu_remove_statistical_outliers (threecrate-gpu/src/filtering.rs:882-893).
 * Per point: the k_neighbors + 1 nearest (:279), d2 = dx*dx + dy*dy + dz*dz in f32, left to right, no FMA; the entries equal to
 * the point are dropped (:287) and the distances sqrt(d2) of the rest are summed in ascending order in f32 and divided by
 * their count (:295); no entry left -> 0 (:291-293).  Then threshold = mean + std_dev_multiplier * sqrt(population variance) of
 * those means (:300-309), and the points with mean <= threshold are kept (:316).
 *   out_xyz        capacity n x 3, or NULL: the kept points in input order (:312-318).
 *   kept_index     capacity n, or NULL: their original indices, ascending.
 *   mean_distance  n entries, or NULL: every point's mean distance, in input order.
 *   n_out, threshold_used   host pointers in both variants; threshold_used may be NULL.
 * Errors, in the reference's order (:254-268, :340-354): an empty cloud -> TC_OK with *n_out = 0 before any other check;
 * TC_INVALID_DATA for k_neighbors == 0 ("k_neighbors must be greater than 0"), std_dev_multiplier <= 0 ("std_dev_multiplier
 * must be positive"), threshold <= 0 ("threshold must be positive").  NaN parameters pass these checks as they do in Rust; a NaN
 * multiplier or threshold then keeps nothing (`x <= NaN` is false).
 * Limits, TC_UNSUPPORTED: k_neighbors > 2047 (the k + 1 nearest come from the 2048-entry selection); n >= 2^32 - 16.
 * Deviations:
 *   - a point with a non-finite coordinate is inert: never a neighbour, never kept, not part of the statistics, whose divisor is
 *     the count of finite points; its mean_distance is NaN (the reference's kd-tree returns whatever its NaN comparisons visit).
 *   - "skip self" (:287, a comparison by value) is d2 == 0: the two differ only where the squares of a non-zero offset underflow
 *     to zero.
 *   - the global mean and variance of tc_statistical_outlier_removal are summed in f64 in a fixed order, not in the reference's
 *     sequential f32; the threshold is rounded to f32 once.  Bit-identical from run to run (no float atomics).  The
 *     _with_threshold variant has no such difference.
 * The _device variants take device pointers (xyz, out_xyz, kept_index, mean_distance). */
tc_status tc_statistical_outlier_removal(tc_context *ctx, const float *xyz, size_t n, size_t k_neighbors, float std_dev_multiplier,
                                         float *out_xyz, uint32_t *kept_index, float *mean_distance, size_t *n_out, float *threshold_used);
tc_status tc_statistical_outlier_removal_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k_neighbors, float std_dev_multiplier,
                                                float *d_out_xyz, uint32_t *d_kept_index, float *d_mean_distance, size_t *n_out,
                                                float *threshold_used);
tc_status tc_statistical_outlier_removal_with_threshold(tc_context *ctx, const float *xyz, size_t n, size_t k_neighbors, float threshold,
                                                        float *out_xyz, uint32_t *kept_index, float *mean_distance, size_t *n_out);
tc_status tc_statistical_outlier_removal_with_threshold_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k_neighbors,
                                                               float threshold, float *d_out_xyz, uint32_t *d_kept_index,
                                                               float *d_mean_distance, size_t *n_out);

/* ---- radius_outlier_removal ----
 * radius_outlier_removal(&PointCloud<Point3f>, radius, min_neighbors) -> Result<PointCloud<Point3f>>
 * (threecrate-algorithms/src/filtering.rs:167-213), the wheel's remove_radius_outliers (threecrate-python/src/lib.rs:805-817) and
 * the facade gpu_radius_outlier_removal (threecrate-gpu/src/filtering.rs:895-905).
 * A point is kept when at least min_neighbors OTHER points lie within the radius: the count of d2 <= radius * radius (f32, as
 * above; nearest_neighbor.rs:259, 271) with the point itself included, minus one (:199), compared in 64 bits (:208) -- a huge
 * min_neighbors keeps nothing.  No cap on the neighbours of a point.  out_xyz / kept_index as above.
 * Errors, in the reference's order (:172-186): an empty cloud -> TC_OK with *n_out = 0; TC_INVALID_DATA for radius <= 0 ("radius
 * must be positive"), min_neighbors == 0 ("min_neighbors must be greater than 0").  A NaN radius passes and keeps nothing.  When
 * radius * radius is not finite, every finite point has (finite points - 1) neighbours.
 * Limits, TC_UNSUPPORTED: n >= 2^32 - 16.
 * Deviation: a point with a non-finite coordinate is inert -- never a neighbour, never kept. */
tc_status tc_radius_outlier_removal(tc_context *ctx, const float *xyz, size_t n, float radius, size_t min_neighbors, float *out_xyz,
                                    uint32_t *kept_index, size_t *n_out);
tc_status tc_radius_outlier_removal_device(tc_context *ctx, const float *d_xyz, size_t n, float radius, size_t min_neighbors,
                                           float *d_out_xyz, uint32_t *d_kept_index, size_t *n_out);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_FILTERS_H */
