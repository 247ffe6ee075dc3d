/* threecrate_hip_global.h -- companion surface: the two device steps of global registration that the main library lacks,
 * descriptor matching and RANSAC over correspondences.
 *
 * The symbols live in a library of their own, libthreecrate_hip_global.so, which is linked against libthreecrate_hip.so (it
 * sits in the same directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by
 * tc_context_create serves both.  tc_abi_version() is unchanged.  A consumer links both libraries.
 * The pipeline of global_registration (threecrate-algorithms/src/global_registration.rs:185-333: normals, FPFH, matching,
 * RANSAC, optional point-to-point ICP) is composed by the callers of this header (the Python and the Rust facade) out of public
 * entry points: three of its five steps are exports of threecrate_hip.h. */
#ifndef THREECRATE_HIP_GLOBAL_H
#define THREECRATE_HIP_GLOBAL_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- tc_match_features: find_feature_correspondences (global_registration.rs:85-110) ----
 * For every source descriptor the nearest target descriptor by squared L2 distance.  Every operation is f32, in this order,
 * no FMA (fpfh_dist_sq, :87-89: a sequential sum):
 *   acc = 0;  for j in 0 .. dim:  t = s[j] - g[j];  acc = acc + t*t.
 * The winner of source i: start with target 0 as the incumbent, walk the targets in ascending order and replace the incumbent
 * iff d_new < d_best.  That is Rust's min_by with partial_cmp(..).unwrap_or(Equal) (:102-106): among equal distances the
 * LOWEST index wins; a NaN distance never replaces an incumbent; a NaN incumbent (target 0) is never replaced.
 *
 *   src_desc, tgt_desc  ns x dim and nt x dim floats, row i the descriptor of point i.
 *   dim                 must be TC_FPFH_DIM (the reference matches nothing else).
 *   match_index         ns entries: the winner of every source.
 *   match_dist          ns entries, or NULL: the winner's acc.  When it is a NaN (a NaN in the source row, or in target 0), its sign
 *                       and payload are unspecified: IEEE 754 leaves them to the implementation, and the device's differ from a CPU's.
 * The correspondences of the reference are the pairs (i, match_index[i]).
 *
 * Checks, in this order: a NULL context is TC_INVALID_DATA; dim != TC_FPFH_DIM is TC_UNSUPPORTED; ns == 0 is TC_OK and
 * writes nothing; a NULL src_desc, tgt_desc or match_index, or nt == 0, is TC_INVALID_DATA (the reference's filter_map drops
 * every source then; here there is no index to write); ns or nt >= 2^32 - 16 is TC_UNSUPPORTED.  A call that fails writes
 * nothing.
 * The _device variant takes device pointers (src_desc, tgt_desc, match_index, match_dist).  The result has the same bits on
 * every run. */
tc_status tc_match_features(tc_context *ctx, const float *src_desc, size_t ns, const float *tgt_desc, size_t nt, size_t dim,
                            uint32_t *match_index, float *match_dist);
tc_status tc_match_features_device(tc_context *ctx, const float *d_src_desc, size_t ns, const float *d_tgt_desc, size_t nt, size_t dim,
                                   uint32_t *d_match_index, float *d_match_dist);

/* ---- tc_ransac_correspondences: the RANSAC loop of global_registration_with_normals (:252-299) ----
 * with estimate_transform_svd (:112-145) and count_inliers (:147-163).  Pair p of the m correspondences is
 * (src_xyz[corr_src[p]], tgt_xyz[corr_tgt[p]]).
 *
 * Samples.  The reference draws from the thread's RNG and cannot be reproduced.  tc_ransac_correspondences draws from plane
 * segmentation's 64-bit LCG (threecrate_hip_segmentation.h):
 *   state0 = ((m << 32) ^ max_iters ^ 0x9E3779B97F4A7C15) ^ seed;
 *   draw:    state = state * 6364136223846793005 + 1442695040888963407 (mod 2^64);  r = state >> 32;
 * three draws r0, r1, r2 per iteration, mapped to three distinct correspondence indices the way :261-272 does:
 *   i0 = r0 % m;  i1 = r1 % (m - 1), i1 += (i1 >= i0);  i2 = r2 % (m - 2), i2 += (i2 >= min(i0, i1)), i2 += (i2 >= max(i0, i1)).
 * The triples are generated on the device (every iteration jumps the LCG ahead to its own three draws).
 * tc_ransac_correspondences_samples takes n_samples rows of three correspondence indices from the caller.  A row with an
 * index >= m or with two equal indices is a candidate without a model; it is never dereferenced.
 *
 * Model from three pairs.  The six points are widened to f64; in f64: the centroids c_s, c_t (sum of the three, divided by 3),
 *   H = sum ds * dt^T (ds = s - c_s, dt = t - c_t),  H = U S V^T,  R = V diag(1, 1, det(V U^T)) U^T,  t = c_t - R c_s.
 * R (row-major) and t are then rounded ONCE to f32 and stored: 12 floats, the candidate's transform.
 * A candidate has no model when one of its six points is non-finite, when an index of one of its pairs is out of range of
 * ns / nt, or when sigma_2(H) <= 1e-9 * sigma_1(H) (three collinear or coincident points on either side).
 *
 * Score: the number of pairs that are inliers under the STORED f32 R, t; f32, left to right, no FMA:
 *   x' = ((R00*x + R01*y) + R02*z) + tx, likewise y', z';  dx = x' - X, ..;  d2 = (dx*dx + dy*dy) + dz*dz;
 *   inlier iff d2 <= threshold*threshold (the product in f32, :155).
 * A pair with an index out of range, or whose d2 is NaN, is never an inlier.
 *
 * Winner: the sequential loop's (:291-298).  E = max(3, ceil(inlier_ratio * m)) with the product and the ceiling in f32 and the
 * conversion saturating (NaN -> 0) as :255; a strict `>` updates the best; the loop stops at the first iteration whose count
 * is a new best and >= E.  The best is below E until the loop stops, so the rule has a closed form, which is what runs:
 *   if any candidate reaches E, the FIRST such iteration wins: early_exit = 1, iterations_run = its index + 1;
 *   otherwise the lowest-indexed maximum wins: early_exit = 0, iterations_run = all of them.
 * A candidate without a model or with count 0 never wins.  When nothing wins the call still succeeds (the reference keeps
 * Isometry3::identity() and goes on to ICP): transform is the identity, inlier_count 0, best_iteration 0.
 *
 *   transform       12 floats: R row-major, then t, of the winner.
 *   result          inlier_count (the winner's score), iterations_run, best_iteration, early_exit,
 *                   inlier_ratio = (float)inlier_count / (float)m (:302-306).
 *   cand_transform  iterations x 12 floats, or NULL: every candidate's stored transform; twelve NaNs for a candidate without
 *                   a model.
 *   cand_count      iterations entries, or NULL: every candidate's score; 0 for a candidate without a model.  Candidates are
 *                   scored in chunks of 4096 in iteration order, and chunks behind the one that holds the exit are not
 *                   scored: their entries are 0.  Entries below iterations_run are always the scores.
 *   transform and result are host pointers in both variants.  A call that fails writes nothing.
 *
 * Errors, in this order.  TC_INVALID_DATA: a NULL context, transform or result; m < 3 ("Too few feature correspondences for
 * RANSAC (need >= 3)", :235-238); threshold <= 0 ("Threshold must be positive"; NaN passes, every test is then false and
 * nothing wins); max_iters == 0 / n_samples == 0 ("Max iterations must be positive"); a NULL src_xyz, tgt_xyz, corr_src,
 * corr_tgt or samples.  TC_UNSUPPORTED: m, ns or nt >= 2^32 - 16; more than TC_RANSAC_MAX_ITERS candidates (a candidate takes
 * 68 bytes of device memory for the duration of the call).
 * Deviations:
 *   - the reference estimates the model in f32 through nalgebra's iterative SVD and converts the rotation to a unit
 *     quaternion; here the solve is f64 and the rounded matrix itself is stored and applied.
 *   - on collinear or coincident triples the reference still returns whatever its SVD yields; here such a candidate has no
 *     model.
 * The result has the same bits on every run: the scores are integer sums.
 * The _device variants take device pointers (src_xyz, tgt_xyz, corr_src, corr_tgt, samples, cand_transform, cand_count). */
#define TC_RANSAC_MAX_ITERS ((size_t)1 << 20)

typedef struct tc_ransac_result {
    uint64_t inlier_count, iterations_run;
    uint32_t best_iteration;
    int32_t  early_exit;
    float    inlier_ratio;
} tc_ransac_result;

tc_status tc_ransac_correspondences(tc_context *ctx, const float *src_xyz, size_t ns, const float *tgt_xyz, size_t nt,
                                    const uint32_t *corr_src, const uint32_t *corr_tgt, size_t m, float threshold, float inlier_ratio,
                                    size_t max_iters, uint64_t seed, float *transform, tc_ransac_result *result, float *cand_transform,
                                    uint32_t *cand_count);
tc_status tc_ransac_correspondences_device(tc_context *ctx, const float *d_src_xyz, size_t ns, const float *d_tgt_xyz, size_t nt,
                                           const uint32_t *d_corr_src, const uint32_t *d_corr_tgt, size_t m, float threshold,
                                           float inlier_ratio, size_t max_iters, uint64_t seed, float *transform, tc_ransac_result *result,
                                           float *d_cand_transform, uint32_t *d_cand_count);
tc_status tc_ransac_correspondences_samples(tc_context *ctx, const float *src_xyz, size_t ns, const float *tgt_xyz, size_t nt,
                                            const uint32_t *corr_src, const uint32_t *corr_tgt, size_t m, float threshold,
                                            float inlier_ratio, const uint32_t *samples, size_t n_samples, float *transform,
                                            tc_ransac_result *result, float *cand_transform, uint32_t *cand_count);
tc_status tc_ransac_correspondences_samples_device(tc_context *ctx, const float *d_src_xyz, size_t ns, const float *d_tgt_xyz, size_t nt,
                                                   const uint32_t *d_corr_src, const uint32_t *d_corr_tgt, size_t m, float threshold,
                                                   float inlier_ratio, const uint32_t *d_samples, size_t n_samples, float *transform,
                                                   tc_ransac_result *result, float *d_cand_transform, uint32_t *d_cand_count);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_GLOBAL_H */
