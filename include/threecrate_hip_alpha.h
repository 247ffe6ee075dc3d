/* threecrate_hip_alpha.h -- companion surface: alpha-shape surface reconstruction on the device, a point cloud to a triangle mesh
 * (alpha_shape_reconstruction and AlphaComplex::extract_surface, threecrate-reconstruction/src/alpha_shape.rs), what the wheel's
 * alpha_shape_reconstruct(cloud, alpha) runs: the "quality" road in BoundaryOnly mode.  That road is no Delaunay filtration.  It is a local
 * enumeration: the points inside a ball around each point, all index-ordered triples of them, a geometric test per triple, then a count of
 * the candidate triangles on every edge.  The reference stops after 50 000 candidates in index order, so on a cloud of more than a few
 * hundred points its mesh covers the lowest-indexed corner of the cloud only; here that cap is a parameter.
 *
 * The symbols live in a library of their own, libthreecrate_hip_alpha.so, which is linked against libthreecrate_hip.so (it sits in the same
 * directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by tc_context_create serves both.
 * tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * ---- the contract, in the order of operations.  All arithmetic is f32, one rounding per operation, no contraction; sqrtf and / are
 * ---- correctly rounded.  |v|^2 means (vx*vx + vy*vy) + vz*vz, |v| = sqrtf(|v|^2).  The outputs are vertex indices: bit for bit, in order
 *    1. NEIGHBOURS of i: every j != i with |p_i - p_j| <= alpha.  The test is on the rooted length, as in the reference.  Only j > i can
 *       form a triangle.  Duplicates of p_i are neighbours
 *    2. TRIPLES: for every i in ascending order, every pair j < k of i's neighbours with i < j forms the triple (i, j, k), in lexicographic
 *       order of (i, j, k).  j and k need not be neighbours of each other.  The result depends on the order of the points, by design
 *    3. a triple is a CANDIDATE when all of the following hold (comparisons as written: a NaN fails them)
 *         a2 = |p_j - p_i|^2, b2 = |p_k - p_j|^2, c2 = |p_i - p_k|^2 are all >= 1e-20f
 *         x = (p_j - p_i) x (p_k - p_i), each component two products and one difference; X = |x|^2; X * 0.25f >= 1e-20f
 *         R2 = ((a2*b2)*c2) / (16.0f * (X*0.25f)) is not +infinity (the reference's circumradius_sq == INFINITY: an overflow is dropped
 *              like the guards above)
 *         area = sqrtf(X) * 0.5f with area >= min_triangle_area
 *         per = (sqrtf(a2) + sqrtf(b2)) + sqrtf(c2) with per >= 1e-10f
 *         (4.0f*area) / (per*per) > 0.01f
 *    4. CAP: with max_triangles > 0 only the first max_triangles candidates in the order of (2) exist for what follows.  The reference
 *       uses 50 000.  0 means no cap
 *    5. BOUNDARY: every remaining candidate gives the edges (i,j), (j,k), (i,k), with key lo << 32 | hi.  An edge's multiplicity is the
 *       number of remaining candidates on it.  A candidate is a BOUNDARY candidate when one of its three edges has multiplicity 1
 *    6. FACES: the remaining candidates with R2 <= alpha*alpha and area >= min_triangle_area; in TC_ALPHA_BOUNDARY_ONLY they must also be
 *       boundary candidates, TC_ALPHA_FULL has no further condition.  They are written as uint32 triples (i, j, k) in the order of (2).
 *       The mesh's vertices are the n input points, unchanged and all of them: the entry points do not copy them
 *    7. no candidate after (4): TC_ALGORITHM ("No candidate triangles generated"); no face after (6): TC_ALGORITHM ("No triangles
 *       survived alpha filtering")
 * Deviations from alpha_shape.rs:
 *   - a coordinate that is not finite, and an alpha that is NaN, infinite or <= 0, are TC_INVALID_DATA; the reference carries them
 *   - fast_mode and AlphaMode::Adaptive are out of scope
 *   - the cap is a parameter
 *   - the reference's HashMap iteration order plays no part in its result, so nothing is lost by grouping the edges with a sort */
#ifndef THREECRATE_HIP_ALPHA_H
#define THREECRATE_HIP_ALPHA_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_ALPHA_BOUNDARY_ONLY 0u
#define TC_ALPHA_FULL          1u

typedef struct tc_alpha_config {        /* AlphaComplexConfig without fast_mode, and the cap of generate_triangles_quality */
    float    alpha;                     /* > 0, finite */
    uint32_t mode;                      /* TC_ALPHA_BOUNDARY_ONLY | TC_ALPHA_FULL */
    float    min_triangle_area;         /* >= 0 */
    uint32_t max_triangles;             /* 0 = no cap */
} tc_alpha_config;

typedef struct tc_alpha_stats {         /* AlphaComplexStats' counts */
    uint64_t candidates;                /* after the cap (4) */
    uint64_t boundary_candidates;       /* of those, (5) */
    uint64_t faces;                     /* (6) */
    uint32_t capped;                    /* 1 when the cap cut candidates off */
} tc_alpha_stats;

/* alpha as given, TC_ALPHA_BOUNDARY_ONLY, 1e-8f, 50000: alpha_shape_reconstruction(cloud, alpha).  NULL is allowed. */
void tc_alpha_config_default(float alpha, tc_alpha_config *cfg);

/* Reconstruct the alpha shape of n points (n x 3 floats).
 *   out_faces   room for cap_faces x 3 uint32, or NULL
 *   stats       the counts; written by every call that returns TC_OK and by one that fails check (8)
 * The number of faces is not known in advance.  With out_faces NULL the call gives the counts alone (cap_faces is not read); otherwise
 * cap_faces below stats->faces is TC_INVALID_DATA and nothing but the counts is written (as tc_marching_cubes answers).  No output may
 * overlap the input.
 * Checks, in this order:
 *   1. a NULL context, points, cfg or stats: TC_INVALID_DATA
 *   2. n == 0: TC_INVALID_DATA ("Point cloud is empty"); then n < 3: TC_INVALID_DATA ("Need at least 3 points for triangulation")
 *   3. mode > 1: TC_INVALID_DATA
 *   4. alpha NaN, infinite or <= 0: TC_INVALID_DATA; then min_triangle_area negative or NaN: TC_INVALID_DATA
 *   5. n >= 2^32 - 16: TC_UNSUPPORTED
 *   6. a coordinate that is not finite: TC_INVALID_DATA.  Found on the device
 *   7. a neighbour-pair total (the j > i of (1), over all i) or a candidate total before the cap of 2^32 - 16 or more, or three times the
 *      remaining candidates at 2^32 - 16 or more: TC_UNSUPPORTED.  The scratch is indexed in 32 bits; this is known after the count
 *      passes, before anything of that size is allocated
 *   8. the capacity
 * then the two TC_ALGORITHM results of (7) of the contract, which precede check (8).  A call that fails writes nothing, except that from
 * check (8) on the counts are written.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for points and out_faces (cfg and
 * stats are host pointers in both) and works on the context's stream.  Host waits of a call, besides those of the index build: the
 * finite flag together with the neighbour-pair total; the candidate total; the face count; and, when faces are written, a final drain.
 * The call's scratch is released on return. */
tc_status tc_alpha_shape(tc_context *ctx, const float *points, size_t n, const tc_alpha_config *cfg, uint32_t *out_faces, size_t cap_faces,
                         tc_alpha_stats *stats);
tc_status tc_alpha_shape_device(tc_context *ctx, const float *points, size_t n, const tc_alpha_config *cfg, uint32_t *out_faces,
                                size_t cap_faces, tc_alpha_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_ALPHA_H */
