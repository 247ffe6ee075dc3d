/* threecrate_hip_shot.h -- companion surface: SHOT and USC descriptors with their local reference frame on the device
 * (extract_shot_features_with_normals, ShotConfig, ShotVariant: threecrate-algorithms/src/features.rs:287-645).  Per point a frame
 * x, y, z from its normal and the weighted covariance of its neighbourhood, then a histogram of the neighbours in that frame: SHOT counts
 * the cosine between the frame's z and each neighbour's normal in 2 radial x 2 elevation x 8 azimuth volumes of 11 bins (352 values), USC
 * counts the neighbours themselves in 8 azimuth x 4 elevation x 4 radial cells (128 values).
 *
 * The symbols live in a library of their own, libthreecrate_hip_shot.so, which is linked against libthreecrate_hip.so (it sits in the same
 * directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by tc_context_create serves both.
 * tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * ---- the rule, in the order of operations
 *    1. NEIGHBOURS of point i (features.rs:351-378), the rule of tc_extract_fpfh_features_with_normals: every j != i (by index) with
 *       d2 = (dx*dx + dy*dy) + dz*dz <= r*r, all in f32, one rounding per operation, no contraction (the BALL road).  With fewer than
 *       k_neighbors such points: the k_neighbors + 1 nearest by (d2, index), the query dropped, the first k_neighbors kept (the FALLBACK
 *       road).  A point with a coordinate that is not finite is INERT: an all-zero row, a zero frame, and it is nobody's neighbour.  The
 *       order of a list plays no part in any result.  An EMPTY list (a single point; k_neighbors = 0 and an empty ball) gives an all-zero
 *       row and a zero frame (:462, :531)
 *    2. dv = p_j - p_i and dist = sqrtf((x*x + y*y) + z*z) are the reference's f32 operations, so every decision on dist is the reference's
 *       bit for bit: dist < 1e-10f, dist > radius, dist <= radius * 0.5f, (dist / radius * 4.0f) as usize
 *    3. THE FRAME (:385-452) in f64, from those f32 values widened:
 *         z = normal / |normal| (the f64 norm), or (0, 0, 1) when the f32 norm sqrtf((nx*nx + ny*ny) + nz*nz) is not > 1e-10f (a NaN normal
 *             too); negated when 2 * #{j: z . dv_j >= 0} < len
 *         cov = sum over the list of max(radius - dist_j, 0) * dv_j dv_j^T (every neighbour, those beyond the radius with weight 0)
 *         e = the unit eigenvector of cov's largest eigenvalue (cyclic Jacobi, csrc/sym3_eigen.h), or (1, 0, 0) when cov is zero (its
 *             trace is not > 0); its sign made canonical: the component of largest magnitude is positive, on equal magnitudes the first;
 *             then negated when 2 * #{j: e . dv_j >= 0} < len
 *         x = e - z (z . e), normalised when its length is > 1e-10; else the same of (1, 0, 0); else of (0, 1, 0)
 *         y = z cross x
 *    4. HISTOGRAMS (:455-518, :524-585) over the neighbours with neither dist < 1e-10f nor dist > radius (a fallback neighbour beyond the
 *       radius votes in (3) and is in no bin), with lx = x . dv, ly = y . dv, lz = z . dv in f64, PI the f64 constant:
 *         azimuth   a = min((usize)((atan2(ly, lx) + PI) / (2 PI) * 8), 7)
 *         SHOT      r = dist <= radius * 0.5f ? 0 : 1;  e = lz < 0 ? 0 : 1;  volume = r * 16 + e * 8 + a;
 *                   bin = to_bin(clamp(z . normal_j, -1, 1), -1, 1, 11);  entry volume * 11 + bin
 *         USC       e = to_bin(clamp(lz / dist, -1, 1), -1, 1, 4);  r = min((usize)(dist / radius * 4.0f), 3);  entry a * 16 + e * 4 + r
 *       to_bin(v, lo, hi, n) = min((usize)((v - lo) / (hi - lo) * n), n - 1); every (usize) saturates: a NaN and a negative value give 0
 *    5. NORMALISATION in f64 on the integer counts, rounded once to f32: SHOT divides every volume's 11 counts by the volume's total,
 *       USC every count by the number of binned neighbours; then the row is divided by its L2 norm when that is > 1e-10
 * flags of a row: bits 0-1 the road (TC_SHOT_ROAD_BALL, _FALLBACK, _INERT); TC_SHOT_X_TIE: the vote on e was even, its sign is the
 * canonical one; TC_SHOT_ZERO_COV: cov was zero, e = (1, 0, 0); TC_SHOT_EMPTY: the list was empty.
 * DETERMINISM.  No floating-point atomics: the counts are integer LDS atomics, every f64 sum has a fixed order (a lane's neighbours in
 * the order it meets them, then a fixed shuffle tree).  Two calls, and the host and the _device variant, give identical bits.
 * Deviations from features.rs:
 *   - the frame, the local coordinates and the normalisation are f64 (the reference: f32 sums in list order, nalgebra's symmetric_eigen in f32)
 *   - the reference leaves the sign of e at an even vote to its eigen-solver; here it is the canonical sign, and TC_SHOT_X_TIE marks the row
 *   - a zero covariance takes (1, 0, 0) as e (the reference: whatever its solver returns for the zero matrix), marked TC_SHOT_ZERO_COV
 *   - the azimuth is taken with the canonical e and moved by exactly four sectors when the vote negates it (x and y both change sign: the
 *     angle moves by PI).  This is the formula on the final axes except where atan2 rounds across a sector edge
 *   - an inert point, as for FPFH; search_radius that is NaN or infinite is refused (the reference tests <= 0 only)
 *   - a normal with an infinite component gives a frame that is not finite; the row stays finite (every such value lands in bin 0) */
#ifndef THREECRATE_HIP_SHOT_H
#define THREECRATE_HIP_SHOT_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_SHOT_DIM 352   /* 2 radial x 2 elevation x 8 azimuth volumes x 11 bins */
#define TC_USC_DIM  128   /* 8 azimuth x 4 elevation x 4 radial */

#define TC_SHOT_VARIANT_SHOT 0
#define TC_SHOT_VARIANT_USC  1

#define TC_SHOT_ROAD_BALL     0u
#define TC_SHOT_ROAD_FALLBACK 1u
#define TC_SHOT_ROAD_INERT    2u
#define TC_SHOT_ROAD_MASK     3u
#define TC_SHOT_X_TIE         4u
#define TC_SHOT_ZERO_COV      8u
#define TC_SHOT_EMPTY         16u

typedef struct tc_shot_config {         /* ShotConfig */
    float  search_radius;
    size_t k_neighbors;
    int    variant;                     /* TC_SHOT_VARIANT_SHOT (ShotVariant::Standard) or TC_SHOT_VARIANT_USC (UniqueShapeContext) */
} tc_shot_config;

/* ShotConfig::default(): 0.2, 10, SHOT.  NULL is allowed. */
void tc_shot_config_default(tc_shot_config *cfg);

/* The row length of a variant: 352, 128, and 0 for anything else. */
size_t tc_shot_dim(int variant);

/* Descriptors of n points with normals (n x 6 floats: position, normal).
 *   out     n x tc_shot_dim(cfg->variant) floats
 *   lrf     n x 9 floats, or NULL: row i is x, y, z of point i's frame
 *   flags   n uint32, or NULL: the road taken and the two "reference undefined" bits
 * No output may overlap the input or another output.
 * Checks, in this order:
 *   1. a NULL context, cfg or out: TC_INVALID_DATA; normal_points may be NULL only with n == 0
 *   2. variant neither 0 nor 1: TC_INVALID_DATA
 *   3. search_radius not finite or not > 0: TC_INVALID_DATA ("search_radius must be positive")
 *   4. n == 0: TC_OK, nothing written
 *   5. n > 2^32 - 16 or k_neighbors + 1 > 2048: TC_UNSUPPORTED
 * A call that fails a check writes nothing.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for normal_points, out, lrf and
 * flags (cfg is a host pointer in both) and works on the context's stream.  Host waits of a call: the number of fallback points; the
 * final drain.  The call's scratch is released on return. */
tc_status tc_extract_shot_features_with_normals(tc_context *ctx, const float *normal_points, size_t n, const tc_shot_config *cfg, float *out,
                                                float *lrf, uint32_t *flags);
tc_status tc_extract_shot_features_with_normals_device(tc_context *ctx, const float *normal_points, size_t n, const tc_shot_config *cfg, float *out,
                                                       float *lrf, uint32_t *flags);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_SHOT_H */
