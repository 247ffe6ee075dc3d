/* threecrate_hip_qem.h -- companion surface: simplify a triangle mesh on the device by quadric-error edge collapse
 * (QuadricErrorSimplifier, threecrate-simplification/src/quadric_error.rs; Garland & Heckbert 1997), what the wheel's
 * simplify_mesh(mesh, reduction_ratio) runs.  The reference's collapse has no flip test and no link condition: it remaps one vertex, drops
 * the faces that became degenerate and adds two quadrics, and it rebuilds its queue every 100 collapses.  Here that runs as ROUNDS: in each
 * round every edge that is the cheapest at both of its ends collapses at once (a matching), cheapest first, up to the face budget.
 *
 * The symbols live in a library of their own, libthreecrate_hip_qem.so, which is linked against libthreecrate_hip.so (it sits in the same
 * directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by tc_context_create serves both.
 * tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * In scope: max_edge_length, preserve_boundary, the reduction ratio.  feature_angle_threshold is a field of the reference's struct that
 * quadric_error.rs never reads: it is not in tc_qem_config.  No normals or colours: the reference's rebuild_mesh drops them.
 *
 * ---- the contract, in the order of operations; every result is bit for bit; one rounding per operation, no contraction ----
 *    1. target = (size_t)((1.0f - ratio) * (float)n_faces): the product in f32, truncated (quadric_error.rs:428)
 *    2. input faces: a face that repeats an index is dropped before anything else and contributes no quadric; alive = the number of
 *       faces left.  The faces keep their input order through everything that follows
 *    3. plane of a face, f32: e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 (each component two products and one difference),
 *       len = sqrtf((nx*nx + ny*ny) + nz*nz), n = n / len per component.  If a component of n is not finite the plane is (0, 0, 1, 0);
 *       otherwise d = -((nx*v0x + ny*v0y) + nz*v0z).  (a, b, c, d) = (nx, ny, nz, d) widened to f64
 *    4. quadric of a plane: the ten f64 products aa ab ac ad bb bc bd cc cd dd (the matrix is symmetric: both triangles hold the same
 *       bits).  Quadric of a vertex: per product an f64 fold from +0.0 over its incident faces, in ascending face index
 *    5. a round, repeated while alive > target:
 *       a. edges: every alive face gives (min, max) of (a,b), (b,c), (c,a); key = lo << 32 | hi; the unique edges in ascending key
 *          order, each with its multiplicity c (the number of face sides on it)
 *       b. boundary (preserve_boundary only): a vertex is a boundary vertex when it ends an edge with c == 1; recomputed every round
 *       c. a unique edge is a CANDIDATE unless an end is a boundary vertex (preserve_boundary only), or max_edge_length > 0 and its f32
 *          length sqrtf((dx*dx + dy*dy) + dz*dz), d = p_lo - p_hi, exceeds it, or its cost (e) is NaN
 *       d. position: Q = Q_lo + Q_hi element by element (f64); with q_ij the elements of Q, a_ij = q_ij for i, j < 3, b = (q03, q13, q23):
 *              c00 = a11*a22 - a12*a12   c01 = a02*a12 - a01*a22   c02 = a01*a12 - a02*a11
 *              c11 = a00*a22 - a02*a02   c12 = a01*a02 - a00*a12   c22 = a00*a11 - a01*a01
 *              det = (a00*c00 + a01*c01) + a02*c02
 *              x = -(((c00*b0 + c01*b1) + c02*b2) / det)
 *              y = -(((c01*b0 + c11*b1) + c12*b2) / det)
 *              z = -(((c02*b0 + c12*b1) + c22*b2) / det)
 *          each rounded to f32.  The midpoint (p_lo + p_hi) * 0.5f (f32, per component) is taken instead when det == 0, when det is not
 *          finite, or when one of the three f32 results is not finite
 *       e. cost: with (x, y, z) the f64 of that f32 position, r_i = ((q_i0*x + q_i1*y) + q_i2*z) + q_i3 for i = 0..3 (the four row sums,
 *          left to right), cost = ((x*r0 + y*r1) + z*r2) + r3 (the dot with (x, y, z, 1), left to right).  Costs are ordered by
 *          f64::total_cmp, as in the reference: by the key k(cost) = bits ^ 0xFFFFFFFFFFFFFFFF when the sign bit is set, else
 *          bits | 0x8000000000000000, compared as u64.  The RANK of an edge is (k(cost), lo, hi), lexicographic
 *       f. selection and budget: a candidate is SELECTED when no other candidate incident to lo or to hi has a lower rank; selected
 *          edges share no vertex.  The selected edges sorted by rank; TAKEN is the shortest prefix whose multiplicities sum to at least
 *          alive - target, all of them if the total is less.  No face holds two selected edges, so the round removes exactly that sum of
 *          faces.  When nothing is selected the loop ends
 *       g. a taken edge is applied: the position of lo = (d); Q_lo = Q, the sum already formed; hi maps to lo (the smaller index
 *          survives, vertex1 < vertex2 in the reference).  Faces: hi -> lo; a face that now repeats an index is dropped; alive = the
 *          number left
 *    6. output: the vertices referenced by a surviving face, in ascending input index, renumbered; the faces in input order with their
 *       orientation; out_vertex_map[i] = the output index of the vertex that i ended in (chains always go to smaller indices),
 *       0xFFFFFFFF when that vertex is in no surviving face
 * Termination: the number of rounds is not bounded by a constant (a fan with preserve_boundary = 0 takes one collapse per round), but every
 * round with a candidate selects the candidate of lowest rank and takes at least that one, which removes at least one face, and a round
 * without a candidate ends the loop.  There is no cap on the rounds.
 * Deviations from quadric_error.rs:
 *   - rounds instead of one global queue: the order of collapses differs, so results are compared with the reference for quality, not
 *     for identity
 *   - boundary vertices are recomputed every round; the reference does so every 100 collapses
 *   - an input face that repeats an index is dropped first; in the reference it adds the quadric of the plane z = 0 to its vertices
 *   - only vertices referenced by a surviving face are output; the reference keeps some orphans through its never-updated `faces` sets
 *   - a face index out of range and a coordinate that is not finite are errors; the reference panics or carries the NaN
 *   - (5d) restates the rule of nalgebra's try_inverse (a zero determinant gives None) through cofactors; it does not claim nalgebra's
 *     bits, and adds the fallback for results that are not finite
 *   - like the reference: no fold-over test and no conditioning guard on det.  Results need not be manifold */
#ifndef THREECRATE_HIP_QEM_H
#define THREECRATE_HIP_QEM_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tc_qem_config {          /* QuadricErrorSimplifier's fields that are read, and simplify()'s ratio, quadric_error.rs */
    float    reduction_ratio;           /* [0, 1] */
    uint32_t preserve_boundary;         /* 0 | 1 */
    float    max_edge_length;           /* 0 = no limit (the reference's None); > 0: longer edges do not collapse */
} tc_qem_config;

/* ratio as given, 1, 0 (no limit).  NULL is allowed. */
void tc_qem_config_default(float reduction_ratio, tc_qem_config *cfg);

/* Simplify n_vertices vertices (n_vertices x 3 floats) over the faces (n_faces x 3 uint32 vertex indices).
 *   out_vertices     room for cap_vertices x 3 floats, or NULL
 *   out_faces        room for cap_faces x 3 uint32, or NULL
 *   out_vertex_map   n_vertices uint32, or NULL: step 6 of the contract
 *   n_out_vertices, n_out_faces   the counts; written by every call that passes its checks (1) to (6)
 *   n_rounds         NULL, or the number of rounds that took at least one collapse; written with the counts
 * n_vertices and n_faces are upper bounds of the counts: a caller who allocates those calls once.  With out_vertices, out_faces and
 * out_vertex_map all NULL the call gives the counts alone.  With any of them present, cap_vertices below n_out_vertices or cap_faces below
 * n_out_faces is TC_INVALID_DATA and nothing but the counts is written (as tc_simplify_clustering answers).  No output may overlap an
 * input.
 * Checks, in this order:
 *   1. a NULL context, vertices, faces, cfg, n_out_vertices or n_out_faces: TC_INVALID_DATA
 *   2. n_vertices == 0 or n_faces == 0: TC_INVALID_DATA ("Mesh is empty")
 *   3. preserve_boundary > 1: TC_INVALID_DATA
 *   4. reduction_ratio not in [0, 1], or NaN: TC_INVALID_DATA ("Reduction ratio must be between 0.0 and 1.0"); then max_edge_length
 *      negative or NaN: TC_INVALID_DATA
 *   5. n_vertices >= 2^32 - 16 or 3 n_faces >= 2^32 - 16: TC_UNSUPPORTED.  Vertex indices and the 3 n_faces edges are 32-bit
 *   6. a face index >= n_vertices, or a vertex coordinate that is not finite: TC_INVALID_DATA.  Both are found on the device and share
 *      one read-back
 *   7. the capacities
 * reduction_ratio == 0 is TC_OK after checks (1) to (6) with the mesh copied: all n_vertices vertices, unreferenced ones included, the
 * faces as given (those that repeat an index too), the map the identity, no rounds; the counts are n_vertices and n_faces and the
 * capacities are checked against them.  An output of zero faces and zero vertices is TC_OK.  A call that fails writes nothing but, from
 * check (7) on, the counts.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for every array (cfg, the two
 * counts and n_rounds are host pointers in both), works on the context's stream, waits for the flags of (6), once per round for the
 * round's result, and for the counts, and returns with the work complete (the call's scratch is released on return). */
tc_status tc_simplify_quadric(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                              const tc_qem_config *cfg, float *out_vertices, size_t cap_vertices, uint32_t *out_faces, size_t cap_faces,
                              uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces, uint32_t *n_rounds);
tc_status tc_simplify_quadric_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                     const tc_qem_config *cfg, float *out_vertices, size_t cap_vertices, uint32_t *out_faces,
                                     size_t cap_faces, uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces,
                                     uint32_t *n_rounds);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_QEM_H */
