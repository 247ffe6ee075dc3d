/* threecrate_hip_simplify.h -- companion surface: simplify a triangle mesh on the device by vertex clustering (ClusteringSimplifier,
 * threecrate-simplification/src/clustering.rs; Rossignac & Borrel 1993): a cell key per vertex, one representative per cell, the faces
 * remapped, degenerate and repeated faces dropped.
 *
 * The symbols live in a library of their own, libthreecrate_hip_simplify.so, which is linked against libthreecrate_hip.so (it sits
 * in the same directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by
 * tc_context_create serves both.  tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * In scope: ClusteringMode::Uniform; RepresentativeStrategy::Centroid and WeightedAverage; preserve_boundary;
 * feature_angle_threshold; per-vertex normals and colours carried through.
 * Out of scope:
 *   - ClusteringMode::Adaptive: its octree subdivides on insertion, so its result depends on a sequential insertion order.
 *   - RepresentativeStrategy::MinimumError: its answer is nalgebra's try_inverse of a 3 x 3 f64 matrix, which cannot be pinned
 *     bit for bit without nalgebra.
 *   - the other simplifiers of the crate: quadric edge collapse has a header of its own, threecrate_hip_qem.h (rounds of independent
 *     collapses); progressive meshes are a priority-queue algorithm, one collapse at a time.
 *
 * ---- the contract, in the order of operations; every result is bit for bit ----
 *    1. box: per axis the minimum and maximum over ALL vertices (referenced by a face or not), as f64 of the f32 values;
 *       size = max - min in f64
 *    2. cell size (host, f64): target = f64(max((1.0f - ratio) * f32(n_vertices), 1.0f)), product and max in f32; extents = the sizes
 *       > 1e-6, dim of them; dim == 0: cell = 1.0; else cell = pow(product(extents) / target, 1.0 / dim), C pow, the product taken
 *       in axis order from 1.0.  Per axis floor(size / cell) must be below 2^20 (check 7)
 *    3. edges: every face (a, b, c) contributes the undirected edges (min, max) of (a,b), (b,c), (c,a), with multiplicity; a face
 *       that repeats an index contributes what that gives.  An edge with exactly one incidence makes both its ends BOUNDARY.  An edge
 *       with exactly two incidences makes both its ends FEATURE when dot < cosf(feature_angle_threshold) (the host's cosf), dot taken
 *       between the normals of the two incident faces.  Face normal, f32, one rounding per operation, no contraction:
 *           e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 (each component two products and one difference),
 *           len = sqrtf((nx*nx + ny*ny) + nz*nz), n / len when len > 1e-12f, else (0, 0, 1);
 *           dot = (ax*bx + ay*by) + az*bz
 *       Both sets are computed whether or not they are used; preserve_boundary == 0 ignores the boundary set
 *    4. class of a vertex: 1 when preserve_boundary and the vertex is boundary; else 2 when it is feature; else 0
 *    5. cell: ix = (int64) floor((f64(x) - min_x) / cell), f64 subtraction and IEEE f64 division; iy, iz the same way.  A cluster is
 *       the set of vertices with equal (ix, iy, iz, class)
 *    6. order: clusters are numbered in ascending lexicographic order of (ix, iy, iz, class); the members of a cluster are in
 *       ascending vertex index (the packed key ix << 42 | iy << 22 | iz << 2 | class, stable sort, the vertex index as value)
 *    7. representative: a cluster of one is its vertex, the f32 bits unchanged.  Centroid: per component s = +0.0 (f64); for the
 *       members in order s = s + f64(x); the result is f32(s / f64(count)).  Weighted average: w = f64(max(valence, 1)), valence = the
 *       number of face incidences of the vertex; s = s + f64(x) * w (one product, one sum); W = W + w; the result is f32(s / W)
 *    8. faces: face f maps to (c0, c1, c2), the cluster numbers of its vertices; it is dropped when two of them are equal; of the
 *       faces whose sorted triples are equal the one with the smallest face index survives, with its own orientation; survivors keep
 *       their input order
 *    9. compaction: the clusters that occur in a surviving face are renumbered in cluster order: the output vertex order; the faces
 *       are rewritten to the new numbers
 *   10. normals: per component an f32 fold from +0 over the members in order; len = sqrtf((x*x + y*y) + z*z); each component is
 *       divided by len when len > 1e-12f.  Clusters of one go through the same arithmetic, as in the reference
 *   11. colours: per channel the u32 sum over the members, integer-divided by the count
 * Deviations from clustering.rs:
 *   - the output vertex order is fixed by (6).  The reference's comes out of a HashMap and differs from process to process; its
 *     member order is the vertex order, as here, so no summation-order bound is needed: the sums are the reference's own
 *   - a coordinate that is not finite is an error.  In the reference `NaN as i64` is 0, and the box ignores NaN
 *   - the 20-bit cell index limit is new.  The reference uses i64 cell indices
 *   - a face index out of range is an error.  The reference panics
 *   - the two omitted modes, above */
#ifndef THREECRATE_HIP_SIMPLIFY_H
#define THREECRATE_HIP_SIMPLIFY_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_SIMPLIFY_CENTROID          0u
#define TC_SIMPLIFY_WEIGHTED_AVERAGE  1u

typedef struct tc_simplify_config {     /* ClusteringSimplifier's fields and simplify()'s ratio, clustering.rs */
    uint32_t strategy;                  /* TC_SIMPLIFY_CENTROID | TC_SIMPLIFY_WEIGHTED_AVERAGE */
    uint32_t preserve_boundary;         /* 0 | 1 */
    float    feature_angle_threshold;   /* radians */
    float    reduction_ratio;           /* [0, 1] */
} tc_simplify_config;

/* centroid, 1, 45 degrees as f32 radians (45.0f32.to_radians()), ratio as given.  NULL is allowed. */
void tc_simplify_config_default(float reduction_ratio, tc_simplify_config *cfg);

/* Simplify n_vertices vertices (n_vertices x 3 floats) over the faces (n_faces x 3 uint32 vertex indices).
 *   normals          n_vertices x 3 floats, or NULL            colors        n_vertices x 3 bytes, or NULL
 *   out_vertices     room for cap_vertices x 3 floats, or NULL
 *   out_normals      cap_vertices x 3 floats; required exactly when normals is given
 *   out_colors       cap_vertices x 3 bytes; required exactly when colors is given
 *   out_faces        room for cap_faces x 3 uint32, or NULL
 *   out_vertex_map   n_vertices uint32, or NULL: the output index of the cluster vertex i fell into, 0xFFFFFFFF when that cluster
 *                    is in no surviving face
 *   n_out_vertices, n_out_faces   the counts; written by every call that passes its checks (1) to (7)
 * n_vertices and n_faces are upper bounds of the counts: a caller who allocates those calls once.  With out_vertices, out_normals,
 * out_colors, out_faces and out_vertex_map all NULL the call gives the counts alone.  With any of them present, cap_vertices below
 * n_out_vertices or cap_faces below n_out_faces is TC_INVALID_DATA and nothing but the counts is written (as
 * tc_mesh_vertex_adjacency and tc_tsdf_extract_surface answer).  No output may overlap an input.
 * Checks, in this order:
 *   1. a NULL context, vertices, faces, cfg, n_out_vertices or n_out_faces; normals without out_normals or the reverse; colors
 *      without out_colors or the reverse: TC_INVALID_DATA
 *   2. n_vertices == 0 or n_faces == 0: TC_INVALID_DATA ("Mesh is empty")
 *   3. strategy > 1 or preserve_boundary > 1: TC_INVALID_DATA
 *   4. reduction_ratio not in [0, 1], or NaN: TC_INVALID_DATA ("Reduction ratio must be between 0.0 and 1.0"); then
 *      feature_angle_threshold not finite: TC_INVALID_DATA
 *   5. n_vertices >= 2^32 - 16 or 3 n_faces >= 2^32 - 16: TC_UNSUPPORTED.  Vertex indices and the 3 n_faces edges are 32-bit
 *   6. a face index >= n_vertices, or a vertex coordinate that is not finite: TC_INVALID_DATA.  Both are found on the device and
 *      share one read-back
 *   7. a cell index that does not fit 20 bits (step 2 of the contract): TC_UNSUPPORTED; decided on the host from the box and the
 *      cell size
 *   8. the capacities
 * reduction_ratio == 0 is TC_OK after checks (1) to (6) with the mesh copied: all n_vertices vertices, unreferenced ones included,
 * the faces as given, normals and colours as given, the map the identity; the counts are n_vertices and n_faces and the capacities
 * are checked against them.  An output of zero faces and zero vertices is TC_OK.  A call that fails writes nothing but, from check
 * (8) on, the counts.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for every array (cfg and the
 * two counts are host pointers in both), works on the context's stream, waits for the box, for the flag of (6) and for the counts,
 * and returns with the work complete (the call's scratch is released on return). */
tc_status tc_simplify_clustering(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                 const float *normals, const uint8_t *colors, const tc_simplify_config *cfg, float *out_vertices,
                                 float *out_normals, uint8_t *out_colors, size_t cap_vertices, uint32_t *out_faces, size_t cap_faces,
                                 uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces);
tc_status tc_simplify_clustering_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                        const float *normals, const uint8_t *colors, const tc_simplify_config *cfg, float *out_vertices,
                                        float *out_normals, uint8_t *out_colors, size_t cap_vertices, uint32_t *out_faces,
                                        size_t cap_faces, uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_SIMPLIFY_H */
