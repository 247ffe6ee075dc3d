/* threecrate_hip_mesh.h -- companion surface: smooth a triangle mesh on the device (smooth_laplacian, smooth_taubin, smooth_hc,
 * threecrate-algorithms/src/mesh_smoothing.rs; the wheel's smooth_mesh_laplacian / _taubin / _hc) and the one-ring vertex adjacency
 * they sweep over, as a CSR built from the faces.
 *
 * The symbols live in a library of their own, libthreecrate_hip_mesh.so, which is linked against libthreecrate_hip.so (it sits
 * in the same directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by
 * tc_context_create serves both.  tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * ---- the contract, in the order of operations; every result is bit for bit ----
 * All arithmetic is f32, one rounding per operation (no contraction), IEEE division.  Coordinates that are not finite propagate by
 * IEEE rules; nothing is filtered.
 *    1. adjacency: every face (a, b, c) contributes the directed pairs (a,b) (a,c) (b,a) (b,c) (c,a) (c,b); adj[i] is the set of
 *       distinct j with a pair (i, j), in ASCENDING order of j.  A face that repeats an index makes a vertex its own neighbour
 *       (the reference's HashSet does the same)
 *    2. centroid of x at vertex i, deg = |adj[i]| > 0: per component s = +0; for j in adj[i], ascending: s = s + x[j];
 *       c = s / f32(deg).  A vertex with deg == 0 has no centroid: it keeps its position wherever one is asked for
 *    3. Laplacian step with factor t: d = c - v; m = d * t; out = v + m (three roundings per component); deg == 0: out = v
 *    4. TC_MESH_LAPLACIAN: `iterations` steps with lambda
 *    5. TC_MESH_TAUBIN: per iteration a step with lambda, then a step with mu
 *    6. TC_MESH_HC: p = the input, q = p; w = 1 - alpha and u = 1 - beta, rounded once; per iteration, for every vertex
 *           qbar  = centroid of q (deg == 0: q)
 *           blend = p * alpha + q * w                       (two products, one sum)
 *           b     = qbar - blend
 *       and then, for every vertex
 *           avg   = (fold of b[j] over adj[i], ascending, from +0) / f32(deg)        (deg == 0: +0)
 *           corr  = b * beta + avg * u
 *           q     = qbar - corr
 * Deviations from mesh_smoothing.rs:
 *   - the summation order of (2) and (6) is fixed: ascending neighbour index.  The reference iterates a HashSet, whose order differs
 *     from process to process; any of its orders lies within 2 (deg - 1) 2^-24 sum|x_j| of this one per component.
 *   - a face index >= n_vertices is TC_INVALID_DATA.  The reference panics, or with iterations == 0 does not look; here the check
 *     precedes the iterations == 0 shortcut.
 *   - a parameter that is not finite is TC_INVALID_DATA.  The reference's `lambda <= 0 || lambda > 1` lets a NaN through. */
#ifndef THREECRATE_HIP_MESH_H
#define THREECRATE_HIP_MESH_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_MESH_LAPLACIAN 0u
#define TC_MESH_TAUBIN    1u
#define TC_MESH_HC        2u

typedef struct tc_mesh_smooth_config {  /* LaplacianSmoothingConfig | TaubinSmoothingConfig | HcSmoothingConfig, mesh_smoothing.rs */
    uint32_t method;                    /* TC_MESH_LAPLACIAN | TC_MESH_TAUBIN | TC_MESH_HC */
    uint32_t iterations;
    float    lambda;                    /* Laplacian: (0, 1]; Taubin: (0, 1) */
    float    mu;                        /* Taubin: < 0 */
    float    alpha;                     /* HC: [0, 1] */
    float    beta;                      /* HC: [0, 1] */
} tc_mesh_smooth_config;

/* method as given, 10 iterations, lambda 0.5, mu -0.53, alpha 0, beta 0.5 (the three Default impls).  NULL is allowed. */
void tc_mesh_smooth_config_default(uint32_t method, tc_mesh_smooth_config *cfg);

/* Smooth n_vertices vertices (n_vertices x 3 floats) over the faces (n_faces x 3 uint32 vertex indices).
 *   out_vertices   n_vertices x 3 floats; may be `vertices` itself
 * Checks, in this order:
 *   1. a NULL context, vertices, faces, cfg or out_vertices: TC_INVALID_DATA
 *   2. n_vertices == 0 or n_faces == 0: TC_INVALID_DATA ("Mesh is empty")
 *   3. method > 2: TC_INVALID_DATA
 *   4. the method's parameters (the other methods' are not read): Laplacian "lambda must be in (0, 1]"; Taubin "lambda must be in
 *      (0, 1)", then "mu must be negative"; HC "alpha must be in [0, 1]", then "beta must be in [0, 1]"; a parameter that is not
 *      finite fails the same check: TC_INVALID_DATA
 *   5. n_vertices >= 2^32 - 16 or 6 n_faces >= 2^32 - 16 (n_faces > 715 827 879): TC_UNSUPPORTED.  Vertex indices, the 6 n_faces
 *      directed pairs and the CSR offsets are 32-bit
 *   6. a face index >= n_vertices: TC_INVALID_DATA.  Found on the device; costs the call's one read-back
 * iterations == 0 is then TC_OK with the input copied.  A call that fails writes nothing.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for vertices, faces and
 * out_vertices (cfg is a host pointer in both) and works on the context's stream: it waits once for the read-back of (6), enqueues
 * every sweep without a host wait between them, and returns with the work complete (the call's scratch is released on return). */
tc_status tc_mesh_smooth(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                         const tc_mesh_smooth_config *cfg, float *out_vertices);
tc_status tc_mesh_smooth_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                const tc_mesh_smooth_config *cfg, float *out_vertices);

/* The one-ring adjacency of (1) as a CSR: the neighbours of vertex i are neighbors[offsets[i] .. offsets[i + 1]), ascending.
 *   offsets     n_vertices + 1 uint32, or NULL
 *   neighbors   room for `capacity` uint32, or NULL
 *   n_entries   the number of entries (offsets[n_vertices]); always written by a call that passes its checks
 * Count, then fill: with offsets and neighbors both NULL the call gives the count alone.  With either array present, a capacity
 * below the count is TC_INVALID_DATA (as tc_voxel_map_extract and tc_tsdf_extract_surface answer) and nothing but n_entries is written.
 * Checks, in this order: a NULL context, faces or n_entries: TC_INVALID_DATA; (2), (5) and (6) of tc_mesh_smooth; the capacity.
 * The _device variant takes device pointers for faces, offsets and neighbors; n_entries is a host pointer in both. */
tc_status tc_mesh_vertex_adjacency(tc_context *ctx, size_t n_vertices, const uint32_t *faces, size_t n_faces, uint32_t *offsets,
                                   uint32_t *neighbors, size_t capacity, size_t *n_entries);
tc_status tc_mesh_vertex_adjacency_device(tc_context *ctx, size_t n_vertices, const uint32_t *faces, size_t n_faces, uint32_t *offsets,
                                          uint32_t *neighbors, size_t capacity, size_t *n_entries);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_MESH_H */
