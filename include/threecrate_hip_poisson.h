/* threecrate_hip_poisson.h -- companion surface: Poisson surface reconstruction on the device, an oriented point cloud (points +
 * normals) to an indicator field on a dense grid and to a closed triangle mesh (poisson_reconstruction,
 * threecrate-reconstruction/src/poisson.rs).
 *
 * The symbols live in a library of their own, libthreecrate_hip_poisson.so, which is linked against libthreecrate_hip.so and
 * libthreecrate_hip_mc.so (they sit in the same directory and are found through $ORIGIN) and uses their status, context and grid
 * types: a tc_context made by tc_context_create serves all of them.  tc_abi_version() is unchanged.  A consumer links this library and
 * libthreecrate_hip.so; tc_mc_grid comes from threecrate_hip_mc.h.
 *
 * ---- DEVIATION: the solver is this header's, not the reference's ----
 * The reference validates its input and hands it to the external poisson_reconstruction crate (an adaptive octree, depth at most 6).
 * That crate is not part of the reference tree and its octree cannot be restated here.  This surface keeps the reference's entry
 * checks (empty cloud, fewer than 10 points, the magnitude rule of the normals) and its configuration names where they have a meaning
 * (depth, scale) and solves the screened Poisson equation on a DENSE grid of N = 2^depth nodes per axis, as specified in full below.
 * Its output is therefore not the reference's mesh; what is pinned is this contract, restated in numpy by tests/poisson_checker.py.
 * Out of scope: the adaptive octree, per-point confidence, output_density, multigrid or FFT solvers.
 *
 * ---- the contract ----
 * 1. Checks, in this order.  A failing call writes nothing.
 *      a NULL context, points, normals, config or stats (tc_poisson_field: or grid; tc_poisson_reconstruct: or n_vertices, n_faces):
 *          TC_INVALID_DATA
 *      n == 0: TC_INVALID_DATA, "Point cloud is empty"
 *      n < 10: TC_INVALID_DATA, "Point cloud too small for Poisson reconstruction (minimum 10 points)"
 *      depth outside 2 .. 8; scale < 1 or not finite; a negative or NaN point_weight, tolerance or min_density: TC_INVALID_DATA
 *      n >= 2^29: TC_UNSUPPORTED (the 8 n splat records are indexed in 32 bits)
 *      a coordinate that is not finite, or a normal with |n| < 1e-6f or | |n| - 1.0f | > 0.1f (a NaN fails), where
 *          |n| = sqrtf((x x + y y) + z z) in f32: TC_INVALID_DATA.  Found on the device in one pass, which also gives the bounding box
 *      a bounding box whose largest extent is 0: TC_INVALID_DATA
 * 2. Grid, f32, one rounding per operation.  N = 2^depth.
 *      c_k = 0.5f * (min_k + max_k);  side = scale * max_k(max_k - min_k);  h = side / f32(N - 1);  origin_k = c_k - 0.5f * side
 *      grid.dims = (N, N, N), grid.voxel_size = (h, h, h), grid.origin = origin, grid.layout = TC_MC_X_FASTEST: node (x, y, z) is
 *      element (z N + y) N + x of chi and density, so both go straight into tc_marching_cubes.
 * 3. Splat.  For point p: g_k = (p_k - origin_k) / h;  i_k = min(floor(g_k), N - 2), and 0 when g_k < 0;  f_k = g_k - f32(i_k).
 *      Corner c = 0 .. 7 is node (i_x + (c & 1), i_y + ((c >> 1) & 1), i_z + (c >> 2)); its weight is (wx * wy) * wz in f32 with
 *      w_k = f_k for an upper corner and 1.0f - f_k for a lower one.
 *      V_k(node) = sum of f64(w) * f64(n_k) and W(node) = sum of f64(w) over the records of the node, IN INPUT ORDER of their points, in
 *      f64, each rounded to f32 once.  There are no floating-point atomics: the 8 n records are keyed by node, sorted stably and every
 *      run is folded sequentially.  density = W.  occupied_nodes = the nodes with W > 0.
 * 4. Right-hand side, f32:  b = (-0.5f * h) * (((Vx[x+1] - Vx[x-1]) + (Vy[y+1] - Vy[y-1])) + (Vz[z+1] - Vz[z-1])); a neighbour
 *      outside the grid reads 0.
 * 5. Operator, f32:  S = ((((p[x-1] + p[x+1]) + p[y-1]) + p[y+1]) + p[z-1]) + p[z+1], a neighbour outside the grid reads 0
 *      (Dirichlet);  (A p)_i = (6.0f * p_i - S) + (point_weight * W_i) * p_i.  The last term is added only when point_weight > 0.
 * 6. Solve A chi = b by plain conjugate gradient from chi = 0, r = b, p = 0, beta = 0, rr = b.b.  Vectors are f32; every inner product
 *      is the sum of f64(u_i) * f64(v_i) in f64, reduced in a fixed two-level order (per-block partials over a fixed grid, then one
 *      folding block), so two calls give the same bits.  b.b == 0, or max_iterations == 0: chi = 0, 0 iterations, rel_residual 0
 *      (b.b == 0) or 1.  One iteration:
 *          p_i = r_i + beta * p_i;  q = A p;  alpha = f32(rr / p.q)     (an f64 quotient, rounded once)
 *          chi_i = chi_i + alpha * p_i;  r_i = r_i - alpha * q_i;  rr' = r.r;  iterations += 1;  rel_residual = f32(sqrt(rr' / b.b))
 *          stop when sqrt(rr' / b.b) <= tolerance (compared in f64) or iterations == max_iterations; else beta = f32(rr' / rr), rr = rr'
 *      Neither ending is an error.  p.q <= 0 or NaN (A is positive definite: only rounding reaches it) ends the loop before the update.
 *      stats.rel_residual is the last recurrence value, not a recomputed residual.
 * 7. iso_value = f32((sum over the points, in input order, in f64, of s_p) / f64(n)), where s_p = the sum over corners c = 0 .. 7, in
 *      that order, of f64(w_c) * f64(chi[corner c]) with step 3's weights.
 * 8. Orientation.  grad chi follows the normals: with outward normals chi < iso_value is the inside, which is marching cubes' "inside"
 *      (threecrate_hip_mc.h: a triangle's right-hand normal (v1 - v0) x (v2 - v0) points to the inside).  The welded faces of
 *      tc_poisson_reconstruct therefore wind so that their right-hand normals point AGAINST the input normals: a sphere given outward
 *      normals has a negative signed volume.  Marching cubes is used as it is.
 * tc_poisson_reconstruct = tc_poisson_field, then tc_marching_cubes_device with flags TC_MC_WELD, iso_level = iso_value and, when
 * min_density > 0, valid = (density >= min_density), bit for bit what the two calls give when made separately. */
#ifndef THREECRATE_HIP_POISSON_H
#define THREECRATE_HIP_POISSON_H

#include "threecrate_hip.h"
#include "threecrate_hip_mc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_POISSON_MIN_POINTS 10u
#define TC_POISSON_MIN_DEPTH  2u
#define TC_POISSON_MAX_DEPTH  8u

typedef struct tc_poisson_config {
    uint32_t depth;                     /* 2 .. 8: N = 2^depth nodes per axis */
    float    scale;                     /* >= 1: the grid's side over the bounding box's largest extent */
    float    point_weight;              /* >= 0: the screening weight (0 = plain Poisson) */
    uint32_t max_iterations;
    float    tolerance;                 /* >= 0: on sqrt(r.r / b.b) */
    float    min_density;               /* >= 0; tc_poisson_reconstruct: nodes with density below it are not usable (0 = no trimming) */
} tc_poisson_config;

typedef struct tc_poisson_stats {
    uint32_t iterations;
    float    rel_residual;
    float    iso_value;
    uint32_t occupied_nodes;
} tc_poisson_stats;

/* depth 6 (what the reference's clamp makes of its default 8), scale 1.1, point_weight 0, max_iterations 200, tolerance 1e-5,
 * min_density 0.  NULL is allowed. */
void tc_poisson_config_default(tc_poisson_config *cfg);

/* The indicator field of an oriented cloud.  points, normals: n x 3 floats each.  grid: written.  chi, density: room for N^3 floats each,
 * or NULL.  stats: written.  The _device variant takes device pointers for points, normals, chi and density; config, grid and stats are
 * host pointers in both.  Both return with the work complete. */
tc_status tc_poisson_field(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg, tc_mc_grid *grid,
                           float *chi, float *density, tc_poisson_stats *stats);
tc_status tc_poisson_field_device(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg, tc_mc_grid *grid,
                                  float *chi, float *density, tc_poisson_stats *stats);

/* The field, then its welded iso surface.  vertices: room for vertex_capacity x 3 floats, or NULL; faces: room for face_capacity x 3
 * uint32, or NULL.  With both NULL the call gives the counts (and stats) alone.  Otherwise vertex_capacity below n_vertices or
 * face_capacity below n_faces is TC_INVALID_DATA and nothing but the counts is written (tc_marching_cubes' protocol).  The _device
 * variant takes device pointers for points, normals, vertices and faces; config, counts and stats are host pointers in both. */
tc_status tc_poisson_reconstruct(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg,
                                 float *vertices, uint32_t *faces, size_t vertex_capacity, size_t face_capacity, size_t *n_vertices, size_t *n_faces,
                                 tc_poisson_stats *stats);
tc_status tc_poisson_reconstruct_device(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg,
                                        float *vertices, uint32_t *faces, size_t vertex_capacity, size_t face_capacity, size_t *n_vertices,
                                        size_t *n_faces, tc_poisson_stats *stats);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_POISSON_H */
