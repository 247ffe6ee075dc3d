// simplify.hip -- simplify a triangle mesh by vertex clustering (ClusteringSimplifier, threecrate-simplification/src/clustering.rs, its
// uniform road); the entry points of include/threecrate_hip_simplify.h, which pins the arithmetic and the order of everything.
// This unit is the whole of the companion library libthreecrate_hip_simplify.so; the host layer of tc_internal.h (ensure, stage_in,
// read_back, cloud_bbox, group_by_key, sort_pairs, exclusive_scan_u32, ProfScope) resolves from libthreecrate_hip.so.
//   The class stage, one profile row (simplify_classes):
//   simp_pack        a thread per vertex: its 16-byte record (x, y, z, 0); a coordinate that is not finite raises flag bit 1
//   simp_edge_key    a thread per face: its three undirected edges as packed keys min << b | max (b = bits_for_value(n - 1)), the face as
//                    value; an integer atomicAdd per corner counts the valence; an index >= n raises flag bit 0 and its face writes vertex 0
//   group_by_key (grid.hip)   one run per distinct edge, the faces of a run ascending
//   simp_edge_class  a thread per run head: a run of one ORs the boundary bit into both ends, a run of two computes the two face normals
//                    and ORs the feature bit where dot < cos.  The ORs are idempotent: no order shows
//   -- the box (cloud_bbox) and one read-back: the flags --   the cell size, on the host
//   The cluster stage (simplify_clusters):
//   simp_vertex_key  a thread per vertex: ix << 42 | iy << 22 | iz << 2 | class, f64 arithmetic; the vertex as value
//   group_by_key   one run per cluster, its members ascending; the run number is the cluster number
//   simp_cluster_of  the cluster number of every vertex; the clusters of more than kSimplifyLongCluster members, listed
//   simp_fold        a lane per cluster of at most kSimplifyLongCluster members: position (f64), normal (f32) and colour (u32) folded in
//                    member order, four gathers in flight (fold_run_lane's shape, run_fold.h, written out)
//   simp_fold_long   a wave per listed cluster: 64 members loaded at once, the adds sequential on broadcast values (fold_run_wave's shape): the same bits
//   The face stage (simplify_faces):
//   simp_face_key    a thread per face: the sorted triple of its cluster numbers as ONE 64-bit key where three numbers fit, else as a
//                    32-bit key (the largest) and, gathered after the first pass, a 64-bit key (the other two): two stable passes
//   simp_face_keep   a thread per sorted position: the face survives when it is not degenerate and the face before it has another triple
//   exclusive_scan_u32 over the survivors in face order; simp_mark_used; exclusive_scan_u32 over the used clusters
//   -- one read-back: the counts --   the capacities
//   simp_write_vertices / _faces / _map   (simplify_write)
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_simplify.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// A cluster of more members than this is folded by a wave (simp_fold_long).  TC_SIMPLIFY_LONG_CLUSTER: the A/B builds of
// `make simplify-ab` (variants/, what tools/simplify_bench.py --cluster loads); never the product.  128 is mesh.hip's kMeshLongRing, measured
// on the same two roads of run_fold.h (a sequential fold of gathered 16-byte records on one lane against 64 records per wave trip): the
// crossing of THIS fold has not been measured (STATE.md).
#ifdef TC_SIMPLIFY_LONG_CLUSTER
constexpr uint32_t kSimplifyLongCluster = TC_SIMPLIFY_LONG_CLUSTER;
#else
constexpr uint32_t kSimplifyLongCluster = 128;
#endif
constexpr int kSimplifyLongBlocks = 1024;       // the wave-per-cluster kernel's grid is fixed (the list's length stays on the device); its waves stride
constexpr uint32_t kSimpBadIndex = 1u, kSimpNotFinite = 2u;     // SimplifyOut::flags
constexpr uint32_t kSimpBoundary = 1u, kSimpFeature = 2u;       // the per-vertex word of the class stage

// what the folds read and write; one record per cluster
struct SimpFold {
    const float4 *rec;          // positions, 16-byte records
    const uint32_t *valence;    // face incidences per vertex
    const float *normals;       // n x 3, or null
    const uint8_t *colors;      // n x 3, or null
    const uint32_t *members;    // the vertices cluster by cluster, ascending inside one
    const uint32_t *rstart;     // first member of every cluster, rstart[R] = n
    const uint32_t *runpos;     // runpos[n] = R
    float4 *rep;                // representative of every cluster
    float4 *nrm;                // its normal (normals given)
    uint32_t *col;              // its colour, r | g << 8 | b << 16 (colours given)
    uint32_t weighted;          // TC_SIMPLIFY_WEIGHTED_AVERAGE
    uint32_t n;
};

__global__ void __launch_bounds__(256) simp_pack_kernel(const float *__restrict__ xyz, uint32_t n, float4 *__restrict__ rec, uint32_t *__restrict__ flags) {
    pack_xyz_records<true>(xyz, n, rec, flags, kSimpNotFinite);
}

__global__ void __launch_bounds__(256) simp_edge_key_kernel(const uint32_t *__restrict__ faces, uint32_t m, uint32_t n, uint32_t b, uint64_t *__restrict__ keys,
                                                           uint32_t *__restrict__ vals, uint32_t *__restrict__ valence, uint32_t *__restrict__ flags) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (f < m) {
        uint32_t v[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
        bad = v[0] >= n || v[1] >= n || v[2] >= n;
        if (bad) v[0] = v[1] = v[2] = 0u;                       // the call fails; the keys stay inside their bits
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t p = v[k], q = v[k == 2 ? 0 : k + 1];
            keys[3 * (size_t)f + k] = ((uint64_t)min(p, q) << b) | (uint64_t)max(p, q);
            vals[3 * (size_t)f + k] = f;
            atomicAdd(&valence[p], 1u);                         // an integer count: no order shows
        }
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flags, kSimpBadIndex);
}

// the header's (3): the unit normal of face f, one rounding per operation
__device__ __forceinline__ void simp_face_normal(const uint32_t *__restrict__ faces, const float4 *__restrict__ rec, uint32_t f, float &ox, float &oy, float &oz) {
    const float4 v0 = rec[faces[3 * (size_t)f]], v1 = rec[faces[3 * (size_t)f + 1]], v2 = rec[faces[3 * (size_t)f + 2]];
    const float ax = v1.x - v0.x, ay = v1.y - v0.y, az = v1.z - v0.z;
    const float bx = v2.x - v0.x, by = v2.y - v0.y, bz = v2.z - v0.z;
    const float p0 = ay * bz, p1 = az * by, p2 = az * bx, p3 = ax * bz, p4 = ax * by, p5 = ay * bx;
    const float nx = p0 - p1, ny = p2 - p3, nz = p4 - p5;
    const float xx = nx * nx, yy = ny * ny, zz = nz * nz;
    const float len = sqrtf((xx + yy) + zz);
    if (len > 1e-12f) { ox = nx / len; oy = ny / len; oz = nz / len; }
    else { ox = 0.0f; oy = 0.0f; oz = 1.0f; }
}

// (the call has no bad index when this runs to any effect: a bad face wrote vertex 0 into its keys, and the faces it reads here are those
// of valid keys only when the flag is clear; with the flag set every gather is still inside the arrays, see the clamps)
__global__ void __launch_bounds__(256) simp_edge_class_kernel(const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ faces_sorted,
                                                             const uint32_t *__restrict__ head, uint32_t n_keys, uint32_t b, uint32_t n,
                                                             const uint32_t *__restrict__ faces, const float4 *__restrict__ rec, float cos_thr,
                                                             const uint32_t *__restrict__ flags, uint32_t *__restrict__ vclass) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_keys || !head[p]) return;
    if (*flags & kSimpBadIndex) return;                         // the call fails: `faces` holds an index that must not be followed
    const bool one = p + 1 >= n_keys || head[p + 1];
    const bool two = !one && (p + 2 >= n_keys || head[p + 2]);
    if (!one && !two) return;
    const uint64_t key = keys_sorted[p];
    const uint32_t lo = (uint32_t)(key >> b), hi = (uint32_t)(key & ((1ull << b) - 1ull));        // b <= 32
    if (lo >= n || hi >= n) return;                             // (never: the keys were built from checked indices)
    uint32_t bit = kSimpBoundary;
    if (two) {
        float ax, ay, az, bx, by, bz;
        simp_face_normal(faces, rec, faces_sorted[p], ax, ay, az);
        simp_face_normal(faces, rec, faces_sorted[p + 1], bx, by, bz);
        const float xx = ax * bx, yy = ay * by, zz = az * bz;
        const float dot = (xx + yy) + zz;
        if (!(dot < cos_thr)) return;
        bit = kSimpFeature;
    }
    atomicOr(&vclass[lo], bit);
    atomicOr(&vclass[hi], bit);
}

struct SimpCells { double minx, miny, minz, cell; };

__global__ void __launch_bounds__(256) simp_vertex_key_kernel(const float4 *__restrict__ rec, const uint32_t *__restrict__ vclass, uint32_t n, SimpCells c,
                                                             uint32_t preserve_boundary, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r = rec[i];
    const double dx = (double)r.x - c.minx, dy = (double)r.y - c.miny, dz = (double)r.z - c.minz;
    const double qx = dx / c.cell, qy = dy / c.cell, qz = dz / c.cell;
    // the host has seen floor(size / cell) < 2^20 on every axis and the quotient is monotonic in the coordinate: the clamps never act
    const uint64_t ix = (uint64_t)min(max((long long)floor(qx), 0ll), (1ll << 20) - 1), iy = (uint64_t)min(max((long long)floor(qy), 0ll), (1ll << 20) - 1),
                   iz = (uint64_t)min(max((long long)floor(qz), 0ll), (1ll << 20) - 1);
    const uint32_t w = vclass[i];
    const uint32_t cls = (preserve_boundary && (w & kSimpBoundary)) ? 1u : ((w & kSimpFeature) ? 2u : 0u);
    keys[i] = (ix << 42) | (iy << 22) | (iz << 2) | (uint64_t)cls;
    vals[i] = i;
}

__global__ void __launch_bounds__(256) simp_cluster_of_kernel(const uint32_t *__restrict__ members, const uint32_t *__restrict__ head,
                                                             const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ rstart, uint32_t n,
                                                             uint32_t *__restrict__ cluster_of, uint32_t *__restrict__ long_list, uint32_t list_cap,
                                                             uint32_t *__restrict__ n_long) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t c = runpos[p] + head[p] - 1u;                // runpos counts the heads BEFORE p: a head's own run, the next one's for the rest
    cluster_of[members[p]] = c;                                 // members is a permutation of 0 .. n - 1
    if (head[p] && rstart[c + 1] - p > kSimplifyLongCluster) append_long_run(long_list, list_cap, n_long, c);
}

// the running sums of one cluster, the header's (7), (10) and (11); every add is one line of the contract
struct SimpAcc {
    double sx = 0.0, sy = 0.0, sz = 0.0, W = 0.0;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    uint32_t r = 0u, g = 0u, b = 0u;
};
__device__ __forceinline__ void simp_add_pos(SimpAcc &a, float x, float y, float z, uint32_t valence, uint32_t weighted) {
    if (weighted) {
        const double w = (double)max(valence, 1u);
        const double px = (double)x * w, py = (double)y * w, pz = (double)z * w;
        a.sx = a.sx + px; a.sy = a.sy + py; a.sz = a.sz + pz;
        a.W = a.W + w;
    } else {
        a.sx = a.sx + (double)x; a.sy = a.sy + (double)y; a.sz = a.sz + (double)z;
    }
}
__device__ __forceinline__ void simp_finish(const SimpFold &a, uint32_t c, uint32_t s, uint32_t e, const SimpAcc &acc) {
    const uint32_t count = e - s;
    if (count == 1u) {
        a.rep[c] = a.rec[a.members[s]];                         // the f32 bits unchanged
    } else {
        const double d = a.weighted ? acc.W : (double)count;
        a.rep[c] = make_float4((float)(acc.sx / d), (float)(acc.sy / d), (float)(acc.sz / d), 0.0f);
    }
    if (a.normals) {
        const float xx = acc.nx * acc.nx, yy = acc.ny * acc.ny, zz = acc.nz * acc.nz;
        const float len = sqrtf((xx + yy) + zz);
        float4 o = make_float4(acc.nx, acc.ny, acc.nz, 0.0f);
        if (len > 1e-12f) { o.x = acc.nx / len; o.y = acc.ny / len; o.z = acc.nz / len; }
        a.nrm[c] = o;
    }
    if (a.colors) a.col[c] = (acc.r / count) | ((acc.g / count) << 8) | ((acc.b / count) << 16);
}

// The two folds below keep their loops written out: a member's record is position + valence + normal + colour, three of them optional, and the
// batch adds them stage by stage (positions, then normals, then colours) -- through fold_run_lane / fold_run_wave (run_fold.h) the compiler
// orders and unswitches these loops differently (STATE.md).  The order of the adds is run_fold.h's: ascending, one chain per sum.
__global__ void __launch_bounds__(256) simp_fold_kernel(SimpFold a) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n || c >= a.runpos[a.n]) return;
    const uint32_t s = a.rstart[c], e = a.rstart[c + 1];
    if (e - s > kSimplifyLongCluster) return;                   // (a long cluster is folded by its wave)
    SimpAcc acc;
    uint32_t j = s;
    for (; j + 4 <= e; j += 4) {
        uint32_t k[4], val[4];
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) k[u] = a.members[j + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) { r[u] = a.rec[k[u]]; val[u] = a.weighted ? a.valence[k[u]] : 0u; }
#pragma unroll
        for (int u = 0; u < 4; ++u) simp_add_pos(acc, r[u].x, r[u].y, r[u].z, val[u], a.weighted);
        if (a.normals) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float *q = a.normals + 3 * (size_t)k[u];
                acc.nx = acc.nx + q[0]; acc.ny = acc.ny + q[1]; acc.nz = acc.nz + q[2];
            }
        }
        if (a.colors) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint8_t *q = a.colors + 3 * (size_t)k[u];
                acc.r += q[0]; acc.g += q[1]; acc.b += q[2];
            }
        }
    }
    for (; j < e; ++j) {
        const uint32_t k = a.members[j];
        const float4 r = a.rec[k];
        simp_add_pos(acc, r.x, r.y, r.z, a.weighted ? a.valence[k] : 0u, a.weighted);
        if (a.normals) { const float *q = a.normals + 3 * (size_t)k; acc.nx = acc.nx + q[0]; acc.ny = acc.ny + q[1]; acc.nz = acc.nz + q[2]; }
        if (a.colors) { const uint8_t *q = a.colors + 3 * (size_t)k; acc.r += q[0]; acc.g += q[1]; acc.b += q[2]; }
    }
    simp_finish(a, c, s, e, acc);
}

__global__ void __launch_bounds__(256) simp_fold_long_kernel(SimpFold a, const uint32_t *__restrict__ long_list, uint32_t list_cap, const uint32_t *__restrict__ n_long_p) {
    const uint32_t lane = threadIdx.x & 63u;
    for_each_listed_run(long_list, min(*n_long_p, list_cap), [&](uint32_t c) {
        const uint32_t s = a.rstart[c], e = a.rstart[c + 1];
        SimpAcc acc;                                            // every lane runs the same chain
        for (uint64_t base = s; base < e; base += 64) {         // 64 bits: base + 64 may pass 2^32 where e lies within 64 of it
            const uint64_t j = base + lane;
            float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float qx = 0.0f, qy = 0.0f, qz = 0.0f;
            uint32_t val = 0u, rgb = 0u;
            if (j < e) {
                const uint32_t k = a.members[j];
                r = a.rec[k];
                if (a.weighted) val = a.valence[k];
                if (a.normals) { const float *q = a.normals + 3 * (size_t)k; qx = q[0]; qy = q[1]; qz = q[2]; }
                if (a.colors) { const uint8_t *q = a.colors + 3 * (size_t)k; rgb = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16); }
            }
            const int cnt = (int)min((uint64_t)64, e - base);
            for (int l = 0; l < cnt; ++l) {                     // l is wave-uniform: v_readlane with a scalar lane select
                simp_add_pos(acc, lane_f(r.x, l), lane_f(r.y, l), lane_f(r.z, l), lane_u(val, l), a.weighted);
                if (a.normals) { acc.nx = acc.nx + lane_f(qx, l); acc.ny = acc.ny + lane_f(qy, l); acc.nz = acc.nz + lane_f(qz, l); }
                if (a.colors) { const uint32_t w = lane_u(rgb, l); acc.r += w & 255u; acc.g += (w >> 8) & 255u; acc.b += w >> 16; }
            }
        }
        if (lane == 0u) simp_finish(a, c, s, e, acc);
    });
}

// the sorted triple of face f's cluster numbers; false when two of them are equal
__device__ __forceinline__ bool simp_triple(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t f, uint32_t &lo, uint32_t &mid,
                                            uint32_t &hi) {
    const uint32_t c0 = cluster_of[faces[3 * (size_t)f]], c1 = cluster_of[faces[3 * (size_t)f + 1]], c2 = cluster_of[faces[3 * (size_t)f + 2]];
    lo = min(c0, min(c1, c2));
    hi = max(c0, max(c1, c2));
    mid = c0 ^ c1 ^ c2 ^ lo ^ hi;                               // the one that is left (also where two are equal)
    return c0 != c1 && c1 != c2 && c2 != c0;
}

// one pass (bc > 0): key64 = lo << 2 bc | mid << bc | hi.  Two passes (bc == 0): key32 = hi, the first pass's key
__global__ void __launch_bounds__(256) simp_face_key_kernel(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t m, uint32_t bc,
                                                           uint64_t *__restrict__ key64, uint32_t *__restrict__ key32, uint32_t *__restrict__ vals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m) return;
    uint32_t lo, mid, hi;
    simp_triple(faces, cluster_of, f, lo, mid, hi);
    if (bc) key64[f] = ((uint64_t)lo << (2u * bc)) | ((uint64_t)mid << bc) | (uint64_t)hi;
    else key32[f] = hi;
    vals[f] = f;
}

// the second pass's key of the face at every position of the first pass's order
__global__ void __launch_bounds__(256) simp_face_key2_kernel(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t m,
                                                            const uint32_t *__restrict__ order, uint64_t *__restrict__ key64) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    uint32_t lo, mid, hi;
    simp_triple(faces, cluster_of, order[p], lo, mid, hi);
    key64[p] = ((uint64_t)lo << 32) | (uint64_t)mid;
}

// keep[f] for EVERY face: the first of its run of equal triples (the smallest face index: the sorts are stable), unless degenerate
__global__ void __launch_bounds__(256) simp_face_keep_kernel(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t m,
                                                            const uint32_t *__restrict__ order, uint32_t *__restrict__ keep) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t f = order[p];
    uint32_t lo, mid, hi;
    bool live = simp_triple(faces, cluster_of, f, lo, mid, hi);
    if (live && p > 0u) {
        uint32_t l2, m2, h2;
        simp_triple(faces, cluster_of, order[p - 1], l2, m2, h2);          // (a degenerate neighbour's triple repeats a number: never equal)
        live = l2 != lo || m2 != mid || h2 != hi;
    }
    keep[f] = live ? 1u : 0u;
}

__global__ void __launch_bounds__(256) simp_mark_used_kernel(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t m,
                                                            const uint32_t *__restrict__ keep, uint32_t *__restrict__ used) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m || !keep[f]) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) used[cluster_of[faces[3 * (size_t)f + k]]] = 1u;           // every writer stores the same word
}

__global__ void simp_counts_kernel(const uint32_t *__restrict__ cpos_end, const uint32_t *__restrict__ fpos_end, SimplifyOut *__restrict__ out) {
    out->n_out_vertices = *cpos_end;
    out->n_out_faces = *fpos_end;
}

__global__ void __launch_bounds__(256) simp_write_vertices_kernel(SimpFold a, const uint32_t *__restrict__ used, const uint32_t *__restrict__ cpos,
                                                                 float *__restrict__ out_xyz, float *__restrict__ out_nrm, uint8_t *__restrict__ out_rgb) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n || c >= a.runpos[a.n] || !used[c]) return;
    const size_t o = cpos[c];                                   // < the count the host has checked the capacity against
    if (out_xyz) { const float4 r = a.rep[c]; out_xyz[3 * o] = r.x; out_xyz[3 * o + 1] = r.y; out_xyz[3 * o + 2] = r.z; }
    if (out_nrm) { const float4 r = a.nrm[c]; out_nrm[3 * o] = r.x; out_nrm[3 * o + 1] = r.y; out_nrm[3 * o + 2] = r.z; }
    if (out_rgb) { const uint32_t w = a.col[c]; out_rgb[3 * o] = (uint8_t)(w & 255u); out_rgb[3 * o + 1] = (uint8_t)((w >> 8) & 255u); out_rgb[3 * o + 2] = (uint8_t)(w >> 16); }
}

__global__ void __launch_bounds__(256) simp_write_faces_kernel(const uint32_t *__restrict__ faces, const uint32_t *__restrict__ cluster_of, uint32_t m,
                                                              const uint32_t *__restrict__ keep, const uint32_t *__restrict__ fpos,
                                                              const uint32_t *__restrict__ cpos, uint32_t *__restrict__ out_faces) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= m || !keep[f]) return;
    const size_t o = fpos[f];
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * o + k] = cpos[cluster_of[faces[3 * (size_t)f + k]]];
}

__global__ void __launch_bounds__(256) simp_write_map_kernel(const uint32_t *__restrict__ cluster_of, uint32_t n, const uint32_t *__restrict__ used,
                                                            const uint32_t *__restrict__ cpos, uint32_t *__restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = cluster_of[i];
    map[i] = used[c] ? cpos[c] : 0xFFFFFFFFu;
}

__global__ void __launch_bounds__(256) simp_identity_kernel(uint32_t n, uint32_t *__restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[i] = i;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// a call's arrays, all device pointers (the entry points' arguments after staging)
struct SimpCall {
    const float *xyz; size_t n; const uint32_t *faces; size_t m; const float *normals; const uint8_t *colors;
    float *out_xyz; float *out_nrm; uint8_t *out_rgb; size_t cap_vertices; uint32_t *out_faces; size_t cap_faces; uint32_t *out_map;
    bool any_output() const { return out_xyz || out_nrm || out_rgb || out_faces || out_map; }
};

// the header's (2): the cell size, and check (7)
static tc_status simp_cell_size(tc_context *ctx, const float mn[3], const float mx[3], size_t n, float ratio, SimpCells &c) {
    const double size[3] = {(double)mx[0] - (double)mn[0], (double)mx[1] - (double)mn[1], (double)mx[2] - (double)mn[2]};
    const float scaled = (1.0f - ratio) * (float)n;             // clustering.rs:541, f32
    const double target = (double)(scaled > 1.0f ? scaled : 1.0f);
    double product = 1.0;
    int dim = 0;
    for (int a = 0; a < 3; ++a) if (size[a] > 1e-6) { product *= size[a]; ++dim; }
    c.cell = dim == 0 ? 1.0 : std::pow(product / target, 1.0 / (double)dim);
    c.minx = (double)mn[0]; c.miny = (double)mn[1]; c.minz = (double)mn[2];
    for (int a = 0; a < 3; ++a)
        if (!(std::floor(size[a] / c.cell) < 1048576.0)) return fail(ctx, TC_UNSUPPORTED, "simplify_clustering: a cell index does not fit 20 bits");
    return TC_OK;
}

static tc_status simp_check_caps(tc_context *ctx, const SimpCall &a, size_t nv, size_t nf) {
    if (a.cap_vertices < nv) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: cap_vertices is smaller than the number of output vertices");
    if (a.cap_faces < nf) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: cap_faces is smaller than the number of output faces");
    return TC_OK;
}

// a validated call (the header's checks 1 to 5 made); device pointers
static tc_status simplify_on_device(tc_context *ctx, const SimpCall &a, const tc_simplify_config &cfg, size_t *n_out_vertices, size_t *n_out_faces) {
    hipStream_t st = ctx->stream;
    const size_t n = a.n, m = a.m, nk = 3 * m;                  // n, nk < 2^32 - 16
    const size_t big = std::max(nk, n);
    const bool copy = cfg.reduction_ratio == 0.0f;
    const size_t list_cap = n / ((size_t)kSimplifyLongCluster + 1) + 1;
    // keys | values and group_by_key's buffers serve the edges (3 m), then the vertices (n): sized once, for the larger
    ScopedBuf keys, keys_sorted, vals, vals_sorted, head, runpos, rstart, sort_temp, blocksum;
    const GroupBufs group{keys_sorted, vals_sorted, head, runpos, rstart, sort_temp, blocksum};
    ScopedBuf rec, valence, vclass, counters, cluster_of, long_list, rep, nrm, col, key32, key32_sorted, order1, keep, fpos, used, cpos;
    const std::pair<ScopedBuf *, size_t> need[] = {
        {&keys, big * sizeof(uint64_t)}, {&vals, big * sizeof(uint32_t)}, {&rec, n * sizeof(float4)}, {&valence, n * sizeof(uint32_t)}, {&vclass, n * sizeof(uint32_t)}, {&counters, sizeof(SimplifyOut)}};
    for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    uint64_t *d_keys = (uint64_t *)keys.p;
    uint32_t *d_vals = (uint32_t *)vals.p, *d_valence = (uint32_t *)valence.p, *d_vclass = (uint32_t *)vclass.p;
    float4 *d_rec = (float4 *)rec.p;
    SimplifyOut *d_out = (SimplifyOut *)counters.p;
    const unsigned b = bits_for_value(n - 1);                   // <= 32: an edge key has 2 b <= 64 bits
    TC_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, sizeof(SimplifyOut), st));
    TC_HIP_TRY(ctx, hipMemsetAsync(d_valence, 0, n * sizeof(uint32_t), st));
    TC_HIP_TRY(ctx, hipMemsetAsync(d_vclass, 0, n * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "simplify_classes");
        hipLaunchKernelGGL(simp_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, st, a.xyz, (uint32_t)n, d_rec, &d_out->flags);
        hipLaunchKernelGGL(simp_edge_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (uint32_t)m, (uint32_t)n, (uint32_t)b, d_keys, d_vals, d_valence,
                           &d_out->flags);
        if (!copy) {
            KeyGroups edges;
            if (tc_status s = group_by_key(ctx, d_keys, d_vals, nk, 2u * b, group, edges, big)) return s;
            hipLaunchKernelGGL(simp_edge_class_kernel, dim3(blocks_for(nk)), dim3(256), 0, st, edges.keys_sorted, edges.order, (const uint32_t *)edges.head,
                               (uint32_t)nk, (uint32_t)b, (uint32_t)n, a.faces, (const float4 *)d_rec, cosf(cfg.feature_angle_threshold),
                               (const uint32_t *)&d_out->flags, d_vclass);
        }
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    if (!copy) if (tc_status s = cloud_bbox(ctx, a.xyz, n, mn, mx)) return s;            // the first wait: the box
    SimplifyOut *h = &pinned_host(ctx)->simplify_out;
    if (tc_status s = read_back(ctx, h, d_out, sizeof(SimplifyOut))) return s;           // the second: the flags
    if (h->flags & kSimpBadIndex) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: a face index is >= n_vertices");
    if (h->flags & kSimpNotFinite) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: a vertex coordinate is not finite");
    if (copy) {                                                 // clustering.rs:794-796: mesh.clone()
        *n_out_vertices = n; *n_out_faces = m;
        if (!a.any_output()) return TC_OK;
        if (tc_status s = simp_check_caps(ctx, a, n, m)) return s;
        if (a.out_xyz) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_xyz, a.xyz, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (a.out_nrm) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_nrm, a.normals, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (a.out_rgb) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_rgb, a.colors, n * 3, hipMemcpyDeviceToDevice, st));
        if (a.out_faces) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_faces, a.faces, m * 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (a.out_map) hipLaunchKernelGGL(simp_identity_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (uint32_t)n, a.out_map);
        TC_HIP_TRY(ctx, hipGetLastError());
        return synced(ctx);
    }
    SimpCells cells;
    if (tc_status s = simp_cell_size(ctx, mn, mx, n, cfg.reduction_ratio, cells)) return s;

    const std::pair<ScopedBuf *, size_t> need2[] = {
        {&cluster_of, n * sizeof(uint32_t)}, {&long_list, list_cap * sizeof(uint32_t)}, {&rep, n * sizeof(float4)}, {&nrm, (a.normals ? n : 1) * sizeof(float4)},
        {&col, (a.colors ? n : 1) * sizeof(uint32_t)}, {&keep, m * sizeof(uint32_t)}, {&fpos, (m + 1) * sizeof(uint32_t)}, {&used, n * sizeof(uint32_t)},
        {&cpos, (n + 1) * sizeof(uint32_t)}};
    for (const auto &[buf, bytes] : need2) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    uint32_t *d_cluster_of = (uint32_t *)cluster_of.p, *d_long_list = (uint32_t *)long_list.p, *d_keep = (uint32_t *)keep.p, *d_fpos = (uint32_t *)fpos.p,
             *d_used = (uint32_t *)used.p, *d_cpos = (uint32_t *)cpos.p;
    // the cluster runs live in head / runpos / rstart from here on; the face stage has buffers of its own for its sort
    ScopedBuf fkeys, fkeys_sorted, fvals, fvals_sorted;
    SimpFold fold;                                              // (built once the cluster runs are there; simplify_write reads it again)
    {
        ProfScope ps(ctx, "simplify_clusters");
        hipLaunchKernelGGL(simp_vertex_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const float4 *)d_rec, (const uint32_t *)d_vclass, (uint32_t)n, cells,
                           cfg.preserve_boundary, d_keys, d_vals);
        KeyGroups clusters;
        if (tc_status s = group_by_key(ctx, d_keys, d_vals, n, 62u, group, clusters, big)) return s;
        fold = SimpFold{d_rec, d_valence, a.normals, a.colors, clusters.order, clusters.rstart, clusters.runpos, (float4 *)rep.p, (float4 *)nrm.p,
                        (uint32_t *)col.p, cfg.strategy == TC_SIMPLIFY_WEIGHTED_AVERAGE ? 1u : 0u, (uint32_t)n};
        hipLaunchKernelGGL(simp_cluster_of_kernel, dim3(blocks_for(n)), dim3(256), 0, st, clusters.order, (const uint32_t *)clusters.head,
                           (const uint32_t *)clusters.runpos, clusters.rstart, (uint32_t)n, d_cluster_of, d_long_list, (uint32_t)list_cap, &d_out->n_long);
        hipLaunchKernelGGL(simp_fold_kernel, dim3(blocks_for(n)), dim3(256), 0, st, fold);
        hipLaunchKernelGGL(simp_fold_long_kernel, dim3((unsigned)std::min<size_t>((list_cap + 3) / 4, kSimplifyLongBlocks)), dim3(256), 0, st, fold,
                           (const uint32_t *)d_long_list, (uint32_t)list_cap, (const uint32_t *)&d_out->n_long);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    {
        const std::pair<ScopedBuf *, size_t> need3[] = {{&fkeys, m * sizeof(uint64_t)}, {&fkeys_sorted, m * sizeof(uint64_t)}, {&fvals, m * sizeof(uint32_t)},
                                                        {&fvals_sorted, m * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need3) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    uint64_t *d_fkeys = (uint64_t *)fkeys.p, *d_fkeys_sorted = (uint64_t *)fkeys_sorted.p;
    uint32_t *d_fvals = (uint32_t *)fvals.p, *d_fvals_sorted = (uint32_t *)fvals_sorted.p;
    // cluster numbers are below n: three of them fit one key where 3 bits_for_value(n - 1) <= 64 (n <= 2^21)
    const unsigned bc = 3u * b <= 64u ? b : 0u;
    if (!bc) {
        const std::pair<ScopedBuf *, size_t> need4[] = {{&key32, m * sizeof(uint32_t)}, {&key32_sorted, m * sizeof(uint32_t)}, {&order1, m * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need4) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    TC_HIP_TRY(ctx, hipMemsetAsync(d_used, 0, n * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "simplify_faces");
        hipLaunchKernelGGL(simp_face_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (const uint32_t *)d_cluster_of, (uint32_t)m, (uint32_t)bc, d_fkeys,
                           (uint32_t *)key32.p, d_fvals);
        if (bc) {
            if (tc_status s = sort_pairs(ctx, (const uint64_t *)d_fkeys, d_fkeys_sorted, (const uint32_t *)d_fvals, d_fvals_sorted, m, 3u * bc, sort_temp)) return s;
        } else {
            uint32_t *d_order1 = (uint32_t *)order1.p;
            if (tc_status s = sort_pairs(ctx, (const uint32_t *)key32.p, (uint32_t *)key32_sorted.p, (const uint32_t *)d_fvals, d_order1, m, b, sort_temp)) return s;
            hipLaunchKernelGGL(simp_face_key2_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (const uint32_t *)d_cluster_of, (uint32_t)m,
                               (const uint32_t *)d_order1, d_fkeys);
            if (tc_status s = sort_pairs(ctx, (const uint64_t *)d_fkeys, d_fkeys_sorted, (const uint32_t *)d_order1, d_fvals_sorted, m, 32u + b, sort_temp)) return s;
        }
        hipLaunchKernelGGL(simp_face_keep_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (const uint32_t *)d_cluster_of, (uint32_t)m,
                           (const uint32_t *)d_fvals_sorted, d_keep);
        if (tc_status s = exclusive_scan_u32(ctx, d_keep, (uint32_t)m, d_fpos, blocksum)) return s;
        hipLaunchKernelGGL(simp_mark_used_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (const uint32_t *)d_cluster_of, (uint32_t)m, (const uint32_t *)d_keep,
                           d_used);
        if (tc_status s = exclusive_scan_u32(ctx, d_used, (uint32_t)n, d_cpos, blocksum)) return s;
        hipLaunchKernelGGL(simp_counts_kernel, dim3(1), dim3(1), 0, st, (const uint32_t *)(d_cpos + n), (const uint32_t *)(d_fpos + m), d_out);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = read_back(ctx, h, d_out, sizeof(SimplifyOut))) return s;           // the third wait: the counts
    const size_t nv = h->n_out_vertices, nf = h->n_out_faces;
    *n_out_vertices = nv; *n_out_faces = nf;
    if (!a.any_output()) return TC_OK;
    if (tc_status s = simp_check_caps(ctx, a, nv, nf)) return s;
    {
        ProfScope ps(ctx, "simplify_write");
        if (a.out_xyz || a.out_nrm || a.out_rgb)
            hipLaunchKernelGGL(simp_write_vertices_kernel, dim3(blocks_for(n)), dim3(256), 0, st, fold, (const uint32_t *)d_used, (const uint32_t *)d_cpos, a.out_xyz,
                               a.out_nrm, a.out_rgb);
        if (a.out_faces)
            hipLaunchKernelGGL(simp_write_faces_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (const uint32_t *)d_cluster_of, (uint32_t)m,
                               (const uint32_t *)d_keep, (const uint32_t *)d_fpos, (const uint32_t *)d_cpos, a.out_faces);
        if (a.out_map)
            hipLaunchKernelGGL(simp_write_map_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t *)d_cluster_of, (uint32_t)n, (const uint32_t *)d_used,
                               (const uint32_t *)d_cpos, a.out_map);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_simplify.h) -----------------------------------------------------------------------
// the header's checks (1) to (5), in its order
static tc_status simplify_check(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces, const float *normals,
                                const uint8_t *colors, const tc_simplify_config *cfg, float *out_normals, uint8_t *out_colors, size_t *n_out_vertices,
                                size_t *n_out_faces) {
    if (!ctx) return TC_INVALID_DATA;
    if (!vertices) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: vertices is NULL");
    if (!faces) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: faces is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: config is NULL");
    if (!n_out_vertices || !n_out_faces) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: a count pointer is NULL");
    if ((normals != nullptr) != (out_normals != nullptr)) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: out_normals goes with normals, both or neither");
    if ((colors != nullptr) != (out_colors != nullptr)) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: out_colors goes with colors, both or neither");
    if (n_vertices == 0 || n_faces == 0) return fail(ctx, TC_INVALID_DATA, "Mesh is empty");                               // clustering.rs:786-788
    if (cfg->strategy > TC_SIMPLIFY_WEIGHTED_AVERAGE) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: strategy is neither centroid (0) nor weighted average (1)");
    if (cfg->preserve_boundary > 1u) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: preserve_boundary is neither 0 nor 1");
    if (!(cfg->reduction_ratio >= 0.0f && cfg->reduction_ratio <= 1.0f)) return fail(ctx, TC_INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0");   // :789-793
    if (!std::isfinite(cfg->feature_angle_threshold)) return fail(ctx, TC_INVALID_DATA, "simplify_clustering: feature_angle_threshold is not finite");
    if (n_vertices >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "simplify_clustering: n_vertices is 2^32 - 16 or more");
    if (n_faces >= (kMaxPoints + 2) / 3) return fail(ctx, TC_UNSUPPORTED, "simplify_clustering: 3 n_faces is 2^32 - 16 or more");
    return TC_OK;
}

extern "C" {

void tc_simplify_config_default(float reduction_ratio, tc_simplify_config *cfg) try {
    if (!cfg) return;
    cfg->strategy = TC_SIMPLIFY_CENTROID;
    cfg->preserve_boundary = 1u;
    cfg->feature_angle_threshold = 0.785398185253143310546875f;            // 45.0f32.to_radians(): 45 * (pi / 180) in f32, 0x3F490FDB
    cfg->reduction_ratio = reduction_ratio;
} TC_CATCH_VOID

tc_status tc_simplify_clustering_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                        const float *normals, const uint8_t *colors, const tc_simplify_config *cfg, float *out_vertices,
                                        float *out_normals, uint8_t *out_colors, size_t cap_vertices, uint32_t *out_faces,
                                        size_t cap_faces, uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces) try {
    if (tc_status s = simplify_check(ctx, vertices, n_vertices, faces, n_faces, normals, colors, cfg, out_normals, out_colors, n_out_vertices, n_out_faces)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const SimpCall call{vertices, n_vertices, faces, n_faces, normals, colors, out_vertices, out_normals, out_colors, cap_vertices, out_faces, cap_faces, out_vertex_map};
    return simplify_on_device(ctx, call, *cfg, n_out_vertices, n_out_faces);
} TC_CATCH_STATUS(ctx)

tc_status tc_simplify_clustering(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                 const float *normals, const uint8_t *colors, const tc_simplify_config *cfg, float *out_vertices,
                                 float *out_normals, uint8_t *out_colors, size_t cap_vertices, uint32_t *out_faces, size_t cap_faces,
                                 uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces) try {
    if (tc_status s = simplify_check(ctx, vertices, n_vertices, faces, n_faces, normals, colors, cfg, out_normals, out_colors, n_out_vertices, n_out_faces)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = n_vertices, m = n_faces;
    ScopedBuf d_colors, o_xyz, o_nrm, o_rgb, o_faces, o_map;
    if (tc_status s = stage_in(ctx, ctx->in_a, vertices, n * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, faces, m * 3 * sizeof(uint32_t))) return s;
    if (normals) if (tc_status s = stage_in(ctx, ctx->in_c, normals, n * 3 * sizeof(float))) return s;
    if (colors) if (tc_status s = stage_in(ctx, d_colors, colors, n * 3)) return s;
    // the device-side outputs are as large as the counts can get, whatever the caller's capacities: the capacity check is the caller's
    if (out_vertices) if (tc_status s = ensure(ctx, o_xyz, n * 3 * sizeof(float))) return s;
    if (out_normals) if (tc_status s = ensure(ctx, o_nrm, n * 3 * sizeof(float))) return s;
    if (out_colors) if (tc_status s = ensure(ctx, o_rgb, n * 3)) return s;
    if (out_faces) if (tc_status s = ensure(ctx, o_faces, m * 3 * sizeof(uint32_t))) return s;
    if (out_vertex_map) if (tc_status s = ensure(ctx, o_map, n * sizeof(uint32_t))) return s;
    const SimpCall call{(const float *)ctx->in_a.p, n, (const uint32_t *)ctx->in_b.p, m, normals ? (const float *)ctx->in_c.p : nullptr,
                        colors ? (const uint8_t *)d_colors.p : nullptr, (float *)o_xyz.p, (float *)o_nrm.p, (uint8_t *)o_rgb.p, cap_vertices, (uint32_t *)o_faces.p,
                        cap_faces, (uint32_t *)o_map.p};
    if (tc_status s = simplify_on_device(ctx, call, *cfg, n_out_vertices, n_out_faces)) return s;          // (a capacity failure has set the counts)
    if (!call.any_output()) return TC_OK;
    const size_t nv = *n_out_vertices, nf = *n_out_faces;
    if (out_vertices && nv) TC_HIP_TRY(ctx, hipMemcpyAsync(out_vertices, o_xyz.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_normals && nv) TC_HIP_TRY(ctx, hipMemcpyAsync(out_normals, o_nrm.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_colors && nv) TC_HIP_TRY(ctx, hipMemcpyAsync(out_colors, o_rgb.p, nv * 3, hipMemcpyDeviceToHost, st));
    if (out_faces && nf) TC_HIP_TRY(ctx, hipMemcpyAsync(out_faces, o_faces.p, nf * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_vertex_map) TC_HIP_TRY(ctx, hipMemcpyAsync(out_vertex_map, o_map.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return synced(ctx);                                         // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

}  // extern "C"
