// qem.hip -- simplify a triangle mesh by quadric-error edge collapse in rounds (QuadricErrorSimplifier,
// threecrate-simplification/src/quadric_error.rs); the entry points of include/threecrate_hip_qem.h, which pins the arithmetic and the order
// of everything.  This unit is the whole of the companion library libthreecrate_hip_qem.so; the host layer of tc_internal.h (ensure,
// stage_in, read_back, group_by_key, sort_pairs, exclusive_scan_u32, ProfScope) resolves from libthreecrate_hip.so.
//   The set-up, one profile row (qem_setup):
//   qem_pack          a thread per vertex: its 16-byte record (x, y, z, 0); a coordinate that is not finite raises flag bit 1
//   qem_face_check    a thread per face: keep = its three indices differ; an index >= n raises flag bit 0 (and the face is not kept)
//   exclusive_scan_u32 + qem_face_compact   the kept faces, in input order, into the working face list
//   -- one read-back: the flags and alive --
//   qem_plane         a thread per alive face: its plane (header (3)) as four floats; the keys (vertex) and values (3 f + corner) of its corners
//   group_by_key      one run per referenced vertex, its corners in ascending face index
//   qem_ring_list     the runs of more than kQemLongRing corners, listed
//   qem_fold          a lane per run of at most kQemLongRing corners: the ten f64 sums of header (4), fold_run_lane
//   qem_fold_long     a wave per listed run: fold_run_wave, the same bits
//   A round, one profile row (qem_round), every launch sized by the face count the host read after the round before:
//   qem_edge_emit     a thread per alive face: its three undirected edges as packed keys lo << b | hi (b = bits_for_value(n - 1): the
//                     order of lo << 32 | hi with fewer sort passes)
//   group_by_key      one run per unique edge; a run's length is the edge's multiplicity.  A unique edge is named by the sorted position p
//                     of its run's head: ascending p is ascending (lo, hi)
//   qem_boundary      a thread per position: the head of a run of one stores 1 at both ends (every writer stores the same word)
//   qem_cost          a thread per position, f64: a head decides (5c), solves (5d), prices (5e); the cost key goes to cost[p], the position
//                     to where[p], and a 64-bit atomicMin of the key to both ends
//   qem_claim         the edges whose key equals an end's minimum: a 32-bit atomicMin of p at that end
//   qem_win           an edge wins when it holds both ends
//   exclusive_scan_u32 + qem_win_scatter   the winners, in ascending p, into a list of min(n / 2, 3 alive) slots pre-filled with the largest key
//   sort_pairs        by cost key, all 64 bits.  rocPRIM's radix sort is stable, the winners went in by ascending p and the filler (key
//                     2^64 - 1, which no cost maps to: it is the key of a NaN, and a NaN is no candidate) sorts behind them: equal keys keep
//                     ascending (lo, hi), the rank of the header
//   qem_mult + exclusive_scan_u32   the multiplicities in rank order and their prefix sums: winner i is taken when the sum before it is below
//                     alive - target
//   qem_apply         a thread per taken edge: position and quadric of lo, parent[hi] = lo; the last taken one stores the count
//   qem_face_remap    a thread per alive face: its indices through parent (one step: both ends of a taken edge were alive, and no vertex is
//                     in two taken edges), keep = they still differ
//   exclusive_scan_u32 + qem_face_compact   the survivors into the other face list; alive
//   -- one read-back per round: alive and the number taken --
//   The write-out (qem_write): qem_mark_used, exclusive_scan_u32, -- one read-back: the vertex count --, qem_write_vertices / _faces / _map
// Host waits of a call: the flags, one per round run (the round that takes nothing included), the vertex count, and the final drain.
// Atomics: integer only (atomicOr of a flag, atomicAdd of a list counter, atomicMin of keys and positions: each result is the same whatever
// the order).  No f64 atomic anywhere: every f64 sum has the order of the header.
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_qem.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// A vertex with more incident faces than this has its quadric folded by a wave (qem_fold_long).  TC_QEM_LONG_RING: the A/B builds of
// `make qem-ab` (variants/, what tools/qem_bench.py --ring loads); never the product.  128 is mesh.hip's kMeshLongRing, measured on the same
// two roads of run_fold.h with another record: the crossing of THIS fold (a 16-byte plane gathered per corner, ten products and ten f64
// adds) has not been measured (STATE.md).
#ifdef TC_QEM_LONG_RING
constexpr uint32_t kQemLongRing = TC_QEM_LONG_RING;
#else
constexpr uint32_t kQemLongRing = 128;
#endif
constexpr int kQemLongBlocks = 1024;            // the wave-per-run kernel's grid is fixed (the list's length stays on the device); its waves stride
constexpr uint32_t kQemBadIndex = 1u, kQemNotFinite = 2u;       // QemOut::flags
constexpr uint64_t kQemNoCandidate = ~0ull;     // cost[p] of an edge that is no candidate; also the filler of the winners' list
constexpr float kF32Max = 3.4028234664e38f;
constexpr double kF64Max = 1.7976931348623157e308;

// the quadric of a vertex: aa ab ac ad bb bc bd cc cd dd = q00 q01 q02 q03 q11 q12 q13 q22 q23 q33
struct Quadric { double q[10]; };

// the ten running sums of one vertex, the header's (4): every add is one product and one sum
struct QemAcc {
    double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    __device__ __forceinline__ void add(const float4 &pl) {
        const double a = (double)pl.x, b = (double)pl.y, c = (double)pl.z, d = (double)pl.w;
        const double aa = a * a, ab = a * b, ac = a * c, ad = a * d, bb = b * b, bc = b * c, bd = b * d, cc = c * c, cd = c * d, dd = d * d;
        q[0] = q[0] + aa; q[1] = q[1] + ab; q[2] = q[2] + ac; q[3] = q[3] + ad; q[4] = q[4] + bb;
        q[5] = q[5] + bc; q[6] = q[6] + bd; q[7] = q[7] + cc; q[8] = q[8] + cd; q[9] = q[9] + dd;
    }
};

__device__ __forceinline__ bool finite_f32(float v) { return fabsf(v) <= kF32Max; }      // false for NaN

__global__ void __launch_bounds__(256) qem_pack_kernel(const float *__restrict__ xyz, uint32_t n, float4 *__restrict__ rec, uint32_t *__restrict__ flags) {
    pack_xyz_records<true>(xyz, n, rec, flags, kQemNotFinite);
}

__global__ void __launch_bounds__(256) qem_identity_kernel(uint32_t n, uint32_t *__restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) map[i] = i;
}

__global__ void __launch_bounds__(256) qem_face_check_kernel(const uint32_t *__restrict__ faces, uint32_t m, uint32_t n, uint32_t *__restrict__ keep,
                                                            uint32_t *__restrict__ flags) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (f < m) {
        const uint32_t a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
        bad = a >= n || b >= n || c >= n;
        keep[f] = (!bad && a != b && b != c && c != a) ? 1u : 0u;           // (a bad face is never followed: the call fails)
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flags, kQemBadIndex);
}

// the kept faces of `in` (count of them) to their scanned positions in `out`; pos[count] = the number kept, stored into *alive
__global__ void __launch_bounds__(256) qem_face_compact_kernel(const uint32_t *__restrict__ in, uint32_t count, const uint32_t *__restrict__ keep,
                                                              const uint32_t *__restrict__ pos, uint32_t *__restrict__ out, uint32_t *__restrict__ alive) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f == 0u) *alive = pos[count];
    if (f >= count || !keep[f]) return;
    const size_t o = pos[f];                                    // <= f: inside `out`, which has the room of `in`
#pragma unroll
    for (int k = 0; k < 3; ++k) out[3 * o + k] = in[3 * (size_t)f + k];
}

// the header's (3), and the corners of the face for the grouping by vertex
__global__ void __launch_bounds__(256) qem_plane_kernel(const uint32_t *__restrict__ faces, uint32_t alive, const float4 *__restrict__ rec,
                                                       float4 *__restrict__ plane, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= alive) return;
    const uint32_t i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    const float4 v0 = rec[i0], v1 = rec[i1], v2 = rec[i2];
    const float ax = v1.x - v0.x, ay = v1.y - v0.y, az = v1.z - v0.z;
    const float bx = v2.x - v0.x, by = v2.y - v0.y, bz = v2.z - v0.z;
    const float p0 = ay * bz, p1 = az * by, p2 = az * bx, p3 = ax * bz, p4 = ax * by, p5 = ay * bx;
    const float cx = p0 - p1, cy = p2 - p3, cz = p4 - p5;
    const float xx = cx * cx, yy = cy * cy, zz = cz * cz;
    const float len = sqrtf((xx + yy) + zz);
    const float nx = cx / len, ny = cy / len, nz = cz / len;
    float4 pl = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
    if (finite_f32(nx) && finite_f32(ny) && finite_f32(nz)) {
        const float dx = nx * v0.x, dy = ny * v0.y, dz = nz * v0.z;
        pl = make_float4(nx, ny, nz, -((dx + dy) + dz));
    }
    plane[f] = pl;
    const uint32_t v[3] = {i0, i1, i2};
#pragma unroll
    for (int k = 0; k < 3; ++k) { keys[3 * (size_t)f + k] = (uint64_t)v[k]; vals[3 * (size_t)f + k] = 3u * f + (uint32_t)k; }
}

// what the two folds read and write
struct QemFold {
    const float4 *plane;        // per alive face
    const uint64_t *keys_sorted;    // the vertex of every sorted corner
    const uint32_t *corners;    // 3 f + corner, run by run, ascending inside a run
    const uint32_t *rstart;     // first corner of every run, rstart[R] = nk
    const uint32_t *n_runs;     // R
    Quadric *quadric;           // per vertex
    uint32_t nk;
};

__global__ void __launch_bounds__(256) qem_ring_list_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ rstart,
                                                           uint32_t nk, uint32_t *__restrict__ long_list, uint32_t list_cap, uint32_t *__restrict__ n_long) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nk || !head[p]) return;
    const uint32_t r = runpos[p];                               // the heads before p: p's own run
    if (rstart[r + 1] - p > kQemLongRing) append_long_run(long_list, list_cap, n_long, r);
}

__device__ __forceinline__ void qem_store_quadric(const QemFold &a, uint32_t s, const QemAcc &acc) {
    Quadric out;
#pragma unroll
    for (int k = 0; k < 10; ++k) out.q[k] = acc.q[k];
    a.quadric[(uint32_t)a.keys_sorted[s]] = out;                // the run's vertex, < n: it came out of a checked face
}

__global__ void __launch_bounds__(256) qem_fold_kernel(QemFold a) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.nk || r >= *a.n_runs) return;
    const uint32_t s = a.rstart[r], e = a.rstart[r + 1];
    if (e - s > kQemLongRing) return;                           // (a long ring is folded by its wave)
    QemAcc acc;
    fold_run_lane<4>(s, e, [&](uint32_t j) { return a.plane[a.corners[j] / 3u]; }, [&](const float4 &pl) { acc.add(pl); });
    qem_store_quadric(a, s, acc);
}

__global__ void __launch_bounds__(256) qem_fold_long_kernel(QemFold a, const uint32_t *__restrict__ long_list, uint32_t list_cap, const uint32_t *__restrict__ n_long_p) {
    const uint32_t lane = threadIdx.x & 63u;
    for_each_listed_run(long_list, min(*n_long_p, list_cap), [&](uint32_t r) {
        const uint32_t s = a.rstart[r], e = a.rstart[r + 1];
        QemAcc acc;                                             // every lane runs the same chain
        fold_run_wave(s, e, lane, [&](uint32_t j) { return a.plane[a.corners[j] / 3u]; }, [&](const float4 &pl) { acc.add(pl); });
        if (lane == 0u) qem_store_quadric(a, s, acc);
    });
}

__global__ void __launch_bounds__(256) qem_edge_emit_kernel(const uint32_t *__restrict__ faces, uint32_t alive, uint32_t b, uint64_t *__restrict__ keys,
                                                           uint32_t *__restrict__ vals) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= alive) return;
    const uint32_t v[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t p = v[k], q = v[k == 2 ? 0 : k + 1];
        keys[3 * (size_t)f + k] = ((uint64_t)min(p, q) << b) | (uint64_t)max(p, q);
        vals[3 * (size_t)f + k] = 3u * f + (uint32_t)k;
    }
}

// the unique edges of a round, as group_by_key left them, and what the round's kernels keep per edge (indexed by the head's position)
struct QemEdges {
    const uint64_t *keys_sorted;
    const uint32_t *head, *runpos, *rstart;
    uint32_t nk, b, n;
    __device__ __forceinline__ void ends(uint32_t p, uint32_t &lo, uint32_t &hi) const {
        const uint64_t key = keys_sorted[p];
        lo = (uint32_t)(key >> b); hi = (uint32_t)(key & ((1ull << b) - 1ull));          // b <= 32; both < n
    }
    __device__ __forceinline__ uint32_t multiplicity(uint32_t p) const { return rstart[runpos[p] + 1u] - p; }
};

__global__ void __launch_bounds__(256) qem_boundary_kernel(QemEdges e, uint32_t *__restrict__ boundary) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= e.nk || !e.head[p]) return;
    if (!(p + 1u >= e.nk || e.head[p + 1u])) return;            // a run of more than one
    uint32_t lo, hi;
    e.ends(p, lo, hi);
    if (lo >= e.n || hi >= e.n) return;                         // (never: the keys were built from checked indices)
    boundary[lo] = 1u; boundary[hi] = 1u;                       // every writer stores the same word
}

// the monotone map of f64::total_cmp to u64
__device__ __forceinline__ uint64_t qem_cost_key(double cost) {
    const uint64_t bits = (uint64_t)__double_as_longlong(cost);
    return (bits >> 63) ? ~bits : (bits | 0x8000000000000000ull);
}

// the header's (5c), (5d) and (5e) for the edge at head position p
__global__ void __launch_bounds__(256) qem_cost_kernel(QemEdges e, const uint32_t *__restrict__ boundary, const float4 *__restrict__ rec,
                                                      const Quadric *__restrict__ quadric, float max_edge_length, uint64_t *__restrict__ cost,
                                                      float4 *__restrict__ where, unsigned long long *__restrict__ vmin) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= e.nk || !e.head[p]) return;
    cost[p] = kQemNoCandidate;
    uint32_t lo, hi;
    e.ends(p, lo, hi);
    if (lo >= e.n || hi >= e.n) return;                         // (never)
    if (boundary && (boundary[lo] | boundary[hi])) return;
    const float4 pl = rec[lo], ph = rec[hi];
    if (max_edge_length > 0.0f) {
        const float dx = pl.x - ph.x, dy = pl.y - ph.y, dz = pl.z - ph.z;
        const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
        if (sqrtf((xx + yy) + zz) > max_edge_length) return;
    }
    const Quadric ql = quadric[lo], qh = quadric[hi];
    double q[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) q[k] = ql.q[k] + qh.q[k];
    const double a00 = q[0], a01 = q[1], a02 = q[2], b0 = q[3], a11 = q[4], a12 = q[5], b1 = q[6], a22 = q[7], b2 = q[8], q33 = q[9];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    bool solved = det != 0.0 && fabs(det) <= kF64Max;
    if (solved) {
        const double sx = -(((c00 * b0 + c01 * b1) + c02 * b2) / det);
        const double sy = -(((c01 * b0 + c11 * b1) + c12 * b2) / det);
        const double sz = -(((c02 * b0 + c12 * b1) + c22 * b2) / det);
        x = (float)sx; y = (float)sy; z = (float)sz;
        solved = finite_f32(x) && finite_f32(y) && finite_f32(z);
    }
    if (!solved) { x = (pl.x + ph.x) * 0.5f; y = (pl.y + ph.y) * 0.5f; z = (pl.z + ph.z) * 0.5f; }
    const double X = (double)x, Y = (double)y, Z = (double)z;
    const double r0 = ((a00 * X + a01 * Y) + a02 * Z) + b0;
    const double r1 = ((a01 * X + a11 * Y) + a12 * Z) + b1;
    const double r2 = ((a02 * X + a12 * Y) + a22 * Z) + b2;
    const double r3 = ((b0 * X + b1 * Y) + b2 * Z) + q33;
    const double c = ((X * r0 + Y * r1) + Z * r2) + r3;
    if (c != c) return;                                         // a NaN cost: no candidate
    const uint64_t key = qem_cost_key(c);
    cost[p] = key;
    where[p] = make_float4(x, y, z, 0.0f);
    atomicMin(&vmin[lo], (unsigned long long)key);              // integer minima: no order shows
    atomicMin(&vmin[hi], (unsigned long long)key);
}

__global__ void __launch_bounds__(256) qem_claim_kernel(QemEdges e, const uint64_t *__restrict__ cost, const unsigned long long *__restrict__ vmin,
                                                       uint32_t *__restrict__ vwin) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= e.nk || !e.head[p]) return;
    const uint64_t key = cost[p];
    if (key == kQemNoCandidate) return;
    uint32_t lo, hi;
    e.ends(p, lo, hi);
    if (vmin[lo] == key) atomicMin(&vwin[lo], p);
    if (vmin[hi] == key) atomicMin(&vwin[hi], p);
}

__global__ void __launch_bounds__(256) qem_win_kernel(QemEdges e, const uint64_t *__restrict__ cost, const uint32_t *__restrict__ vwin, uint32_t *__restrict__ win) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= e.nk) return;
    uint32_t w = 0u;
    if (e.head[p] && cost[p] != kQemNoCandidate) {
        uint32_t lo, hi;
        e.ends(p, lo, hi);
        w = (vwin[lo] == p && vwin[hi] == p) ? 1u : 0u;
    }
    win[p] = w;
}

__global__ void __launch_bounds__(256) qem_win_scatter_kernel(uint32_t nk, const uint32_t *__restrict__ win, const uint32_t *__restrict__ wpos,
                                                             const uint64_t *__restrict__ cost, uint32_t cap, uint64_t *__restrict__ wkeys,
                                                             uint32_t *__restrict__ wvals) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nk || !win[p]) return;
    const uint32_t o = wpos[p];
    if (o >= cap) return;                                       // (never: winners share no vertex and are unique edges, cap = min(n / 2, nk))
    wkeys[o] = cost[p]; wvals[o] = p;
}

// the winners in rank order: their multiplicities (0 behind the last winner)
__global__ void __launch_bounds__(256) qem_mult_kernel(QemEdges e, const uint32_t *__restrict__ n_win, uint32_t cap, const uint32_t *__restrict__ wvals_sorted,
                                                      uint32_t *__restrict__ wmult) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    uint32_t c = 0u;
    if (i < min(*n_win, cap)) {
        const uint32_t p = wvals_sorted[i];
        if (p < e.nk) c = e.multiplicity(p);
    }
    wmult[i] = c;
}

// the header's (5f) cut and (5g) for winner i
__global__ void __launch_bounds__(256) qem_apply_kernel(QemEdges e, const uint32_t *__restrict__ n_win, uint32_t cap, const uint32_t *__restrict__ wvals_sorted,
                                                       const uint32_t *__restrict__ wcum, uint32_t need, const float4 *__restrict__ where,
                                                       float4 *__restrict__ rec, Quadric *__restrict__ quadric, uint32_t *__restrict__ parent,
                                                       uint32_t *__restrict__ taken) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t w = min(*n_win, cap);
    if (i >= w || wcum[i] >= need) return;                      // the faces removed before winner i already meet the budget
    if (i + 1u == w || wcum[i + 1u] >= need) *taken = i + 1u;   // the last one taken: one writer
    const uint32_t p = wvals_sorted[i];
    if (p >= e.nk) return;                                      // (never)
    uint32_t lo, hi;
    e.ends(p, lo, hi);
    if (lo >= e.n || hi >= e.n) return;                         // (never)
    const Quadric ql = quadric[lo], qh = quadric[hi];           // no other taken edge touches lo or hi
    Quadric sum;
#pragma unroll
    for (int k = 0; k < 10; ++k) sum.q[k] = ql.q[k] + qh.q[k];  // the sum qem_cost formed: the same two operands, the same bits
    quadric[lo] = sum;
    rec[lo] = where[p];
    parent[hi] = lo;
}

__global__ void __launch_bounds__(256) qem_face_remap_kernel(uint32_t *__restrict__ faces, uint32_t alive, const uint32_t *__restrict__ parent, uint32_t *__restrict__ keep) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= alive) return;
    const uint32_t a = parent[faces[3 * (size_t)f]], b = parent[faces[3 * (size_t)f + 1]], c = parent[faces[3 * (size_t)f + 2]];
    faces[3 * (size_t)f] = a; faces[3 * (size_t)f + 1] = b; faces[3 * (size_t)f + 2] = c;
    keep[f] = (a != b && b != c && c != a) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) qem_mark_used_kernel(const uint32_t *__restrict__ faces, uint32_t alive, uint32_t *__restrict__ used) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= alive) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) used[faces[3 * (size_t)f + k]] = 1u;        // every writer stores the same word
}

__global__ void qem_counts_kernel(const uint32_t *__restrict__ vpos_end, QemOut *__restrict__ out) { out->n_out_vertices = *vpos_end; }

__global__ void __launch_bounds__(256) qem_write_vertices_kernel(const float4 *__restrict__ rec, uint32_t n, const uint32_t *__restrict__ used,
                                                                const uint32_t *__restrict__ vpos, float *__restrict__ out_xyz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !used[i]) return;
    const size_t o = vpos[i];                                   // < the count the host has checked the capacity against
    const float4 r = rec[i];
    out_xyz[3 * o] = r.x; out_xyz[3 * o + 1] = r.y; out_xyz[3 * o + 2] = r.z;
}

__global__ void __launch_bounds__(256) qem_write_faces_kernel(const uint32_t *__restrict__ faces, uint32_t alive, const uint32_t *__restrict__ vpos,
                                                             uint32_t *__restrict__ out_faces) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= alive) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) out_faces[3 * (size_t)f + k] = vpos[faces[3 * (size_t)f + k]];
}

__global__ void __launch_bounds__(256) qem_write_map_kernel(const uint32_t *__restrict__ parent, uint32_t n, const uint32_t *__restrict__ used,
                                                           const uint32_t *__restrict__ vpos, uint32_t *__restrict__ map) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r = i;
    for (uint32_t up = parent[r]; up < r; up = parent[r]) r = up;           // a parent is smaller than its child: the chain ends at a root
    map[i] = used[r] ? vpos[r] : 0xFFFFFFFFu;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// a call's arrays, all device pointers (the entry points' arguments after staging)
struct QemCall {
    const float *xyz; size_t n; const uint32_t *faces; size_t m;
    float *out_xyz; size_t cap_vertices; uint32_t *out_faces; size_t cap_faces; uint32_t *out_map;
    bool any_output() const { return out_xyz || out_faces || out_map; }
};

static tc_status qem_check_caps(tc_context *ctx, const QemCall &a, size_t nv, size_t nf) {
    if (a.cap_vertices < nv) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: cap_vertices is smaller than the number of output vertices");
    if (a.cap_faces < nf) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: cap_faces is smaller than the number of output faces");
    return TC_OK;
}

// a validated call (the header's checks 1 to 5 made); device pointers
static tc_status qem_on_device(tc_context *ctx, const QemCall &a, const tc_qem_config &cfg, size_t *n_out_vertices, size_t *n_out_faces, uint32_t *n_rounds) {
    hipStream_t st = ctx->stream;
    const size_t n = a.n, m = a.m, nk = 3 * m;                  // n, nk < 2^32 - 16
    const size_t big = std::max(nk, n);
    const bool copy = cfg.reduction_ratio == 0.0f;
    const size_t target = (size_t)((1.0f - cfg.reduction_ratio) * (float)m);             // quadric_error.rs:428, f32
    const unsigned b = bits_for_value(n - 1);                   // <= 32: an edge key has 2 b <= 64 bits
    ScopedBuf counters, rec, keep, fpos, faces_a;
    {
        const std::pair<ScopedBuf *, size_t> need[] = {{&counters, sizeof(QemOut)}, {&rec, n * sizeof(float4)}, {&keep, m * sizeof(uint32_t)},
                                                       {&fpos, (m + 1) * sizeof(uint32_t)}, {&faces_a, nk * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    QemOut *d_out = (QemOut *)counters.p;
    float4 *d_rec = (float4 *)rec.p;
    uint32_t *d_keep = (uint32_t *)keep.p, *d_fpos = (uint32_t *)fpos.p;
    uint32_t *d_faces = (uint32_t *)faces_a.p;
    ScopedBuf blocksum;
    TC_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, sizeof(QemOut), st));
    {
        ProfScope ps(ctx, "qem_setup");
        hipLaunchKernelGGL(qem_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, st, a.xyz, (uint32_t)n, d_rec, &d_out->flags);
        hipLaunchKernelGGL(qem_face_check_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (uint32_t)m, (uint32_t)n, d_keep, &d_out->flags);
        if (!copy) {
            if (tc_status s = exclusive_scan_u32(ctx, d_keep, (uint32_t)m, d_fpos, blocksum)) return s;
            hipLaunchKernelGGL(qem_face_compact_kernel, dim3(blocks_for(m)), dim3(256), 0, st, a.faces, (uint32_t)m, (const uint32_t *)d_keep, (const uint32_t *)d_fpos,
                               d_faces, &d_out->alive);
        }
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    QemOut *h = &pinned_host(ctx)->qem_out;
    if (tc_status s = read_back(ctx, h, d_out, sizeof(QemOut))) return s;                // the first wait: the flags and alive
    if (h->flags & kQemBadIndex) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: a face index is >= n_vertices");
    if (h->flags & kQemNotFinite) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: a vertex coordinate is not finite");
    if (copy) {                                                 // quadric_error.rs:424-426: mesh.clone()
        *n_out_vertices = n; *n_out_faces = m;
        if (n_rounds) *n_rounds = 0u;
        if (!a.any_output()) return TC_OK;
        if (tc_status s = qem_check_caps(ctx, a, n, m)) return s;
        if (a.out_xyz) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_xyz, a.xyz, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (a.out_faces) TC_HIP_TRY(ctx, hipMemcpyAsync(a.out_faces, a.faces, m * 3 * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
        if (a.out_map) hipLaunchKernelGGL(qem_identity_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (uint32_t)n, a.out_map);
        TC_HIP_TRY(ctx, hipGetLastError());
        return synced(ctx);
    }
    size_t alive = h->alive;                                    // <= m

    // the scratch of the whole call, sized once for the first round (the largest): nothing below allocates inside the loop.  keys | values
    // and group_by_key's buffers serve the corners (3 alive, once), then every round's edges (3 alive)
    const size_t win_cap = std::min(n / 2, nk) + 1;             // winners share no vertex and are unique edges
    const size_t list_cap = nk / ((size_t)kQemLongRing + 1) + 1;
    ScopedBuf keys, keys_sorted, vals, vals_sorted, head, runpos, rstart, sort_temp;
    const GroupBufs group{keys_sorted, vals_sorted, head, runpos, rstart, sort_temp, blocksum};
    ScopedBuf faces_b, plane, long_list, quadric, parent, boundary, vmin, vwin, cost, where, win, wpos, wkeys, wkeys_sorted, wvals, wvals_sorted, wmult, wcum, used, vpos;
    {
        const std::pair<ScopedBuf *, size_t> need[] = {
            {&keys, big * sizeof(uint64_t)}, {&vals, big * sizeof(uint32_t)}, {&faces_b, nk * sizeof(uint32_t)}, {&plane, m * sizeof(float4)},
            {&long_list, list_cap * sizeof(uint32_t)}, {&quadric, n * sizeof(Quadric)}, {&parent, n * sizeof(uint32_t)}, {&boundary, n * sizeof(uint32_t)},
            {&vmin, n * sizeof(uint64_t)}, {&vwin, n * sizeof(uint32_t)}, {&cost, nk * sizeof(uint64_t)}, {&where, nk * sizeof(float4)},
            {&win, nk * sizeof(uint32_t)}, {&wpos, (nk + 1) * sizeof(uint32_t)}, {&wkeys, win_cap * sizeof(uint64_t)}, {&wkeys_sorted, win_cap * sizeof(uint64_t)},
            {&wvals, win_cap * sizeof(uint32_t)}, {&wvals_sorted, win_cap * sizeof(uint32_t)}, {&wmult, win_cap * sizeof(uint32_t)},
            {&wcum, (win_cap + 1) * sizeof(uint32_t)}, {&used, n * sizeof(uint32_t)}, {&vpos, (n + 1) * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    uint64_t *d_keys = (uint64_t *)keys.p, *d_cost = (uint64_t *)cost.p, *d_wkeys = (uint64_t *)wkeys.p, *d_wkeys_sorted = (uint64_t *)wkeys_sorted.p;
    uint32_t *d_vals = (uint32_t *)vals.p, *d_other = (uint32_t *)faces_b.p, *d_parent = (uint32_t *)parent.p, *d_boundary = (uint32_t *)boundary.p,
             *d_vwin = (uint32_t *)vwin.p, *d_win = (uint32_t *)win.p, *d_wpos = (uint32_t *)wpos.p, *d_wvals = (uint32_t *)wvals.p,
             *d_wvals_sorted = (uint32_t *)wvals_sorted.p, *d_wmult = (uint32_t *)wmult.p, *d_wcum = (uint32_t *)wcum.p, *d_used = (uint32_t *)used.p,
             *d_vpos = (uint32_t *)vpos.p, *d_long_list = (uint32_t *)long_list.p;
    unsigned long long *d_vmin = (unsigned long long *)vmin.p;
    float4 *d_plane = (float4 *)plane.p, *d_where = (float4 *)where.p;
    Quadric *d_quadric = (Quadric *)quadric.p;

    TC_HIP_TRY(ctx, hipMemsetAsync(d_quadric, 0, n * sizeof(Quadric), st));              // +0.0: a vertex in no face keeps it
    hipLaunchKernelGGL(qem_identity_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (uint32_t)n, d_parent);
    if (alive > 0) {
        ProfScope ps(ctx, "qem_setup");
        const size_t ak = 3 * alive;
        hipLaunchKernelGGL(qem_plane_kernel, dim3(blocks_for(alive)), dim3(256), 0, st, (const uint32_t *)d_faces, (uint32_t)alive, (const float4 *)d_rec, d_plane, d_keys,
                           d_vals);
        KeyGroups rings;
        if (tc_status s = group_by_key(ctx, d_keys, d_vals, ak, b, group, rings, big)) return s;
        const QemFold fold{d_plane, rings.keys_sorted, rings.order, rings.rstart, rings.n_runs, d_quadric, (uint32_t)ak};
        hipLaunchKernelGGL(qem_ring_list_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, (const uint32_t *)rings.head, (const uint32_t *)rings.runpos, rings.rstart,
                           (uint32_t)ak, d_long_list, (uint32_t)list_cap, &d_out->n_long);
        hipLaunchKernelGGL(qem_fold_kernel, dim3(blocks_for(std::min(ak, n))), dim3(256), 0, st, fold);
        hipLaunchKernelGGL(qem_fold_long_kernel, dim3((unsigned)std::min<size_t>((list_cap + 3) / 4, kQemLongBlocks)), dim3(256), 0, st, fold,
                           (const uint32_t *)d_long_list, (uint32_t)list_cap, (const uint32_t *)&d_out->n_long);
    }
    TC_HIP_TRY(ctx, hipGetLastError());

    uint32_t rounds = 0;
    while (alive > target) {
        ProfScope ps(ctx, "qem_round");
        const size_t ak = 3 * alive;
        const size_t cap = std::min(n / 2, ak);                 // >= 1: an alive face has three distinct vertices
        const uint32_t need_faces = (uint32_t)(alive - target);
        hipLaunchKernelGGL(qem_edge_emit_kernel, dim3(blocks_for(alive)), dim3(256), 0, st, (const uint32_t *)d_faces, (uint32_t)alive, (uint32_t)b, d_keys, d_vals);
        KeyGroups runs;
        if (tc_status s = group_by_key(ctx, d_keys, d_vals, ak, 2u * b, group, runs, big)) return s;
        const QemEdges edges{runs.keys_sorted, runs.head, runs.runpos, runs.rstart, (uint32_t)ak, (uint32_t)b, (uint32_t)n};
        if (cfg.preserve_boundary) {
            TC_HIP_TRY(ctx, hipMemsetAsync(d_boundary, 0, n * sizeof(uint32_t), st));
            hipLaunchKernelGGL(qem_boundary_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, edges, d_boundary);
        }
        TC_HIP_TRY(ctx, hipMemsetAsync(d_vmin, 0xFF, n * sizeof(uint64_t), st));
        TC_HIP_TRY(ctx, hipMemsetAsync(d_vwin, 0xFF, n * sizeof(uint32_t), st));
        TC_HIP_TRY(ctx, hipMemsetAsync(d_wkeys, 0xFF, cap * sizeof(uint64_t), st));
        TC_HIP_TRY(ctx, hipMemsetAsync(&d_out->taken, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(qem_cost_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, edges, cfg.preserve_boundary ? (const uint32_t *)d_boundary : nullptr,
                           (const float4 *)d_rec, (const Quadric *)d_quadric, cfg.max_edge_length, d_cost, d_where, d_vmin);
        hipLaunchKernelGGL(qem_claim_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, edges, (const uint64_t *)d_cost, (const unsigned long long *)d_vmin, d_vwin);
        hipLaunchKernelGGL(qem_win_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, edges, (const uint64_t *)d_cost, (const uint32_t *)d_vwin, d_win);
        if (tc_status s = exclusive_scan_u32(ctx, d_win, (uint32_t)ak, d_wpos, blocksum)) return s;
        const uint32_t *d_n_win = d_wpos + ak;
        hipLaunchKernelGGL(qem_win_scatter_kernel, dim3(blocks_for(ak)), dim3(256), 0, st, (uint32_t)ak, (const uint32_t *)d_win, (const uint32_t *)d_wpos,
                           (const uint64_t *)d_cost, (uint32_t)cap, d_wkeys, d_wvals);
        if (tc_status s = sort_pairs(ctx, (const uint64_t *)d_wkeys, d_wkeys_sorted, (const uint32_t *)d_wvals, d_wvals_sorted, cap, 64u, sort_temp)) return s;
        hipLaunchKernelGGL(qem_mult_kernel, dim3(blocks_for(cap)), dim3(256), 0, st, edges, d_n_win, (uint32_t)cap, (const uint32_t *)d_wvals_sorted, d_wmult);
        if (tc_status s = exclusive_scan_u32(ctx, d_wmult, (uint32_t)cap, d_wcum, blocksum)) return s;
        hipLaunchKernelGGL(qem_apply_kernel, dim3(blocks_for(cap)), dim3(256), 0, st, edges, d_n_win, (uint32_t)cap, (const uint32_t *)d_wvals_sorted,
                           (const uint32_t *)d_wcum, need_faces, (const float4 *)d_where, d_rec, d_quadric, d_parent, &d_out->taken);
        hipLaunchKernelGGL(qem_face_remap_kernel, dim3(blocks_for(alive)), dim3(256), 0, st, d_faces, (uint32_t)alive, (const uint32_t *)d_parent, d_keep);
        if (tc_status s = exclusive_scan_u32(ctx, d_keep, (uint32_t)alive, d_fpos, blocksum)) return s;
        hipLaunchKernelGGL(qem_face_compact_kernel, dim3(blocks_for(alive)), dim3(256), 0, st, (const uint32_t *)d_faces, (uint32_t)alive, (const uint32_t *)d_keep,
                           (const uint32_t *)d_fpos, d_other, &d_out->alive);
        TC_HIP_TRY(ctx, hipGetLastError());
        if (tc_status s = read_back(ctx, h, d_out, sizeof(QemOut))) return s;            // the round's wait: alive and the number taken
        std::swap(d_faces, d_other);
        if (h->alive > alive) return fail(ctx, TC_GPU, "simplify_quadric: a round's face count grew");     // (never; the launches below are sized by it)
        alive = h->alive;
        if (h->taken == 0u) break;                              // nothing was selected
        ++rounds;
    }

    TC_HIP_TRY(ctx, hipMemsetAsync(d_used, 0, n * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "qem_write");
        if (alive > 0) hipLaunchKernelGGL(qem_mark_used_kernel, dim3(blocks_for(alive)), dim3(256), 0, st, (const uint32_t *)d_faces, (uint32_t)alive, d_used);
        if (tc_status s = exclusive_scan_u32(ctx, d_used, (uint32_t)n, d_vpos, blocksum)) return s;
        hipLaunchKernelGGL(qem_counts_kernel, dim3(1), dim3(1), 0, st, (const uint32_t *)(d_vpos + n), d_out);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = read_back(ctx, h, d_out, sizeof(QemOut))) return s;                // the last wait but the drain: the vertex count
    const size_t nv = h->n_out_vertices, nf = alive;
    *n_out_vertices = nv; *n_out_faces = nf;
    if (n_rounds) *n_rounds = rounds;
    if (!a.any_output()) return TC_OK;
    if (tc_status s = qem_check_caps(ctx, a, nv, nf)) return s;
    {
        ProfScope ps(ctx, "qem_write");
        if (a.out_xyz) hipLaunchKernelGGL(qem_write_vertices_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const float4 *)d_rec, (uint32_t)n, (const uint32_t *)d_used,
                                          (const uint32_t *)d_vpos, a.out_xyz);
        if (a.out_faces && nf) hipLaunchKernelGGL(qem_write_faces_kernel, dim3(blocks_for(nf)), dim3(256), 0, st, (const uint32_t *)d_faces, (uint32_t)nf,
                                                  (const uint32_t *)d_vpos, a.out_faces);
        if (a.out_map) hipLaunchKernelGGL(qem_write_map_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t *)d_parent, (uint32_t)n, (const uint32_t *)d_used,
                                          (const uint32_t *)d_vpos, a.out_map);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_qem.h) -----------------------------------------------------------------------------
// the header's checks (1) to (5), in its order
static tc_status qem_check(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces, const tc_qem_config *cfg,
                           size_t *n_out_vertices, size_t *n_out_faces) {
    if (!ctx) return TC_INVALID_DATA;
    if (!vertices) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: vertices is NULL");
    if (!faces) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: faces is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: config is NULL");
    if (!n_out_vertices || !n_out_faces) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: a count pointer is NULL");
    if (n_vertices == 0 || n_faces == 0) return fail(ctx, TC_INVALID_DATA, "Mesh is empty");                               // quadric_error.rs:414-416
    if (cfg->preserve_boundary > 1u) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: preserve_boundary is neither 0 nor 1");
    if (!(cfg->reduction_ratio >= 0.0f && cfg->reduction_ratio <= 1.0f)) return fail(ctx, TC_INVALID_DATA, "Reduction ratio must be between 0.0 and 1.0");   // :418-422
    if (!(cfg->max_edge_length >= 0.0f)) return fail(ctx, TC_INVALID_DATA, "simplify_quadric: max_edge_length is negative or NaN");
    if (n_vertices >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "simplify_quadric: n_vertices is 2^32 - 16 or more");
    if (n_faces >= (kMaxPoints + 2) / 3) return fail(ctx, TC_UNSUPPORTED, "simplify_quadric: 3 n_faces is 2^32 - 16 or more");
    return TC_OK;
}

extern "C" {

void tc_qem_config_default(float reduction_ratio, tc_qem_config *cfg) try {
    if (!cfg) return;
    cfg->reduction_ratio = reduction_ratio;
    cfg->preserve_boundary = 1u;
    cfg->max_edge_length = 0.0f;
} TC_CATCH_VOID

tc_status tc_simplify_quadric_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                     const tc_qem_config *cfg, float *out_vertices, size_t cap_vertices, uint32_t *out_faces,
                                     size_t cap_faces, uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces,
                                     uint32_t *n_rounds) try {
    if (tc_status s = qem_check(ctx, vertices, n_vertices, faces, n_faces, cfg, n_out_vertices, n_out_faces)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const QemCall call{vertices, n_vertices, faces, n_faces, out_vertices, cap_vertices, out_faces, cap_faces, out_vertex_map};
    return qem_on_device(ctx, call, *cfg, n_out_vertices, n_out_faces, n_rounds);
} TC_CATCH_STATUS(ctx)

tc_status tc_simplify_quadric(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                              const tc_qem_config *cfg, float *out_vertices, size_t cap_vertices, uint32_t *out_faces, size_t cap_faces,
                              uint32_t *out_vertex_map, size_t *n_out_vertices, size_t *n_out_faces, uint32_t *n_rounds) try {
    if (tc_status s = qem_check(ctx, vertices, n_vertices, faces, n_faces, cfg, n_out_vertices, n_out_faces)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = n_vertices, m = n_faces;
    ScopedBuf o_xyz, o_faces, o_map;
    if (tc_status s = stage_in(ctx, ctx->in_a, vertices, n * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, faces, m * 3 * sizeof(uint32_t))) return s;
    // the device-side outputs are as large as the counts can get, whatever the caller's capacities: the capacity check is the caller's
    if (out_vertices) if (tc_status s = ensure(ctx, o_xyz, n * 3 * sizeof(float))) return s;
    if (out_faces) if (tc_status s = ensure(ctx, o_faces, m * 3 * sizeof(uint32_t))) return s;
    if (out_vertex_map) if (tc_status s = ensure(ctx, o_map, n * sizeof(uint32_t))) return s;
    const QemCall call{(const float *)ctx->in_a.p, n, (const uint32_t *)ctx->in_b.p, m, (float *)o_xyz.p, cap_vertices, (uint32_t *)o_faces.p, cap_faces,
                       (uint32_t *)o_map.p};
    if (tc_status s = qem_on_device(ctx, call, *cfg, n_out_vertices, n_out_faces, n_rounds)) return s;     // (a capacity failure has set the counts)
    if (!call.any_output()) return TC_OK;
    const size_t nv = *n_out_vertices, nf = *n_out_faces;
    if (out_vertices && nv) TC_HIP_TRY(ctx, hipMemcpyAsync(out_vertices, o_xyz.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (out_faces && nf) TC_HIP_TRY(ctx, hipMemcpyAsync(out_faces, o_faces.p, nf * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (out_vertex_map) TC_HIP_TRY(ctx, hipMemcpyAsync(out_vertex_map, o_map.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return synced(ctx);                                         // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

}  // extern "C"
