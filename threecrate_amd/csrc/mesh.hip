// mesh.hip -- smooth a triangle mesh (smooth_laplacian, smooth_taubin, smooth_hc, threecrate-algorithms/src/mesh_smoothing.rs) and the
// one-ring vertex adjacency it sweeps over; the entry points of include/threecrate_hip_mesh.h, which pins the arithmetic.
// This unit is the whole of the companion library libthreecrate_hip_mesh.so; the host layer of tc_internal.h (ensure, stage_in,
// read_back, group_by_key, ProfScope) resolves from libthreecrate_hip.so.
//   The adjacency build, one profile row (mesh_adjacency):
//   mesh_key        a thread per face: its six directed pairs as packed keys from << b | to (b = bits_for_value(n - 1)) and `to` as the
//                   value; an index >= n raises the flag (one atomic per wave that has such a lane) and its face writes vertex 0
//   group_by_key (grid.hip)   one run per distinct pair, ascending in `from`, then in `to`
//   mesh_compact    the head of every run stores its `to` at the run's number: the CSR's neighbours
//   mesh_offsets    a thread per vertex: the first sorted position whose `from` is not below it (a binary search; that position is
//                   a run head or the end) has as its run number the vertex's offset.  Unreferenced vertices fall out of the same search
//   mesh_long_list  the vertices whose ring exceeds kMeshLongRing, listed for the wave-per-vertex kernel; the entry count
//   -- one read-back: the flag, the long-ring count, the entry count --
//   The sweeps: positions live as 16-byte records (x, y, z, 0) in scratch; a gather is one 16-byte load.  mesh_pack / mesh_unpack are the
//   only kernels that see the caller's 12-byte layout.
//   mesh_sweep<KIND>       a lane per vertex whose ring is at most kMeshLongRing: the fold is sequential by contract, eight gathers in
//                          flight at a time (fold_run_lane, run_fold.h).  STEP: a Laplacian step; HC_B: qbar and b; HC_Q: q
//   mesh_sweep_long<KIND>  a wave per listed vertex: 64 neighbour records loaded at once, the adds sequential on broadcast values
//                          (fold_run_wave, run_fold.h): the same bits
//   No atomics and no host wait between the launches of a call.
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_mesh.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// A ring of more neighbours than this is folded by a wave (mesh_sweep_long).  TC_MESH_LONG_RING: the A/B builds of `make mesh-ab`
// (variants/, what tools/mesh_bench.py --ring loads); never the product.  Measured with them (STATE.md, one whole sweep over 2 000 fans of
// one ring size): ring 96 on one lane 15.9 us against 17.6 with a wave each, ring 192 28.0 against 24.9, ring 1 024 151 against 86: the
// roads cross between 96 and 192, and of the thresholds 16 / 32 / 64 / 128 / 256 this one has the better road at every size.  A single hub of
// 100 000 gains nothing from its wave (4.87 ms against 4.74 ms on one lane): the chain is what costs there.
#ifdef TC_MESH_LONG_RING
constexpr uint32_t kMeshLongRing = TC_MESH_LONG_RING;
#else
constexpr uint32_t kMeshLongRing = 128;
#endif
constexpr int kMeshLongBlocks = 1024;           // the wave-per-vertex kernel's grid is capped; its waves stride over the list

enum MeshKind { MESH_STEP, MESH_HC_B, MESH_HC_Q };

// what one sweep reads and writes; records of 16 bytes
struct MeshSweep {
    const float4 *gather;       // the array whose neighbour records are folded: STEP the positions, HC_B q, HC_Q b
    const float4 *self;         // HC_Q: qbar (STEP and HC_B read the vertex's own record from `gather`)
    const float4 *p;            // HC_B: the input positions
    float4 *out;                // STEP: the new positions; HC_B: qbar; HC_Q: q
    float4 *out2;               // HC_B: b
    float f0, f1;               // STEP: t; HC_B: alpha, 1 - alpha; HC_Q: beta, 1 - beta
};

__global__ void __launch_bounds__(256) mesh_key_kernel(const uint32_t *__restrict__ faces, uint32_t m, uint32_t n, uint32_t b,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ tos, uint32_t *__restrict__ flag) {
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (f < m) {
        uint32_t v[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
        bad = v[0] >= n || v[1] >= n || v[2] >= n;
        if (bad) v[0] = v[1] = v[2] = 0u;                       // the call fails; the keys stay inside their bits
        const int from[6] = {0, 0, 1, 1, 2, 2}, to[6] = {1, 2, 0, 2, 0, 1};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            keys[6 * (size_t)f + k] = ((uint64_t)v[from[k]] << b) | (uint64_t)v[to[k]];
            tos[6 * (size_t)f + k] = v[to[k]];
        }
    }
    if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(256) mesh_compact_kernel(const uint32_t *__restrict__ tos_sorted, const uint32_t *__restrict__ head,
                                                          const uint32_t *__restrict__ runpos, uint32_t n_keys, uint32_t *__restrict__ neighbors) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_keys || !head[p]) return;
    neighbors[runpos[p]] = tos_sorted[p];                       // runpos[p] < R <= n_keys
}

// offsets[v] for v in [0, n]: the distinct pairs whose `from` is below v
__global__ void __launch_bounds__(256) mesh_offsets_kernel(const uint64_t *__restrict__ keys_sorted, uint32_t n_keys, const uint32_t *__restrict__ runpos,
                                                          uint32_t n, uint32_t b, uint32_t *__restrict__ offsets) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > n) return;
    uint32_t lo = 0u, hi = n_keys;                              // first position in [0, n_keys] whose from >= v
    if (v == n) lo = n_keys;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint32_t)(keys_sorted[mid] >> b) < v) lo = mid + 1u; else hi = mid;
    }
    offsets[v] = runpos[lo];                                    // runpos has n_keys + 1 words
}

__global__ void __launch_bounds__(256) mesh_long_list_kernel(const uint32_t *__restrict__ offsets, uint32_t n, uint32_t *__restrict__ long_list,
                                                            uint32_t list_cap, uint32_t *__restrict__ counters) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    if (v == 0u) counters[2] = offsets[n];
    if (offsets[v + 1] - offsets[v] > kMeshLongRing) append_long_run(long_list, list_cap, &counters[1], v);
}

__global__ void __launch_bounds__(256) mesh_pack_kernel(const float *__restrict__ xyz, uint32_t n, float4 *__restrict__ rec) {
    pack_xyz_records<false>(xyz, n, rec, nullptr, 0u);
}

// (no __restrict__: the caller's output may be anything but the records)
__global__ void __launch_bounds__(256) mesh_unpack_kernel(const float4 *rec, uint32_t n, float *xyz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 r = rec[i];
    xyz[3 * (size_t)i] = r.x; xyz[3 * (size_t)i + 1] = r.y; xyz[3 * (size_t)i + 2] = r.z;
}

// vertex i, its degree and the finished fold of its ring: the header's (3) and (6), one operation per line
template <int KIND>
__device__ __forceinline__ void mesh_finish(const MeshSweep &a, uint32_t i, uint32_t deg, float sx, float sy, float sz) {
    const float fd = (float)deg;
    if constexpr (KIND == MESH_STEP) {
        const float4 v = a.gather[i];
        float4 o = v;
        if (deg) {
            const float cx = sx / fd, cy = sy / fd, cz = sz / fd;
            const float dx = cx - v.x, dy = cy - v.y, dz = cz - v.z;
            const float mx = dx * a.f0, my = dy * a.f0, mz = dz * a.f0;
            o.x = v.x + mx; o.y = v.y + my; o.z = v.z + mz;
        }
        a.out[i] = o;
    } else if constexpr (KIND == MESH_HC_B) {
        const float4 q = a.gather[i], p = a.p[i];
        float4 qb = q;
        if (deg) { qb.x = sx / fd; qb.y = sy / fd; qb.z = sz / fd; }
        const float pax = p.x * a.f0, pay = p.y * a.f0, paz = p.z * a.f0;
        const float qwx = q.x * a.f1, qwy = q.y * a.f1, qwz = q.z * a.f1;
        const float blx = pax + qwx, bly = pay + qwy, blz = paz + qwz;
        a.out[i] = qb;
        a.out2[i] = make_float4(qb.x - blx, qb.y - bly, qb.z - blz, 0.0f);
    } else {
        const float4 qb = a.self[i], b = a.gather[i];
        float ax = 0.0f, ay = 0.0f, az = 0.0f;
        if (deg) { ax = sx / fd; ay = sy / fd; az = sz / fd; }
        const float bbx = b.x * a.f0, bby = b.y * a.f0, bbz = b.z * a.f0;
        const float aux = ax * a.f1, auy = ay * a.f1, auz = az * a.f1;
        const float cx = bbx + aux, cy = bby + auy, cz = bbz + auz;
        a.out[i] = make_float4(qb.x - cx, qb.y - cy, qb.z - cz, 0.0f);
    }
}

template <int KIND>
__global__ void __launch_bounds__(256) mesh_sweep_kernel(MeshSweep a, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ neighbors, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = offsets[i], e = offsets[i + 1];
    if (e - s > kMeshLongRing) return;                          // (a long ring is folded by its wave)
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    fold_run_lane<8>(s, e, [&](uint32_t j) { return a.gather[neighbors[j]]; }, [&](const float4 &r) { sx = sx + r.x; sy = sy + r.y; sz = sz + r.z; });
    mesh_finish<KIND>(a, i, e - s, sx, sy, sz);
}

template <int KIND>
__global__ void __launch_bounds__(256) mesh_sweep_long_kernel(MeshSweep a, const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ neighbors,
                                                             const uint32_t *__restrict__ long_list, uint32_t n_long) {
    const uint32_t lane = threadIdx.x & 63u;
    for_each_listed_run(long_list, n_long, [&](uint32_t i) {
        const uint32_t s = offsets[i], e = offsets[i + 1];
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;                  // every lane runs the same chain
        fold_run_wave(s, e, lane, [&](uint32_t j) { return a.gather[neighbors[j]]; }, [&](const float4 &r) { sx = sx + r.x; sy = sy + r.y; sz = sz + r.z; });
        if (lane == 0u) mesh_finish<KIND>(a, i, e - s, sx, sy, sz);
    });
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the CSR of a call and what the build needed on the way; released when the call returns
struct MeshAdjacency {
    ScopedBuf keys, keys_sorted, tos, tos_sorted, head, runpos, rstart, sort_temp, blocksum;
    ScopedBuf offsets, neighbors, long_list, counters;
    size_t n_entries = 0, n_long = 0;
};

// validated sizes; d_faces is a device pointer.  One read-back; an index out of range is the header's check (6)
static tc_status mesh_build(tc_context *ctx, const char *who, size_t n, const uint32_t *d_faces, size_t m, MeshAdjacency &A) {
    hipStream_t st = ctx->stream;
    const size_t nk = 6 * m;                                    // < 2^32 - 16
    const size_t list_cap = nk / ((size_t)kMeshLongRing + 1) + 1;
    const std::pair<ScopedBuf *, size_t> need[] = {{&A.keys, nk * sizeof(uint64_t)}, {&A.tos, nk * sizeof(uint32_t)}, {&A.offsets, (n + 1) * sizeof(uint32_t)},
                                                   {&A.neighbors, nk * sizeof(uint32_t)}, {&A.long_list, list_cap * sizeof(uint32_t)},
                                                   {&A.counters, sizeof(MeshOut)}};
    for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    const unsigned b = bits_for_value(n - 1);                   // <= 32: a key has 2 b <= 64 bits
    uint64_t *keys = (uint64_t *)A.keys.p;
    uint32_t *tos = (uint32_t *)A.tos.p, *offsets = (uint32_t *)A.offsets.p, *neighbors = (uint32_t *)A.neighbors.p, *long_list = (uint32_t *)A.long_list.p,
             *ctr = (uint32_t *)A.counters.p;
    TC_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, sizeof(MeshOut), st));
    {
        ProfScope ps(ctx, "mesh_adjacency");
        hipLaunchKernelGGL(mesh_key_kernel, dim3(blocks_for(m)), dim3(256), 0, st, d_faces, (uint32_t)m, (uint32_t)n, (uint32_t)b, keys, tos, ctr);
        KeyGroups g;
        if (tc_status s = group_by_key(ctx, keys, tos, nk, 2u * b,
                                       GroupBufs{A.keys_sorted, A.tos_sorted, A.head, A.runpos, A.rstart, A.sort_temp, A.blocksum}, g)) return s;
        hipLaunchKernelGGL(mesh_compact_kernel, dim3(blocks_for(nk)), dim3(256), 0, st, g.order, (const uint32_t *)g.head, (const uint32_t *)g.runpos, (uint32_t)nk,
                           neighbors);
        hipLaunchKernelGGL(mesh_offsets_kernel, dim3(blocks_for(n + 1)), dim3(256), 0, st, g.keys_sorted, (uint32_t)nk, (const uint32_t *)g.runpos, (uint32_t)n,
                           (uint32_t)b, offsets);
        hipLaunchKernelGGL(mesh_long_list_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t *)offsets, (uint32_t)n, long_list,
                           (uint32_t)list_cap, ctr);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    MeshOut *h = &pinned_host(ctx)->mesh_out;
    if (tc_status s = read_back(ctx, h, ctr, sizeof(MeshOut))) return s;
    if (h->bad_index) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": a face index is >= n_vertices");
    A.n_entries = h->n_entries;
    A.n_long = std::min<size_t>(h->n_long, list_cap);
    return TC_OK;
}

template <int KIND>
static void mesh_launch_sweep(tc_context *ctx, const char *row, const MeshSweep &a, const MeshAdjacency &A, size_t n) {
    hipStream_t st = ctx->stream;
    const uint32_t *offsets = (const uint32_t *)A.offsets.p, *neighbors = (const uint32_t *)A.neighbors.p;
    {
        ProfScope ps(ctx, row);
        hipLaunchKernelGGL(mesh_sweep_kernel<KIND>, dim3(blocks_for(n)), dim3(256), 0, st, a, offsets, neighbors, (uint32_t)n);
    }
    if (A.n_long) {
        ProfScope ps(ctx, "mesh_sweep_long");
        const unsigned blocks = (unsigned)std::min<size_t>((A.n_long + 3) / 4, kMeshLongBlocks);
        hipLaunchKernelGGL(mesh_sweep_long_kernel<KIND>, dim3(blocks), dim3(256), 0, st, a, offsets, neighbors, (const uint32_t *)A.long_list.p,
                           (uint32_t)A.n_long);
    }
}

// a validated call; device pointers.  d_out may be d_xyz: the input is packed into records before anything is written
static tc_status mesh_smooth_on_device(tc_context *ctx, const float *d_xyz, size_t n, const uint32_t *d_faces, size_t m, const tc_mesh_smooth_config &cfg,
                                       float *d_out) {
    hipStream_t st = ctx->stream;
    MeshAdjacency A;
    if (tc_status s = mesh_build(ctx, "mesh_smooth", n, d_faces, m, A)) return s;
    if (cfg.iterations == 0) {
        if (d_out != d_xyz) TC_HIP_TRY(ctx, hipMemcpyAsync(d_out, d_xyz, n * 3 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return synced(ctx);
    }
    const bool hc = cfg.method == TC_MESH_HC;
    ScopedBuf rec[4];                                           // Laplacian, Taubin: ping | pong; HC: p | q | qbar | b
    for (int k = 0; k < (hc ? 4 : 2); ++k) if (tc_status s = ensure(ctx, rec[k], n * sizeof(float4))) return s;
    float4 *r0 = (float4 *)rec[0].p, *r1 = (float4 *)rec[1].p, *r2 = (float4 *)rec[2].p, *r3 = (float4 *)rec[3].p;
    hipLaunchKernelGGL(mesh_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_xyz, (uint32_t)n, r0);
    const float4 *result;
    if (hc) {
        TC_HIP_TRY(ctx, hipMemcpyAsync(r1, r0, n * sizeof(float4), hipMemcpyDeviceToDevice, st));      // q = p
        const float w = 1.0f - cfg.alpha, u = 1.0f - cfg.beta;
        for (uint32_t it = 0; it < cfg.iterations; ++it) {
            mesh_launch_sweep<MESH_HC_B>(ctx, "mesh_sweep_hc_b", MeshSweep{r1, nullptr, r0, r2, r3, cfg.alpha, w}, A, n);
            mesh_launch_sweep<MESH_HC_Q>(ctx, "mesh_sweep_hc_q", MeshSweep{r3, r2, nullptr, r1, nullptr, cfg.beta, u}, A, n);
        }
        result = r1;
    } else {
        float4 *src = r0, *dst = r1;                            // the result's buffer follows the parity of the launch count
        const int steps = cfg.method == TC_MESH_TAUBIN ? 2 : 1;
        for (uint32_t it = 0; it < cfg.iterations; ++it)
            for (int k = 0; k < steps; ++k) {
                mesh_launch_sweep<MESH_STEP>(ctx, "mesh_sweep_step", MeshSweep{src, nullptr, nullptr, dst, nullptr, k ? cfg.mu : cfg.lambda, 0.0f}, A, n);
                std::swap(src, dst);
            }
        result = src;
    }
    hipLaunchKernelGGL(mesh_unpack_kernel, dim3(blocks_for(n)), dim3(256), 0, st, result, (uint32_t)n, d_out);
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
}

// offsets / neighbors: the caller's arrays, each optional; device arrays, or -- on_host -- host arrays
static tc_status mesh_adjacency(tc_context *ctx, size_t n, const uint32_t *d_faces, size_t m, uint32_t *offsets, uint32_t *neighbors, size_t capacity,
                                size_t *n_entries, bool on_host) {
    hipStream_t st = ctx->stream;
    MeshAdjacency A;
    if (tc_status s = mesh_build(ctx, "mesh_vertex_adjacency", n, d_faces, m, A)) return s;
    *n_entries = A.n_entries;
    if (!offsets && !neighbors) return TC_OK;
    if (capacity < A.n_entries) return fail(ctx, TC_INVALID_DATA, "mesh_vertex_adjacency: capacity is smaller than the number of entries");
    const hipMemcpyKind kind = on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (offsets) TC_HIP_TRY(ctx, hipMemcpyAsync(offsets, A.offsets.p, (n + 1) * sizeof(uint32_t), kind, st));
    if (neighbors && A.n_entries) TC_HIP_TRY(ctx, hipMemcpyAsync(neighbors, A.neighbors.p, A.n_entries * sizeof(uint32_t), kind, st));
    return synced(ctx);
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_mesh.h) ---------------------------------------------------------------------------
// the header's check (2)
static tc_status mesh_check_empty(tc_context *ctx, size_t n_vertices, size_t n_faces) {
    return (n_vertices == 0 || n_faces == 0) ? fail(ctx, TC_INVALID_DATA, "Mesh is empty") : TC_OK;             // mesh_smoothing.rs:99-101
}

// the header's check (5)
static tc_status mesh_check_limits(tc_context *ctx, const char *who, size_t n_vertices, size_t n_faces) {
    if (n_vertices >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, std::string(who) + ": n_vertices is 2^32 - 16 or more");
    if (n_faces >= (kMaxPoints + 5) / 6) return fail(ctx, TC_UNSUPPORTED, std::string(who) + ": 6 n_faces is 2^32 - 16 or more");
    return TC_OK;
}

static bool mesh_in(float x, float lo, float hi, bool lo_open, bool hi_open) {             // false for a NaN
    return (lo_open ? x > lo : x >= lo) && (hi_open ? x < hi : x <= hi);
}

// the header's checks (1) to (5), in its order
static tc_status mesh_check(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                            const tc_mesh_smooth_config *cfg, float *out_vertices) {
    if (!ctx) return TC_INVALID_DATA;
    if (!vertices) return fail(ctx, TC_INVALID_DATA, "mesh_smooth: vertices is NULL");
    if (!faces) return fail(ctx, TC_INVALID_DATA, "mesh_smooth: faces is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "mesh_smooth: config is NULL");
    if (!out_vertices) return fail(ctx, TC_INVALID_DATA, "mesh_smooth: out_vertices is NULL");
    if (tc_status s = mesh_check_empty(ctx, n_vertices, n_faces)) return s;
    if (cfg->method > TC_MESH_HC) return fail(ctx, TC_INVALID_DATA, "mesh_smooth: method is none of Laplacian (0), Taubin (1), HC (2)");
    if (cfg->method == TC_MESH_LAPLACIAN) {
        if (!mesh_in(cfg->lambda, 0.0f, 1.0f, true, false)) return fail(ctx, TC_INVALID_DATA, "lambda must be in (0, 1]");        // :102-104
    } else if (cfg->method == TC_MESH_TAUBIN) {
        if (!mesh_in(cfg->lambda, 0.0f, 1.0f, true, true)) return fail(ctx, TC_INVALID_DATA, "lambda must be in (0, 1)");         // :162-167
        if (!(cfg->mu < 0.0f) || !std::isfinite(cfg->mu)) return fail(ctx, TC_INVALID_DATA, "mu must be negative");
    } else {
        if (!mesh_in(cfg->alpha, 0.0f, 1.0f, false, false)) return fail(ctx, TC_INVALID_DATA, "alpha must be in [0, 1]");         // :229-234
        if (!mesh_in(cfg->beta, 0.0f, 1.0f, false, false)) return fail(ctx, TC_INVALID_DATA, "beta must be in [0, 1]");
    }
    return mesh_check_limits(ctx, "mesh_smooth", n_vertices, n_faces);
}

static tc_status mesh_check_adjacency(tc_context *ctx, size_t n_vertices, const uint32_t *faces, size_t n_faces, size_t *n_entries) {
    if (!ctx) return TC_INVALID_DATA;
    if (!faces) return fail(ctx, TC_INVALID_DATA, "mesh_vertex_adjacency: faces is NULL");
    if (!n_entries) return fail(ctx, TC_INVALID_DATA, "mesh_vertex_adjacency: n_entries is NULL");
    if (tc_status s = mesh_check_empty(ctx, n_vertices, n_faces)) return s;
    return mesh_check_limits(ctx, "mesh_vertex_adjacency", n_vertices, n_faces);
}

extern "C" {

void tc_mesh_smooth_config_default(uint32_t method, tc_mesh_smooth_config *cfg) try {
    if (!cfg) return;
    cfg->method = method;
    cfg->iterations = 10;
    cfg->lambda = 0.5f;
    cfg->mu = -0.53f;
    cfg->alpha = 0.0f;
    cfg->beta = 0.5f;
} TC_CATCH_VOID

tc_status tc_mesh_smooth_device(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                                const tc_mesh_smooth_config *cfg, float *out_vertices) try {
    if (tc_status s = mesh_check(ctx, vertices, n_vertices, faces, n_faces, cfg, out_vertices)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return mesh_smooth_on_device(ctx, vertices, n_vertices, faces, n_faces, *cfg, out_vertices);
} TC_CATCH_STATUS(ctx)

tc_status tc_mesh_smooth(tc_context *ctx, const float *vertices, size_t n_vertices, const uint32_t *faces, size_t n_faces,
                         const tc_mesh_smooth_config *cfg, float *out_vertices) try {
    if (tc_status s = mesh_check(ctx, vertices, n_vertices, faces, n_faces, cfg, out_vertices)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t b_xyz = n_vertices * 3 * sizeof(float);
    if (tc_status s = stage_in(ctx, ctx->in_a, vertices, b_xyz)) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, faces, n_faces * 3 * sizeof(uint32_t))) return s;
    if (tc_status s = ensure(ctx, ctx->out_a, b_xyz)) return s;
    if (tc_status s = mesh_smooth_on_device(ctx, (const float *)ctx->in_a.p, n_vertices, (const uint32_t *)ctx->in_b.p, n_faces, *cfg, (float *)ctx->out_a.p))
        return s;
    return stage_out(ctx, out_vertices, ctx->out_a.p, b_xyz);   // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

tc_status tc_mesh_vertex_adjacency_device(tc_context *ctx, size_t n_vertices, const uint32_t *faces, size_t n_faces, uint32_t *offsets,
                                          uint32_t *neighbors, size_t capacity, size_t *n_entries) try {
    if (tc_status s = mesh_check_adjacency(ctx, n_vertices, faces, n_faces, n_entries)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return mesh_adjacency(ctx, n_vertices, faces, n_faces, offsets, neighbors, capacity, n_entries, false);
} TC_CATCH_STATUS(ctx)

tc_status tc_mesh_vertex_adjacency(tc_context *ctx, size_t n_vertices, const uint32_t *faces, size_t n_faces, uint32_t *offsets,
                                   uint32_t *neighbors, size_t capacity, size_t *n_entries) try {
    if (tc_status s = mesh_check_adjacency(ctx, n_vertices, faces, n_faces, n_entries)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_b, faces, n_faces * 3 * sizeof(uint32_t))) return s;
    return mesh_adjacency(ctx, n_vertices, (const uint32_t *)ctx->in_b.p, n_faces, offsets, neighbors, capacity, n_entries, true);
} TC_CATCH_STATUS(ctx)

}  // extern "C"
