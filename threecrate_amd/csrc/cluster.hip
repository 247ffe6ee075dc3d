// cluster.hip -- Euclidean cluster extraction (threecrate-algorithms/src/segmentation.rs:396-455): the connected components
// of the relation d2 <= tol^2 (d2_nc: f32, left to right, no FMA), filtered by size and ranked largest first.
//
// The reference seeds a BFS at every unvisited point in index order and keeps the components whose size is within
// [min, max], then sorts them by size with a stable sort: equal sizes stay in the order of their smallest original index.
// Here the edge list is never materialised:
//   index   the grid index of grid.hip (cell edge ~ tol / 2), points cell-sorted;
//   hook    one lane per sorted position p walks the cells within tol (scan_pruned, as radius_all_kernel does) and unites p
//           with every adjacent q > p in a lock-free union-find over sorted positions (ECL-CC style: the larger root is hooked
//           under the smaller one by an agent-scope CAS; parent[v] <= v always, so the forest has no cycles).  One pass,
//           whatever the graph's diameter;
//   compress  every point gets its final root (its own array); per-root size (integer add) and smallest original index (integer min),
//           aggregated per wave;
//   select  qualifying roots, keyed (n - size) << 32 | min_index and radix-sorted (sort_pairs, grid.hip): the reference's order;
//   emit    labels[orig] = rank or TC_CLUSTER_NONE; members: a stable radix sort (sort_pairs again) of (rank, original index) in index order.
// The partition and the ranks are unique, so the output does not depend on the order in which the atomics arrive.
#include "tc_internal.h"
#include "knn_list.h"

#include <cmath>

namespace tc {

// Parent words are re-read after other lanes' CASes on any XCD: every access is an agent-scope atomic (a plain load may be
// served by this XCD's L2 with a stale value, and a loop over stale values need not end).
__device__ __forceinline__ uint32_t uf_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, with intermediate pointer jumping: every visited word is pointed at its grandparent (an ancestor, so the
// store is valid whatever other lanes write there meanwhile; a root is never written by it)
__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
    uint32_t cur = uf_load(&parent[x]);
    if (cur != x) {
        uint32_t prev = x, next;
        while (cur > (next = uf_load(&parent[cur]))) {
            uf_store(&parent[prev], next);
            prev = cur;
            cur = next;
        }
    }
    return cur;
}

// unite the sets of a and b; returns the root of the merged set as it was seen (an ancestor of both from then on)
__device__ __forceinline__ uint32_t uf_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    uint32_t ra = uf_find(parent, a), rb = uf_find(parent, b);
    while (ra != rb) {
        const uint32_t lo = min(ra, rb), hi = max(ra, rb);
        uint32_t expected = hi;
        if (__hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            return lo;
        // hi was hooked by another lane meanwhile: start again from the roots as they are now
        ra = uf_find(parent, expected);
        rb = uf_find(parent, lo);
    }
    return ra;
}

__global__ void __launch_bounds__(256) clu_init_kernel(uint32_t n, uint32_t *__restrict__ parent, uint32_t *__restrict__ size,
                                                      uint32_t *__restrict__ minidx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    parent[p] = p;
    size[p] = 0u;
    minidx[p] = 0xFFFFFFFFu;
}

// one lane per cell-sorted point; the non-finite bucket behind the last cell has no edges
template <bool EXT>
__global__ void __launch_bounds__(128) clu_hook_kernel(GridView gv, float r2, int R, uint32_t *parent) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    const GridGeom &g = gv.g;
    if (p >= gv.cell_start[g.ncell]) return;
    const float4 q = gv.pts[p];
    if (!finite_query(q.x, q.y, q.z)) return;
    const QueryPlace pl = place_query<EXT>(g, q);
    uint32_t rp = p;        // a known ancestor of p: the next find starts there
    scan_pruned<EXT>(gv, q, pl.cx, pl.cy, pl.cz, -1, R, r2, [&](uint32_t j, const float4 &c) {
        if (j > p && d2_nc(c.x, c.y, c.z, q.x, q.y, q.z) <= r2) rp = uf_unite(parent, rp, j);     // nearest_neighbor.rs:271
    });
}

// every point's final root, into comp[] (not into parent[]: another lane's pointer jumping may still store an intermediate
// ancestor there after this lane's store), and per root the size and the smallest original index.  The lanes of a wave that
// share a root add / min once (neighbouring sorted points mostly do).
__global__ void __launch_bounds__(256) clu_compress_kernel(uint32_t n, const float4 *__restrict__ pts, uint32_t *parent,
                                                          uint32_t *__restrict__ comp, uint32_t *__restrict__ size,
                                                          uint32_t *__restrict__ minidx) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool pending = p < n;
    uint32_t r = 0, orig = 0xFFFFFFFFu;
    if (pending) {
        r = uf_find(parent, p);
        comp[p] = r;
        orig = __float_as_uint(pts[p].w);
    }
    const int lane = (int)(threadIdx.x & 63u);
    for (;;) {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) break;
        const int leader = __ffsll((long long)m) - 1;
        const uint32_t lr = __shfl(r, leader);
        const bool mine = pending && r == lr;
        const unsigned long long mm = __ballot(mine);
        uint32_t v = mine ? orig : 0xFFFFFFFFu;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = min(v, (uint32_t)__shfl_xor(v, off));
        if (lane == leader) {
            atomicAdd(&size[lr], (uint32_t)__popcll(mm));
            atomicMin(&minidx[lr], v);
        }
        if (mine) pending = false;
    }
}

__global__ void __launch_bounds__(256) clu_flag_kernel(uint32_t n, const uint32_t *__restrict__ parent, const uint32_t *__restrict__ size,
                                                      uint32_t smin, uint32_t smax, uint32_t *__restrict__ flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t s = size[p];
    flag[p] = (parent[p] == p && s >= smin && s <= smax) ? 1u : 0u;      // segmentation.rs:452
}

// key: size descending, then smallest original index ascending (the stable sort_by of segmentation.rs:458 over seeds in index order)
__global__ void __launch_bounds__(256) clu_key_kernel(uint32_t n, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                                                     const uint32_t *__restrict__ size, const uint32_t *__restrict__ minidx,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ roots) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || !flag[p]) return;
    const uint32_t o = pos[p];
    keys[o] = ((uint64_t)(n - size[p]) << 32) | (uint64_t)minidx[p];
    roots[o] = p;
}

__global__ void __launch_bounds__(256) clu_rank_kernel(uint32_t nc, const uint32_t *__restrict__ roots, const uint32_t *__restrict__ size,
                                                      uint32_t *__restrict__ rank_of, uint32_t *__restrict__ csize) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    const uint32_t r = roots[k];
    rank_of[r] = k;
    csize[k] = size[r];
}

__global__ void __launch_bounds__(256) clu_offsets_kernel(uint32_t nc, const uint32_t *__restrict__ off32, uint64_t *__restrict__ offsets) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= nc) offsets[k] = off32[k];
}

__global__ void __launch_bounds__(256) clu_label_kernel(uint32_t n, const float4 *__restrict__ pts, const uint32_t *__restrict__ comp,
                                                       const uint32_t *__restrict__ flag, const uint32_t *__restrict__ rank_of,
                                                       uint32_t *__restrict__ labels) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = comp[p];
    labels[__float_as_uint(pts[p].w)] = flag[r] ? rank_of[r] : TC_CLUSTER_NONE;
}

// members: sort key = rank (unclustered: nc, behind every cluster), value = original index, in index order
__global__ void __launch_bounds__(256) clu_member_key_kernel(uint32_t n, uint32_t nc, const uint32_t *__restrict__ labels,
                                                            uint32_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t l = labels[i];
    keys[i] = (l == TC_CLUSTER_NONE) ? nc : l;
    idx[i] = i;
}

tc_status cluster_extract_device(tc_context *ctx, const float *d_xyz, size_t n, float tol, size_t min_size, size_t max_size,
                                 uint32_t *d_labels, uint32_t *d_members, uint64_t *d_offsets, size_t *n_clusters) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    const unsigned nb = (unsigned)((n + 255) / 256);
    const float r2 = tol * tol;                         // nearest_neighbor.rs:259
    // sizes are at most n: clamp the bounds into 32 bits without changing which components pass
    const uint32_t smin = (uint32_t)std::min<size_t>(min_size, (size_t)n32 + 1), smax = (uint32_t)std::min<size_t>(max_size, n32);

    DeviceIndex &ix = ctx->tgt_index;
    // (the grid's cell budget may widen the edge; a NaN tolerance keeps the volume-based edge and has no edges at all)
    const bool edges = r2 <= r2;
    if (tc_status s = build_index(ctx, ix, d_xyz, n, ball_grid(tol, false))) return s;
    const GridView gv = view_of(ix);

    auto &B = ctx->clu;             // (what each slot holds: enum CluSlot, tc_internal.h)
    const size_t u32 = sizeof(uint32_t);
    const std::pair<CluSlot, size_t> need[] = {{CLU_PARENT, n * u32}, {CLU_SIZE, n * u32}, {CLU_MIN_INDEX, n * u32}, {CLU_FLAG, n * u32},
                                               {CLU_POS, (n + 1) * u32}, {CLU_KEYS, 2 * n * sizeof(uint64_t)}, {CLU_ROOTS, 2 * n * u32},
                                               {CLU_RANK_OF, n * u32}, {CLU_SIZES, (2 * n + 1) * u32}, {CLU_COMP, n * u32}};
    for (const auto &[slot, bytes] : need) if (tc_status s = ensure(ctx, B[slot], bytes)) return s;
    uint32_t *parent = (uint32_t *)B[CLU_PARENT].p, *size = (uint32_t *)B[CLU_SIZE].p, *minidx = (uint32_t *)B[CLU_MIN_INDEX].p,
             *flag = (uint32_t *)B[CLU_FLAG].p, *pos = (uint32_t *)B[CLU_POS].p, *roots = (uint32_t *)B[CLU_ROOTS].p, *roots_s = roots + n,
             *rank_of = (uint32_t *)B[CLU_RANK_OF].p, *csize = (uint32_t *)B[CLU_SIZES].p, *off32 = csize + n, *comp = (uint32_t *)B[CLU_COMP].p;
    uint64_t *keys = (uint64_t *)B[CLU_KEYS].p, *keys_s = keys + n;
    uint32_t *labels = d_labels;
    if (!labels) {
        if (tc_status s = ensure(ctx, B[CLU_LABELS], n * sizeof(uint32_t))) return s;
        labels = (uint32_t *)B[CLU_LABELS].p;
    }

    {
        ProfScope ps(ctx, "cluster_hook");
        hipLaunchKernelGGL(clu_init_kernel, dim3(nb), dim3(256), 0, st, n32, parent, size, minidx);
        if (edges) {
            const dim3 grid((n32 + 127) / 128), block(128);
            with_clamped(gv, [&](auto ext) { hipLaunchKernelGGL(clu_hook_kernel<decltype(ext)::value>, grid, block, 0, st, gv, r2, ball_rings(gv.g, tol), parent); });
        }
    }
    {
        ProfScope ps(ctx, "cluster_compress");
        hipLaunchKernelGGL(clu_compress_kernel, dim3(nb), dim3(256), 0, st, n32, gv.pts, parent, comp, size, minidx);
    }
    {
        ProfScope ps(ctx, "cluster_select");
        hipLaunchKernelGGL(clu_flag_kernel, dim3(nb), dim3(256), 0, st, n32, (const uint32_t *)parent, (const uint32_t *)size, smin, smax, flag);
        if (tc_status s = exclusive_scan_u32(ctx, flag, n32, pos, ix.blocksum)) return s;
    }
    if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, pos + n, sizeof(uint32_t))) return s;
    const uint32_t nc = pinned_host(ctx)->count;
    *n_clusters = nc;

    if (nc) {
        ProfScope ps(ctx, "cluster_rank");
        hipLaunchKernelGGL(clu_key_kernel, dim3(nb), dim3(256), 0, st, n32, (const uint32_t *)flag, (const uint32_t *)pos, (const uint32_t *)size,
                           (const uint32_t *)minidx, keys, roots);
        if (tc_status s = sort_pairs(ctx, keys, keys_s, roots, roots_s, nc, 32u + bits_for_value(n32), B[CLU_SORT_TEMP])) return s;
        hipLaunchKernelGGL(clu_rank_kernel, dim3((nc + 255) / 256), dim3(256), 0, st, nc, (const uint32_t *)roots_s, (const uint32_t *)size,
                           rank_of, csize);
    }
    {
        ProfScope ps(ctx, "cluster_label");
        hipLaunchKernelGGL(clu_label_kernel, dim3(nb), dim3(256), 0, st, n32, gv.pts, (const uint32_t *)comp, (const uint32_t *)flag,
                           (const uint32_t *)rank_of, labels);
    }
    if (d_offsets) {
        ProfScope ps(ctx, "cluster_offsets");
        if (nc) {
            if (tc_status s = exclusive_scan_u32(ctx, csize, nc, off32, ix.blocksum)) return s;
        } else {
            TC_HIP_TRY(ctx, hipMemsetAsync(off32, 0, sizeof(uint32_t), st));
        }
        hipLaunchKernelGGL(clu_offsets_kernel, dim3((nc + 1 + 255) / 256), dim3(256), 0, st, nc, (const uint32_t *)off32, d_offsets);
    }
    if (d_members && nc) {
        ProfScope ps(ctx, "cluster_members");
        uint32_t *mkeys = (uint32_t *)B[CLU_KEYS].p, *mkeys_s = mkeys + n, *midx = roots;
        hipLaunchKernelGGL(clu_member_key_kernel, dim3(nb), dim3(256), 0, st, n32, nc, (const uint32_t *)labels, mkeys, midx);
        if (tc_status s = sort_pairs(ctx, mkeys, mkeys_s, midx, d_members, n, bits_for_value(nc), B[CLU_SORT_TEMP])) return s;
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- extract_euclidean_clusters (segmentation.rs:396-455) -----------------------------------
// checks in the reference's order (:400-416); then the limits of this implementation
static tc_status cluster_validate(tc_context *ctx, size_t n, float tol, size_t min_size, size_t max_size, const uint32_t *members,
                                  const uint64_t *offsets, size_t *n_clusters) {
    if (!ctx || !n_clusters || (members && !offsets)) return TC_INVALID_DATA;
    *n_clusters = 0;
    if (n == 0) return fail(ctx, TC_INVALID_DATA, "Point cloud is empty");
    if (tol <= 0.0f) return fail(ctx, TC_INVALID_DATA, "Tolerance must be positive");
    if (min_size == 0) return fail(ctx, TC_INVALID_DATA, "min_cluster_size must be at least 1");
    if (min_size > max_size) return fail(ctx, TC_INVALID_DATA, "min_cluster_size must not exceed max_cluster_size");
    if (tc_status s = check_point_count(ctx, n)) return s;
    if (std::isinf(tol * tol)) return fail(ctx, TC_UNSUPPORTED, "extract_euclidean_clusters: tolerance * tolerance is not finite");
    return TC_OK;
}

extern "C" {
tc_status tc_extract_euclidean_clusters_device(tc_context *ctx, const float *d_xyz, size_t n, float tolerance, size_t min_cluster_size,
                                               size_t max_cluster_size, uint32_t *d_labels, uint32_t *d_members, uint64_t *d_offsets,
                                               size_t *n_clusters) try {
    if (tc_status s = cluster_validate(ctx, n, tolerance, min_cluster_size, max_cluster_size, d_members, d_offsets, n_clusters)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = cluster_extract_device(ctx, d_xyz, n, tolerance, min_cluster_size, max_cluster_size, d_labels, d_members, d_offsets,
                                             n_clusters)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_extract_euclidean_clusters(tc_context *ctx, const float *xyz, size_t n, float tolerance, size_t min_cluster_size,
                                        size_t max_cluster_size, uint32_t *labels, uint32_t *members, uint64_t *offsets,
                                        size_t *n_clusters) try {
    if (tc_status s = cluster_validate(ctx, n, tolerance, min_cluster_size, max_cluster_size, members, offsets, n_clusters)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t cap = n / min_cluster_size + 1;         // offsets: at most n / min_cluster_size clusters
    if (tc_status s = ensure(ctx, ctx->out_a, 2 * n * sizeof(uint32_t) + cap * sizeof(uint64_t))) return s;
    uint32_t *d_labels = labels ? (uint32_t *)ctx->out_a.p : nullptr, *d_members = members ? (uint32_t *)ctx->out_a.p + n : nullptr;
    uint64_t *d_offsets = offsets ? (uint64_t *)((uint32_t *)ctx->out_a.p + 2 * n) : nullptr;
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = cluster_extract_device(ctx, (const float *)ctx->in_a.p, n, tolerance, min_cluster_size, max_cluster_size, d_labels,
                                             d_members, d_offsets, n_clusters)) return s;
    if (labels) TC_HIP_TRY(ctx, hipMemcpyAsync(labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (offsets) TC_HIP_TRY(ctx, hipMemcpyAsync(offsets, d_offsets, (*n_clusters + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    TC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (members && offsets[*n_clusters]) {       // (the member count is known once the offsets are back)
        TC_HIP_TRY(ctx, hipMemcpyAsync(members, d_members, offsets[*n_clusters] * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        TC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return TC_OK;
} TC_CATCH_STATUS(ctx)
}  // extern "C"
