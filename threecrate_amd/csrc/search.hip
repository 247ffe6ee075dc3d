// search.hip -- the neighbour-search exports: NearestNeighborSearch::find_k_nearest / find_radius_neighbors over a device index
// (nearest_neighbor.rs:177-298), kernels, launchers and entry points (tc_knn, tc_radius_search, tc_search_index_*).  Other callers of
// the launchers: GICP's covariances (registration.hip), FPFH's fallback lists (fpfh.hip).
//   knn_kernel         a lane per query, k <= 129: sorted register list, ring continuation, collect and rank (as normals_point)
//   knn_coop_kernel    a block per query, k <= 2048: coop_nearest (knn_coop.h)
//   radius_all_kernel  every record within a radius: count, then fill at the caller's offsets
#include "tc_internal.h"
#include "knn_list.h"
#include "knn_coop.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tc {

// A limit handed to the cell walk is widened by this factor.  The walk compares it with squared gaps to cell boxes, the visitor compares
// the distances themselves (exactly, against the limit as it was).  Gap and distance round relative to the QUERY's distance from the cloud:
// 10^6 box diagonals away an ulp of either is more than a cell, the walk's absolute slack (2e-3 h) is gone, and a row whose gap rounded
// up past a member's distance was skipped (4 of 9 neighbours came back).  Both are sums of three squared differences: within 2^-21 of
// each other when they should be equal.
constexpr float kWalkSlack = 1.000004f;

// NearestNeighborSearch::find_k_nearest beyond the register list's 129 entries (k up to 2048): a block per query, the same
// selection; output like knn_kernel: (original index, sqrt(d2)) ascending, count = the entries within radius_sq
template <int CAPB>
__global__ void __launch_bounds__(kCoopThreads) knn_coop_kernel(GridView gv, const float *__restrict__ queries, uint32_t nq, uint32_t k,
                                                                uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                                uint32_t *__restrict__ out_count, float radius_sq) {
    __shared__ CoopShared<CAPB> sh;
    __shared__ uint32_t within_s;
    const GridGeom &g = gv.g;
    const int tid = threadIdx.x;
    const uint32_t nfin = gv.cell_start[g.ncell];
    for (uint32_t t = blockIdx.x; t < nq; t += gridDim.x) {
        const float qx = queries[3 * (size_t)t], qy = queries[3 * (size_t)t + 1], qz = queries[3 * (size_t)t + 2];
        const uint32_t K1 = min(k, nfin);
        // a NaN / infinite query has no finite distance to anything: no neighbours (see knn_kernel)
        if (!finite_query(qx, qy, qz) || K1 == 0) {
            if (tid == 0) out_count[t] = 0;
            continue;
        }
        if (tid == 0) within_s = 0;
        const uint32_t total = coop_nearest<CAPB>(gv, qx, qy, qz, K1, nfin, sh);
        const uint32_t cnt = min(K1, total);
        uint32_t within = 0;
        for (uint32_t r = (uint32_t)tid; r < cnt; r += kCoopThreads) {
            const unsigned long long key = sh.buf[r];
            const float v = __uint_as_float((uint32_t)(key >> 32));
            out_idx[(size_t)t * k + r] = __float_as_uint(gv.pts[(uint32_t)key].w);
            out_dist[(size_t)t * k + r] = sqrtf(v);                                   // nearest_neighbor.rs:249
            within += (v <= radius_sq) ? 1u : 0u;
        }
        if (within) atomicAdd(&within_s, within);
        __syncthreads();
        if (tid == 0) out_count[t] = within_s;
        __syncthreads();
    }
}

// ---- batch k-NN export -----------------------------------------------------
// NearestNeighborSearch::find_k_nearest (nearest_neighbor.rs:177-251, trait core/traits.rs:6-12;
// gpu_find_k_nearest_batch threecrate-gpu/src/nearest_neighbor.rs:345-355): for every query the k
// nearest cloud points, ascending, as (original index, sqrt(d2)).  Same machinery as normals_point
// (normals.hip): sorted register list for the k-th distance, ball-pruned ring continuation (queries may lie
// outside the grid: |p - q|^2 >= |p - clamp(q)|^2 + |q - clamp(q)|^2), LDS position lists, ranking.
template <int L, int BLOCK, bool EXT>
__global__ void __launch_bounds__(BLOCK) knn_kernel(GridView gv, const float *__restrict__ queries, uint32_t nq, uint32_t k,
                                                    uint32_t *__restrict__ out_idx, float *__restrict__ out_dist,
                                                    uint32_t *__restrict__ out_count, float radius_sq) {
    __shared__ uint32_t ldsA_[L * BLOCK];
    __shared__ uint8_t ldsB_[L * BLOCK];
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= nq) return;
    uint32_t *ldsA = ldsA_ + threadIdx.x;
    uint8_t *ldsB = ldsB_ + threadIdx.x;
    const GridGeom &g = gv.g;
    float4 q;
    q.x = queries[3 * (size_t)t]; q.y = queries[3 * (size_t)t + 1]; q.z = queries[3 * (size_t)t + 2]; q.w = 0.0f;
    // a NaN / infinite query has no finite distance to anything: no neighbours (the reference's kd-tree returns whatever nodes
    // its NaN comparisons visit first, with NaN distances)
    if (!finite_query(q.x, q.y, q.z)) { out_count[t] = 0; return; }
    const QueryPlace pl = place_query<EXT>(g, q);
    const int cx = pl.cx, cy = pl.cy, cz = pl.cz;
    const float mf = pl.mf, out2 = pl.out2;
    const uint32_t K1 = min(k, gv.cell_start[g.ncell]);      // the finite points
    if (K1 == 0) { out_count[t] = 0; return; }
    float d[L];
#pragma unroll
    for (int i = 0; i < L; ++i) d[i] = INFINITY;
    auto visit1 = [&](uint32_t, const float4 &c) { list_insert<L>(d, d2_nc(c.x, c.y, c.z, q.x, q.y, q.z)); };
    int R = 1;
    float tau = INFINITY;
    scan_block(gv, cx, cy, cz, R, visit1);
    for (;;) {
        tau = d[0];
#pragma unroll
        for (int i = 1; i < L; ++i) tau = ((uint32_t)i == K1 - 1) ? d[i] : tau;
        const bool covers = (cx - R <= 0) && (cx + R >= g.gx - 1) && (cy - R <= 0) && (cy + R >= g.gy - 1) &&
                            (cz - R <= 0) && (cz + R >= g.gz - 1);
        const float bound = ((float)R + mf - 2e-3f) * g.h;
        if (covers || tau <= bound * bound + out2) break;
        const int Rin = R;                                       // see normals_point
        if (tau == INFINITY) R += max(1, R / 2);
        else R = max(R + 1, (int)fminf(ceilf(sqrtf(fmaxf(tau - out2, 0.0f)) * g.inv_h - mf + 0.01f), 1.0e9f));
        const bool growing = tau == INFINITY || R > Rin + 1;
        float live_lim = tau * kWalkSlack;
        const bool touched = scan_pruned<EXT, true>(gv, q, cx, cy, cz, Rin, R, live_lim, [&](uint32_t j, const float4 &c) {
            visit1(j, c);
            if (growing) live_lim = d[L - 1] * kWalkSlack;       // bounds the k-th entry (static index: see normals_point)
        }, &live_lim);
        if (!touched) {
            tau = d[0];
#pragma unroll
            for (int i = 1; i < L; ++i) tau = ((uint32_t)i == K1 - 1) ? d[i] : tau;
            break;
        }
    }
    uint32_t n_lt = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) n_lt += (d[i] < tau) ? 1u : 0u;
    const uint32_t quota = K1 - min(n_lt, K1);
    uint32_t cnt = 0, ties = 0;
    scan_pruned<EXT>(gv, q, cx, cy, cz, -1, R, tau * kWalkSlack, [&](uint32_t j, const float4 &c) {
        const float v = d2_nc(c.x, c.y, c.z, q.x, q.y, q.z);
        bool take = v < tau;
        if (!take && v == tau && ties < quota) { take = true; ++ties; }
        if (take && cnt < K1) { ldsA[cnt * BLOCK] = j; ++cnt; }
    });
    unsigned long long taken_lo = 0ull, taken_hi = 0ull, taken_x = 0ull;
    auto is_taken = [&](uint32_t r) { return r < 64 ? ((taken_lo >> r) & 1ull) : r < 128 ? ((taken_hi >> (r - 64)) & 1ull) : ((taken_x >> (r - 128)) & 1ull); };
    for (uint32_t e = 0; e < cnt; ++e) {
        const uint32_t j = ldsA[e * BLOCK];
        const float4 c = gv.pts[j];
        const float v = d2_nc(c.x, c.y, c.z, q.x, q.y, q.z);
        uint32_t r = 0;
#pragma unroll
        for (int i = 0; i < L; ++i) r += (d[i] < v) ? 1u : 0u;
        while (is_taken(r)) ++r;
        if (r < 64) taken_lo |= 1ull << r; else if (r < 128) taken_hi |= 1ull << (r - 64); else taken_x |= 1ull << (r - 128);
        ldsB[r * BLOCK] = (uint8_t)e;
    }
    uint32_t within = 0;          // radius search: the entries with d2 <= radius^2 (nearest_neighbor.rs:271), a prefix
    for (uint32_t r = 0; r < cnt; ++r) {
        const float4 c = gv.pts[ldsA[(uint32_t)ldsB[r * BLOCK] * BLOCK]];
        const float v = d2_nc(c.x, c.y, c.z, q.x, q.y, q.z);
        out_idx[(size_t)t * k + r] = __float_as_uint(c.w);
        out_dist[(size_t)t * k + r] = sqrtf(v);                                       // nearest_neighbor.rs:249
        within += (v <= radius_sq) ? 1u : 0u;
    }
    out_count[t] = within;
}

// ---- unbounded radius search: NearestNeighborSearch::find_radius_neighbors (nearest_neighbor.rs:254-298) ----------
// every cloud point with d2 <= radius^2, two launches: count per query, then fill at the caller's offsets (grid scan
// order; the callers sort by distance like the reference's final sort_by).
template <bool EXT, bool FILL>
__global__ void __launch_bounds__(128) radius_all_kernel(GridView gv, const float *__restrict__ queries, uint32_t nq, float radius,
                                                        uint32_t *__restrict__ counts, const unsigned long long *__restrict__ offsets,
                                                        uint32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq) return;
    const GridGeom &g = gv.g;
    float4 q;
    q.x = queries[3 * (size_t)t]; q.y = queries[3 * (size_t)t + 1]; q.z = queries[3 * (size_t)t + 2]; q.w = 0.0f;
    if (!finite_query(q.x, q.y, q.z)) { if (!FILL) counts[t] = 0; return; }
    const QueryPlace pl = place_query<EXT>(g, q);
    const int cx = pl.cx, cy = pl.cy, cz = pl.cz;
    const float r2 = radius * radius;                                                 // nearest_neighbor.rs:259
    const int R = ball_rings(g, radius);
    const unsigned long long base = FILL ? offsets[t] : 0ull;
    uint32_t cnt = 0;
    scan_pruned<EXT>(gv, q, cx, cy, cz, -1, R, r2 * kWalkSlack, [&](uint32_t, const float4 &c) {
        const float v = d2_nc(c.x, c.y, c.z, q.x, q.y, q.z);
        if (v <= r2) {                                                                 // :271
            if (FILL) { out_idx[base + cnt] = __float_as_uint(c.w); out_dist[base + cnt] = sqrtf(v); }
            ++cnt;
        }
    });
    if (!FILL) counts[t] = cnt;
}

tc_status launch_radius_all(tc_context *ctx, const DeviceIndex &ix, const float *d_queries, size_t nq, float radius, uint32_t *d_counts,
                            const unsigned long long *d_offsets, uint32_t *d_idx, float *d_dist) {
    const GridView gv = view_of(ix);
    ProfScope ps(ctx, d_offsets ? "radius_fill" : "radius_count");
    const dim3 grid((unsigned)((nq + 127) / 128)), block(128);
    hipStream_t st = ctx->stream;
    with_clamped(gv, [&](auto ext) {
        constexpr bool EXT = decltype(ext)::value;
        if (!d_offsets) hipLaunchKernelGGL((radius_all_kernel<EXT, false>), grid, block, 0, st, gv, d_queries, (uint32_t)nq, radius, d_counts, nullptr, nullptr, nullptr);
        else hipLaunchKernelGGL((radius_all_kernel<EXT, true>), grid, block, 0, st, gv, d_queries, (uint32_t)nq, radius, nullptr, d_offsets, d_idx, d_dist);
    });
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

// what every k-NN kernel takes behind the index
struct KnnArgs {
    const float *queries; uint32_t nq, k;
    uint32_t *idx; float *dist; uint32_t *count;
    float radius_sq;
};
// the register-list kernel with L entries, BLOCK queries per block
template <int L, int BLOCK>
static void launch_knn_list(hipStream_t st, const GridView &gv, const KnnArgs &a) {
    with_clamped(gv, [&](auto ext) {
        hipLaunchKernelGGL((knn_kernel<L, BLOCK, decltype(ext)::value>), dim3((unsigned)(((size_t)a.nq + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, gv, a.queries, a.nq, a.k,
                           a.idx, a.dist, a.count, a.radius_sq);
    });
}

tc_status launch_knn(tc_context *ctx, const DeviceIndex &ix, const float *d_queries, size_t nq, size_t k,
                     uint32_t *d_idx, float *d_dist, uint32_t *d_count, float radius_sq) {
    if (k > 2048) return fail(ctx, TC_UNSUPPORTED, "k > 2048 is not supported by the HIP k-NN export");
    const GridView gv = view_of(ix);
    ProfScope ps(ctx, "knn_batch");
    hipStream_t st = ctx->stream;
    const KnnArgs a{d_queries, (uint32_t)nq, (uint32_t)k, d_idx, d_dist, d_count, radius_sq};
    if (k > 129) {          // beyond the register list: a block per query (knn_coop_kernel)
        const dim3 grid((unsigned)std::min<size_t>(nq, 1u << 16)), block(kCoopThreads);
        if (k <= 256) hipLaunchKernelGGL(knn_coop_kernel<512>, grid, block, 0, st, gv, a.queries, a.nq, a.k, a.idx, a.dist, a.count, a.radius_sq);
        else hipLaunchKernelGGL(knn_coop_kernel<4096>, grid, block, 0, st, gv, a.queries, a.nq, a.k, a.idx, a.dist, a.count, a.radius_sq);
    }
    else if (k <= 9)  launch_knn_list<9, 256>(st, gv, a);
    else if (k <= 17) launch_knn_list<17, 256>(st, gv, a);
    else if (k <= 33) launch_knn_list<33, 128>(st, gv, a);
    else if (k <= 65) launch_knn_list<65, 64>(st, gv, a);
    else              launch_knn_list<129, 64>(st, gv, a);
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points -------------------------------------------------------------------------------
struct tc_search_index {
    tc_context *ctx;
    tc::DeviceIndex ix;
    size_t n;
    tc::DevBuf q, out;          // staged queries / results of the host-buffer calls
};

static tc_status no_neighbours(tc_context *ctx, uint32_t *d_count, size_t nq) {        // the empty result of a device entry point
    TC_HIP_TRY(ctx, hipMemsetAsync(d_count, 0, nq * sizeof(uint32_t), ctx->stream));
    return synced(ctx);
}

// One staging block holds a search's results: idx (nq x k) | dist (nq x k) | count (nq)
struct SearchOut { uint32_t *idx; float *dist; uint32_t *count; };
static tc_status search_out_layout(tc_context *ctx, DevBuf &block, size_t nq, size_t k, SearchOut *o) {
    if (tc_status s = ensure(ctx, block, nq * k * 8 + nq * 4)) return s;
    o->idx = (uint32_t *)block.p; o->dist = (float *)(o->idx + nq * k); o->count = (uint32_t *)(o->dist + nq * k);
    return TC_OK;
}
static tc_status search_out_download(tc_context *ctx, const SearchOut &o, size_t nq, size_t k, uint32_t *idx, float *dist, uint32_t *count) {
    TC_HIP_TRY(ctx, hipMemcpyAsync(idx, o.idx, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    TC_HIP_TRY(ctx, hipMemcpyAsync(dist, o.dist, nq * k * 4, hipMemcpyDeviceToHost, ctx->stream));
    return stage_out(ctx, count, o.count, nq * 4);
}

// tc_knn (radius == nullptr) / tc_radius_search behind their own argument checks: cloud and queries through the context's staging
// buffers, the device entry point, the three arrays back
static tc_status search_from_host(tc_context *ctx, const float *cloud, size_t n, const float *queries, size_t nq, size_t k, const float *radius,
                                  uint32_t *idx, float *dist, uint32_t *count) {
    if (tc_status s = ensure(ctx, ctx->in_a, n * 3 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, ctx->in_b, nq * 3 * sizeof(float))) return s;
    SearchOut o;
    if (tc_status s = search_out_layout(ctx, ctx->out_a, nq, k, &o)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_a.p, cloud, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_b.p, queries, nq * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    const float *d_cloud = (const float *)ctx->in_a.p, *d_queries = (const float *)ctx->in_b.p;
    if (tc_status s = radius ? tc_radius_search_device(ctx, d_cloud, n, d_queries, nq, *radius, k, o.idx, o.dist, o.count)
                             : tc_knn_device(ctx, d_cloud, n, d_queries, nq, k, o.idx, o.dist, o.count)) return s;
    return search_out_download(ctx, o, nq, k, idx, dist, count);
}

extern "C" {
// ---- batch k-NN (nearest_neighbor.rs:177-251; gpu/nearest_neighbor.rs:332-355) ----------------
tc_status tc_knn_device(tc_context *ctx, const float *d_cloud, size_t n, const float *d_queries, size_t nq, size_t k,
                        uint32_t *d_idx, float *d_dist, uint32_t *d_count) try {
    if (!ctx) return TC_INVALID_DATA;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (k == 0 || n == 0) return no_neighbours(ctx, d_count, nq);           // nearest_neighbor.rs:178-180: empty result
    if (tc_status s = check_point_count(ctx, n, nq)) return s;
    if (k > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k > 2048 is not supported by the HIP k-NN export");
    if (tc_status s = build_index(ctx, ctx->tgt_index, d_cloud, n, knn_grid(k))) return s;
    if (tc_status s = launch_knn(ctx, ctx->tgt_index, d_queries, nq, k, d_idx, d_dist, d_count)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

// ---- radius search export (nearest_neighbor.rs:254-298; gpu_find_radius_neighbors gpu/nearest_neighbor.rs:357-367) ----
tc_status tc_radius_search_device(tc_context *ctx, const float *d_cloud, size_t n, const float *d_queries, size_t nq, float radius, size_t k_max,
                                  uint32_t *d_idx, float *d_dist, uint32_t *d_count) try {
    if (!ctx) return TC_INVALID_DATA;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!(radius > 0.0f) || n == 0 || k_max == 0) return no_neighbours(ctx, d_count, nq);       // nearest_neighbor.rs:255-257: empty result
    if (tc_status s = check_point_count(ctx, n, nq)) return s;
    if (k_max > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k_max > 2048 is not supported by the HIP radius search");
    if (tc_status s = build_index(ctx, ctx->tgt_index, d_cloud, n, knn_grid(k_max))) return s;
    if (tc_status s = launch_knn(ctx, ctx->tgt_index, d_queries, nq, k_max, d_idx, d_dist, d_count, radius * radius)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_radius_search(tc_context *ctx, const float *cloud, size_t n, const float *queries, size_t nq, float radius, size_t k_max,
                           uint32_t *idx, float *dist, uint32_t *count) try {
    if (!ctx) return TC_INVALID_DATA;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!(radius > 0.0f) || n == 0 || k_max == 0) { std::memset(count, 0, nq * sizeof(uint32_t)); return TC_OK; }
    if (k_max > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k_max > 2048 is not supported by the HIP radius search");
    return search_from_host(ctx, cloud, n, queries, nq, k_max, &radius, idx, dist, count);
} TC_CATCH_STATUS(ctx)

tc_status tc_knn(tc_context *ctx, const float *cloud, size_t n, const float *queries, size_t nq, size_t k,
                 uint32_t *idx, float *dist, uint32_t *count) try {
    if (!ctx) return TC_INVALID_DATA;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (k == 0 || n == 0) { std::memset(count, 0, nq * sizeof(uint32_t)); return TC_OK; }
    if (k > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k > 2048 is not supported by the HIP k-NN export");      // before any buffer is sized by k
    return search_from_host(ctx, cloud, n, queries, nq, k, nullptr, idx, dist, count);
} TC_CATCH_STATUS(ctx)

// ---- persistent search index: KdTree::new once, many find_k_nearest / find_radius_neighbors calls --------------
// (threecrate-core/src/traits.rs:6-12; nearest_neighbor.rs:37-58, :177-298; Python KdTree lib.rs:707-776)
tc_status tc_search_index_create_device(tc_context *ctx, const float *d_cloud, size_t n, size_t k_hint, tc_search_index **out) try {
    if (!ctx || !out) return TC_INVALID_DATA;
    *out = nullptr;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status rc = check_point_count(ctx, n)) return rc;
    tc_search_index *s = new tc_search_index{ctx, {}, n, {}, {}};
    if (n) {        // an empty cloud is an empty tree (nearest_neighbor.rs:38-45)
        const size_t k = std::min<size_t>(std::max<size_t>(k_hint, 1), 129);
        tc_status rc = build_index(ctx, s->ix, d_cloud, n, knn_grid(k));
        if (rc == TC_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, TC_GPU, "search index build failed");
        if (rc != TC_OK) { free_index(s->ix); delete s; return rc; }
        // queries only need the sorted records and the cell starts: drop the build scratch (16 B per point)
        for_each_scratch_buf(s->ix, free_buf);
    }
    *out = s;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

tc_status tc_search_index_create(tc_context *ctx, const float *cloud, size_t n, size_t k_hint, tc_search_index **out) try {
    if (!ctx || !out) return TC_INVALID_DATA;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n) if (tc_status s = stage_in(ctx, ctx->in_a, cloud, n * 3 * sizeof(float))) return s;
    return tc_search_index_create_device(ctx, (const float *)ctx->in_a.p, n, k_hint, out);   // the index holds its own sorted copy
} TC_CATCH_STATUS(ctx)

size_t tc_search_index_size(const tc_search_index *s) { return s ? s->n : 0; }

// radius < 0: k nearest; radius >= 0: the neighbours within radius among the k nearest
tc_status tc_search_index_query_device(tc_search_index *s, const float *d_queries, size_t nq, size_t k, float radius,
                                       uint32_t *d_idx, float *d_dist, uint32_t *d_count) try {
    if (!s) return TC_INVALID_DATA;
    tc_context *ctx = s->ctx;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool by_radius = radius >= 0.0f;
    if (k == 0 || s->n == 0 || (by_radius && !(radius > 0.0f))) return no_neighbours(ctx, d_count, nq);     // nearest_neighbor.rs:178-180, :255-257
    if (k > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k > 2048 is not supported by the HIP neighbour search");
    if (tc_status rc = check_point_count(ctx, nq)) return rc;
    if (tc_status rc = launch_knn(ctx, s->ix, d_queries, nq, k, d_idx, d_dist, d_count, by_radius ? radius * radius : INFINITY)) return rc;
    return synced(ctx);
} TC_CATCH_STATUS((s ? s->ctx : nullptr))

tc_status tc_search_index_query(tc_search_index *s, const float *queries, size_t nq, size_t k, float radius, uint32_t *idx, float *dist,
                                uint32_t *count) try {
    if (!s) return TC_INVALID_DATA;
    tc_context *ctx = s->ctx;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (k == 0 || s->n == 0) { std::memset(count, 0, nq * sizeof(uint32_t)); return TC_OK; }
    if (k > kMaxK) return fail(ctx, TC_UNSUPPORTED, "k > 2048 is not supported by the HIP neighbour search");
    SearchOut o;
    if (tc_status rc = search_out_layout(ctx, s->out, nq, k, &o)) return rc;
    if (tc_status rc = stage_in(ctx, s->q, queries, nq * 3 * sizeof(float))) return rc;
    if (tc_status rc = tc_search_index_query_device(s, (const float *)s->q.p, nq, k, radius, o.idx, o.dist, o.count)) return rc;
    return search_out_download(ctx, o, nq, k, idx, dist, count);
} TC_CATCH_STATUS((s ? s->ctx : nullptr))

// find_radius_neighbors without a cap (nearest_neighbor.rs:254-298): count, then fill at the caller's offsets
tc_status tc_search_index_radius_count(tc_search_index *s, const float *queries, size_t nq, float radius, uint32_t *counts) try {
    if (!s) return TC_INVALID_DATA;
    tc_context *ctx = s->ctx;
    if (nq == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!(radius > 0.0f) || s->n == 0) { std::memset(counts, 0, nq * sizeof(uint32_t)); return TC_OK; }      // :255-257
    if (tc_status rc = check_point_count(ctx, nq)) return rc;
    if (tc_status rc = ensure(ctx, s->out, nq * sizeof(uint32_t))) return rc;
    if (tc_status rc = stage_in(ctx, s->q, queries, nq * 3 * sizeof(float))) return rc;
    if (tc_status rc = launch_radius_all(ctx, s->ix, (const float *)s->q.p, nq, radius, (uint32_t *)s->out.p, nullptr, nullptr, nullptr)) return rc;
    return stage_out(ctx, counts, s->out.p, nq * sizeof(uint32_t));
} TC_CATCH_STATUS((s ? s->ctx : nullptr))

tc_status tc_search_index_radius_fill(tc_search_index *s, const float *queries, size_t nq, float radius, const uint64_t *offsets, size_t total,
                                      uint32_t *idx, float *dist) try {
    if (!s) return TC_INVALID_DATA;
    tc_context *ctx = s->ctx;
    if (nq == 0 || total == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!(radius > 0.0f) || s->n == 0) return fail(ctx, TC_INVALID_DATA, "radius fill: nothing to fill for this radius (total must be 0)");
    const size_t q_bytes = (nq * 3 * sizeof(float) + 7) / 8 * 8;
    if (tc_status rc = ensure(ctx, s->q, q_bytes + nq * sizeof(uint64_t))) return rc;
    if (tc_status rc = ensure(ctx, s->out, total * 8)) return rc;
    float *d_q = (float *)s->q.p;
    unsigned long long *d_off = (unsigned long long *)((char *)s->q.p + q_bytes);
    uint32_t *d_idx = (uint32_t *)s->out.p;
    float *d_dist = (float *)(d_idx + total);
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_q, queries, nq * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, nq * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    if (tc_status rc = launch_radius_all(ctx, s->ix, d_q, nq, radius, nullptr, d_off, d_idx, d_dist)) return rc;
    TC_HIP_TRY(ctx, hipMemcpyAsync(idx, d_idx, total * 4, hipMemcpyDeviceToHost, ctx->stream));
    return stage_out(ctx, dist, d_dist, total * 4);
} TC_CATCH_STATUS((s ? s->ctx : nullptr))

void tc_search_index_destroy(tc_search_index *s) try {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    free_index(s->ix);
    free_buf(s->q); free_buf(s->out);
    delete s;
} TC_CATCH_VOID
}  // extern "C"
