// outlier.hip -- statistical_outlier_removal[_with_threshold] and radius_outlier_removal
// (threecrate-algorithms/src/filtering.rs:167-395); the entry points of include/threecrate_hip_filters.h.
//
// The reference asks its kd-tree for the k + 1 nearest of every point (:279), drops the entries that equal the point (:287), and
// averages the rest in ascending order (:295); then a global mean / standard deviation of those means gives the threshold
// (:300-309) and the points with mean <= threshold are kept in input order (:312-318).  Only the distance MULTISET of the k + 1
// nearest is needed, which is what the first phase of knn_kernel (search.hip) leaves in its sorted register list: the kernel here
// stops there -- no position lists, no collect pass, no ranking, no n x (k + 1) output.
//   sor_mean      a lane per cell-sorted point (k + 1 <= 129) or a block per point (coop_nearest): mean[original index]
//   sor_stats     mean and population variance of mean[] in f64, two passes, per-block partials in a fixed layout folded by one
//                 block: no float atomics, the threshold has the same bits on every run
//   flag, exclusive_scan_u32, compact   kept points and their indices in input order (store_compacted, as compact_flagged); shared
//                 with the radius filter
//   radius_keep   the ball walk of radius_all_kernel over self-queries, count >= min_neighbors + 1 (self included, :199)
#include "tc_internal.h"
#include "knn_list.h"
#include "knn_coop.h"
#include "../../include/threecrate_hip_filters.h"

#include <algorithm>
#include <cmath>

namespace tc {

// ---- per-point mean distance ------------------------------------------------------------------
// knn_kernel's first phase (search.hip) with the cell-sorted records as their own queries; then the mean over the list.
// The phase is written out here, not shared through an inline function: behind one, knn_kernel's register allocation changes
// (L = 17: 73 -> 104 VGPRs, L = 65: 122 -> 179) and this kernel's too (L = 65: 119 -> 168), with the same source text.
template <int L, int BLOCK, bool EXT>
__global__ void __launch_bounds__(BLOCK) sor_mean_kernel(GridView gv, uint32_t n, uint32_t k1, float *__restrict__ mean) {
    const uint32_t p = blockIdx.x * BLOCK + threadIdx.x;
    if (p >= n) return;
    const GridGeom &g = gv.g;
    const float4 q = gv.pts[p];
    const uint32_t orig = __float_as_uint(q.w);
    const uint32_t nfin = gv.cell_start[g.ncell];
    if (p >= nfin) { mean[orig] = NAN; return; }             // the non-finite bucket behind the last cell: inert
    const QueryPlace pl = place_query<EXT>(g, q);
    const int cx = pl.cx, cy = pl.cy, cz = pl.cz;
    const float mf = pl.mf, out2 = pl.out2;
    const uint32_t K1 = min(k1, nfin);
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
        float live_lim = tau;
        const bool touched = scan_pruned<EXT, true>(gv, q, cx, cy, cz, Rin, R, live_lim, [&](uint32_t j, const float4 &c) {
            visit1(j, c);
            if (growing) live_lim = d[L - 1];
        }, &live_lim);
        if (!touched) break;
    }
    // d[0 .. K1) is the ascending distance multiset of the K1 nearest, the point itself (d2 == 0) among them.  Static indices
    // under a predicate: a dynamic index would send the list to scratch.
    float sum = 0.0f;
    uint32_t cnt = 0;
#pragma unroll
    for (int i = 0; i < L; ++i) {
        if ((uint32_t)i < K1 && d[i] > 0.0f) { sum += sqrtf(d[i]); ++cnt; }     // filtering.rs:287 (skip self), :295 (sequential f32 sum)
    }
    mean[orig] = cnt ? sum / (float)cnt : 0.0f;                                  // :291-295
}

// k + 1 beyond the register list: a block per point, the sorted keys of coop_nearest summed in order by thread 0
template <int CAPB>
__global__ void __launch_bounds__(kCoopThreads) sor_mean_coop_kernel(GridView gv, uint32_t n, uint32_t k1, float *__restrict__ mean) {
    __shared__ CoopShared<CAPB> sh;
    const GridGeom &g = gv.g;
    const int tid = threadIdx.x;
    const uint32_t nfin = gv.cell_start[g.ncell];
    const uint32_t K1 = min(k1, nfin);
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const float4 q = gv.pts[p];
        const uint32_t orig = __float_as_uint(q.w);
        if (p >= nfin) {
            if (tid == 0) mean[orig] = NAN;
            continue;
        }
        const uint32_t total = coop_nearest<CAPB>(gv, q.x, q.y, q.z, K1, nfin, sh);
        if (tid == 0) {
            const uint32_t m = min(K1, total);
            float sum = 0.0f;
            uint32_t cnt = 0;
            for (uint32_t r = 0; r < m; ++r) {
                const float v = __uint_as_float((uint32_t)(sh.buf[r] >> 32));
                if (v > 0.0f) { sum += sqrtf(v); ++cnt; }
            }
            mean[orig] = cnt ? sum / (float)cnt : 0.0f;
        }
        __syncthreads();
    }
}

// ---- global statistics (filtering.rs:300-309, in f64) -------------------------------------------
constexpr int kStatBlock = 256;
constexpr int kStatMaxBlocks = 1024;
struct SorStats {
    double partial[kStatMaxBlocks];
    double mean;            // of the finite points' mean distances
    float  threshold;
    uint32_t result[2];     // what the host reads back in one copy: kept count, threshold bits
};

__device__ __forceinline__ double block_sum_f64(double acc, double *sh) {
    sh[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int s = kStatBlock / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}

// PASS 0: the sum of the means; PASS 1: the sum of (mean - m)^2.  The entries of inert points are NaN and take no part.
// Thread t of block b folds elements b * 256 + t, + gridDim.x * 256, ... in that order: the layout is a function of n alone.
template <int PASS>
__global__ void __launch_bounds__(kStatBlock) sor_stat_partial_kernel(const float *__restrict__ mean, uint32_t n, SorStats *st) {
    __shared__ double sh[kStatBlock];
    const double m = PASS ? st->mean : 0.0;
    double acc = 0.0;
    for (size_t i = (size_t)blockIdx.x * kStatBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kStatBlock) {
        const float x = mean[i];
        if (x == x) {
            const double v = (double)x - m;
            acc += PASS ? v * v : v;
        }
    }
    const double total = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) st->partial[blockIdx.x] = total;
}

template <int PASS>
__global__ void __launch_bounds__(kStatBlock) sor_stat_fold_kernel(SorStats *st, uint32_t nb, const uint32_t *__restrict__ nfin_p, float mult) {
    __shared__ double sh[kStatBlock];
    double acc = 0.0;
    for (uint32_t b = threadIdx.x; b < nb; b += kStatBlock) acc += st->partial[b];
    const double total = block_sum_f64(acc, sh);
    if (threadIdx.x == 0) {
        const double cnt = (double)*nfin_p;                     // the divisor: the finite points
        if (PASS == 0) st->mean = total / cnt;
        else st->threshold = (float)(st->mean + (double)mult * sqrt(total / cnt));      // :308-309, rounded once
    }
}

// ---- flag, compact ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sor_flag_kernel(const float *__restrict__ mean, uint32_t n, const float *__restrict__ thr_dev, float thr_val,
                                                      uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float thr = thr_dev ? *thr_dev : thr_val;
    flag[i] = (mean[i] <= thr) ? 1u : 0u;                        // :316; a NaN mean (inert point) or a NaN threshold keeps nothing
}

__global__ void __launch_bounds__(256) finite_flag_kernel(const float *__restrict__ xyz, uint32_t n, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    flag[i] = finite_query(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) ? 1u : 0u;
}

// compact_flagged_kernel (grid.hip) with two duties of its own: the gate, and the two words the host reads back (count, threshold bits).
// gated: the flags mark the finite points and all of them are kept when there are more than gate_min of them, else none (an
// infinite ball: every finite point has nfin - 1 neighbours).
__global__ void __launch_bounds__(256) outlier_compact_kernel(const float *__restrict__ xyz, uint32_t n, const uint32_t *__restrict__ flag,
                                                             const uint32_t *__restrict__ pos, int gated, unsigned long long gate_min,
                                                             const float *__restrict__ thr_dev, float thr_val, float *__restrict__ out_xyz,
                                                             uint32_t *__restrict__ kept_index, uint32_t *__restrict__ result) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t total = pos[n];
    const bool open = !gated || (unsigned long long)total > gate_min;
    if (i == 0) {
        result[0] = open ? total : 0u;
        result[1] = __float_as_uint(thr_dev ? *thr_dev : thr_val);
    }
    if (i >= n || !open || !flag[i]) return;
    store_compacted(xyz, i, pos[i], out_xyz, kept_index);
}

// ---- radius filter ------------------------------------------------------------------------------
// one lane per cell-sorted point: the records with d2 <= r2, the point itself among them (find_radius_neighbors, then
// saturating_sub(1), filtering.rs:197-199); kept when count - 1 >= min_neighbors, compared in 64 bits (:208)
template <bool EXT>
__global__ void __launch_bounds__(128) radius_keep_kernel(GridView gv, uint32_t n, float r2, int R, unsigned long long min_neighbors,
                                                         uint32_t *__restrict__ flag) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const GridGeom &g = gv.g;
    const float4 q = gv.pts[p];
    const uint32_t orig = __float_as_uint(q.w);
    if (p >= gv.cell_start[g.ncell]) { flag[orig] = 0u; return; }
    const QueryPlace pl = place_query<EXT>(g, q);
    uint32_t cnt = 0;
    scan_pruned<EXT>(gv, q, pl.cx, pl.cy, pl.cz, -1, R, r2, [&](uint32_t, const float4 &c) {
        cnt += (d2_nc(c.x, c.y, c.z, q.x, q.y, q.z) <= r2) ? 1u : 0u;             // nearest_neighbor.rs:271
    });
    flag[orig] = ((unsigned long long)cnt > min_neighbors) ? 1u : 0u;
}

// ---- host side ------------------------------------------------------------------------------------
namespace {

// the temporaries of one call, one block: statistics | mean (when the caller wants none) | flags | positions (n + 1)
struct OutlierTemps {
    ScopedBuf block;
    SorStats *stats = nullptr;
    float *mean = nullptr;
    uint32_t *flag = nullptr, *pos = nullptr;
    tc_status take(tc_context *ctx, size_t n, bool own_mean) {
        const size_t words = (own_mean ? n : 0) + n + (n + 1);
        if (tc_status s = ensure(ctx, block, sizeof(SorStats) + words * sizeof(uint32_t))) return s;
        stats = (SorStats *)block.p;
        uint32_t *w = (uint32_t *)(stats + 1);
        if (own_mean) { mean = (float *)w; w += n; }
        flag = w; pos = w + n;
        return TC_OK;
    }
};

// scan the flags, write the kept points, bring the count (and the threshold) back in one read
tc_status compact_and_count(tc_context *ctx, const float *d_xyz, size_t n, OutlierTemps &t, DeviceIndex &ix, bool gated, unsigned long long gate_min,
                            const float *thr_dev, float thr_val, float *d_out_xyz, uint32_t *d_kept_index, size_t *n_out, float *threshold_used) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    {
        ProfScope ps(ctx, "outlier_compact");
        if (tc_status s = exclusive_scan_u32(ctx, t.flag, n32, t.pos, ix.blocksum)) return s;
        hipLaunchKernelGGL(outlier_compact_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_xyz, n32, (const uint32_t *)t.flag,
                           (const uint32_t *)t.pos, gated ? 1 : 0, gate_min, thr_dev, thr_val, d_out_xyz, d_kept_index, t.stats->result);
    }
    uint32_t *h = pinned_host(ctx)->filter_out;
    if (tc_status s = read_back(ctx, h, t.stats->result, 2 * sizeof(uint32_t))) return s;
    *n_out = h[0];
    if (threshold_used) __builtin_memcpy(threshold_used, &h[1], sizeof(float));
    return TC_OK;
}

template <int L, int BLOCK>
void launch_sor_list(hipStream_t st, const GridView &gv, uint32_t n, uint32_t k1, float *mean) {
    with_clamped(gv, [&](auto ext) {
        hipLaunchKernelGGL((sor_mean_kernel<L, BLOCK, decltype(ext)::value>), dim3((unsigned)(((size_t)n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, gv, n, k1, mean);
    });
}

}  // namespace

// a validated call (n >= 1, 1 <= k <= 2047).  with_threshold: `param` is the threshold, else the standard deviation multiplier
tc_status sor_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k, bool with_threshold, float param, float *d_out_xyz,
                     uint32_t *d_kept_index, float *d_mean, size_t *n_out, float *threshold_used) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n, k1 = (uint32_t)k + 1;
    OutlierTemps t;
    if (tc_status s = t.take(ctx, n, d_mean == nullptr)) return s;
    float *mean = d_mean ? d_mean : t.mean;
    DeviceIndex &ix = ctx->tgt_index;
    if (tc_status s = build_index(ctx, ix, d_xyz, n, knn_grid(k1))) return s;
    const GridView gv = view_of(ix);
    {
        ProfScope ps(ctx, "sor_mean");
        if (k1 > 129) {         // beyond the register list (launch_knn's hand-over)
            const dim3 grid((unsigned)std::min<size_t>(n, 1u << 16)), block(kCoopThreads);
            if (k1 <= 256) hipLaunchKernelGGL(sor_mean_coop_kernel<512>, grid, block, 0, st, gv, n32, k1, mean);
            else hipLaunchKernelGGL(sor_mean_coop_kernel<4096>, grid, block, 0, st, gv, n32, k1, mean);
        }
        else if (k1 <= 9)  launch_sor_list<9, 256>(st, gv, n32, k1, mean);
        else if (k1 <= 17) launch_sor_list<17, 256>(st, gv, n32, k1, mean);
        else if (k1 <= 33) launch_sor_list<33, 128>(st, gv, n32, k1, mean);
        else if (k1 <= 65) launch_sor_list<65, 64>(st, gv, n32, k1, mean);
        else               launch_sor_list<129, 64>(st, gv, n32, k1, mean);
    }
    const unsigned nb = (unsigned)((n + 255) / 256);
    const float *thr_dev = nullptr;
    if (!with_threshold) {
        ProfScope ps(ctx, "sor_stats");
        const uint32_t sb = (uint32_t)std::min<size_t>((n + kStatBlock - 1) / kStatBlock, kStatMaxBlocks);
        const uint32_t *nfin_p = gv.cell_start + gv.g.ncell;
        hipLaunchKernelGGL(sor_stat_partial_kernel<0>, dim3(sb), dim3(kStatBlock), 0, st, (const float *)mean, n32, t.stats);
        hipLaunchKernelGGL(sor_stat_fold_kernel<0>, dim3(1), dim3(kStatBlock), 0, st, t.stats, sb, nfin_p, param);
        hipLaunchKernelGGL(sor_stat_partial_kernel<1>, dim3(sb), dim3(kStatBlock), 0, st, (const float *)mean, n32, t.stats);
        hipLaunchKernelGGL(sor_stat_fold_kernel<1>, dim3(1), dim3(kStatBlock), 0, st, t.stats, sb, nfin_p, param);
        thr_dev = &t.stats->threshold;
    }
    {
        ProfScope ps(ctx, "sor_flag");
        hipLaunchKernelGGL(sor_flag_kernel, dim3(nb), dim3(256), 0, st, (const float *)mean, n32, thr_dev, param, t.flag);
    }
    return compact_and_count(ctx, d_xyz, n, t, ix, false, 0ull, thr_dev, param, d_out_xyz, d_kept_index, n_out, threshold_used);
}

// a validated call (n >= 1, min_neighbors >= 1, radius > 0 or NaN)
tc_status radius_outlier_device(tc_context *ctx, const float *d_xyz, size_t n, float radius, size_t min_neighbors, float *d_out_xyz,
                                uint32_t *d_kept_index, size_t *n_out) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    const float r2 = radius * radius;                               // nearest_neighbor.rs:259
    *n_out = 0;
    if (!(r2 <= r2)) return TC_OK;                                  // NaN: `d2 <= NaN` holds for nothing, nothing is kept
    OutlierTemps t;
    if (tc_status s = t.take(ctx, n, false)) return s;
    const unsigned nb = (unsigned)((n + 255) / 256);
    DeviceIndex &ix = ctx->tgt_index;
    if (std::isinf(r2)) {       // the ball holds every finite point: nfin - 1 neighbours each, no index and no walk
        {
            ProfScope ps(ctx, "radius_keep");
            hipLaunchKernelGGL(finite_flag_kernel, dim3(nb), dim3(256), 0, st, d_xyz, n32, t.flag);
        }
        return compact_and_count(ctx, d_xyz, n, t, ix, true, (unsigned long long)min_neighbors, nullptr, 0.0f, d_out_xyz, d_kept_index, n_out, nullptr);
    }
    if (tc_status s = build_index(ctx, ix, d_xyz, n, ball_grid(radius, false))) return s;
    const GridView gv = view_of(ix);
    {
        ProfScope ps(ctx, "radius_keep");
        const dim3 grid((unsigned)((n + 127) / 128)), block(128);
        with_clamped(gv, [&](auto ext) {
            hipLaunchKernelGGL(radius_keep_kernel<decltype(ext)::value>, grid, block, 0, st, gv, n32, r2, ball_rings(gv.g, radius), (unsigned long long)min_neighbors, t.flag);
        });
    }
    return compact_and_count(ctx, d_xyz, n, t, ix, false, 0ull, nullptr, 0.0f, d_out_xyz, d_kept_index, n_out, nullptr);
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_filters.h) ------------------------------------------------
// checks in the reference's order (filtering.rs:254-268, :340-354), then the limits of this implementation
static tc_status sor_validate(tc_context *ctx, size_t n, size_t k, float param, const char *param_msg, size_t *n_out, bool *empty) {
    *empty = false;
    if (!ctx || !n_out) return TC_INVALID_DATA;
    *n_out = 0;
    if (n == 0) { *empty = true; return TC_OK; }
    if (k == 0) return fail(ctx, TC_INVALID_DATA, "k_neighbors must be greater than 0");
    if (param <= 0.0f) return fail(ctx, TC_INVALID_DATA, param_msg);
    if (k > kMaxK - 1) return fail(ctx, TC_UNSUPPORTED, "statistical_outlier_removal: k_neighbors > 2047 is not supported by the HIP backend");
    return check_point_count(ctx, n);
}

// (:172-186)
static tc_status radius_validate(tc_context *ctx, size_t n, float radius, size_t min_neighbors, size_t *n_out, bool *empty) {
    *empty = false;
    if (!ctx || !n_out) return TC_INVALID_DATA;
    *n_out = 0;
    if (n == 0) { *empty = true; return TC_OK; }
    if (radius <= 0.0f) return fail(ctx, TC_INVALID_DATA, "radius must be positive");
    if (min_neighbors == 0) return fail(ctx, TC_INVALID_DATA, "min_neighbors must be greater than 0");
    return check_point_count(ctx, n);
}

// the host twins: the cloud through in_a, the device road (`run`: cloud, then the three outputs in out_a, out_xyz | kept_index |
// mean_distance, the first two null when the caller wants none), the wanted arrays back under one wait
template <class Run>
static tc_status outlier_host(tc_context *ctx, const float *xyz, size_t n, float *out_xyz, uint32_t *kept_index, float *mean_distance, size_t *n_out,
                              Run run) {
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, ctx->out_a, n * 5 * sizeof(float))) return s;
    float *d_out = (float *)ctx->out_a.p, *d_mean = d_out + 4 * n;
    uint32_t *d_kept = (uint32_t *)(d_out + 3 * n);
    if (tc_status s = run((const float *)ctx->in_a.p, out_xyz ? d_out : nullptr, kept_index ? d_kept : nullptr, d_mean)) return s;
    if (out_xyz && *n_out) TC_HIP_TRY(ctx, hipMemcpyAsync(out_xyz, d_out, *n_out * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (kept_index && *n_out) TC_HIP_TRY(ctx, hipMemcpyAsync(kept_index, d_kept, *n_out * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (mean_distance) return stage_out(ctx, mean_distance, d_mean, n * sizeof(float));
    return synced(ctx);
}

extern "C" {

tc_status tc_statistical_outlier_removal_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k_neighbors, float std_dev_multiplier,
                                                float *d_out_xyz, uint32_t *d_kept_index, float *d_mean_distance, size_t *n_out,
                                                float *threshold_used) try {
    bool empty;
    if (tc_status s = sor_validate(ctx, n, k_neighbors, std_dev_multiplier, "std_dev_multiplier must be positive", n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return sor_device(ctx, d_xyz, n, k_neighbors, false, std_dev_multiplier, d_out_xyz, d_kept_index, d_mean_distance, n_out, threshold_used);
} TC_CATCH_STATUS(ctx)

tc_status tc_statistical_outlier_removal(tc_context *ctx, const float *xyz, size_t n, size_t k_neighbors, float std_dev_multiplier,
                                         float *out_xyz, uint32_t *kept_index, float *mean_distance, size_t *n_out, float *threshold_used) try {
    bool empty;
    if (tc_status s = sor_validate(ctx, n, k_neighbors, std_dev_multiplier, "std_dev_multiplier must be positive", n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return outlier_host(ctx, xyz, n, out_xyz, kept_index, mean_distance, n_out, [&](const float *d_xyz, float *d_out, uint32_t *d_kept, float *d_mean) {
        return sor_device(ctx, d_xyz, n, k_neighbors, false, std_dev_multiplier, d_out, d_kept, d_mean, n_out, threshold_used);
    });
} TC_CATCH_STATUS(ctx)

tc_status tc_statistical_outlier_removal_with_threshold_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k_neighbors, float threshold,
                                                               float *d_out_xyz, uint32_t *d_kept_index, float *d_mean_distance,
                                                               size_t *n_out) try {
    bool empty;
    if (tc_status s = sor_validate(ctx, n, k_neighbors, threshold, "threshold must be positive", n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return sor_device(ctx, d_xyz, n, k_neighbors, true, threshold, d_out_xyz, d_kept_index, d_mean_distance, n_out, nullptr);
} TC_CATCH_STATUS(ctx)

tc_status tc_statistical_outlier_removal_with_threshold(tc_context *ctx, const float *xyz, size_t n, size_t k_neighbors, float threshold,
                                                        float *out_xyz, uint32_t *kept_index, float *mean_distance, size_t *n_out) try {
    bool empty;
    if (tc_status s = sor_validate(ctx, n, k_neighbors, threshold, "threshold must be positive", n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return outlier_host(ctx, xyz, n, out_xyz, kept_index, mean_distance, n_out, [&](const float *d_xyz, float *d_out, uint32_t *d_kept, float *d_mean) {
        return sor_device(ctx, d_xyz, n, k_neighbors, true, threshold, d_out, d_kept, d_mean, n_out, nullptr);
    });
} TC_CATCH_STATUS(ctx)

tc_status tc_radius_outlier_removal_device(tc_context *ctx, const float *d_xyz, size_t n, float radius, size_t min_neighbors, float *d_out_xyz,
                                           uint32_t *d_kept_index, size_t *n_out) try {
    bool empty;
    if (tc_status s = radius_validate(ctx, n, radius, min_neighbors, n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return radius_outlier_device(ctx, d_xyz, n, radius, min_neighbors, d_out_xyz, d_kept_index, n_out);
} TC_CATCH_STATUS(ctx)

tc_status tc_radius_outlier_removal(tc_context *ctx, const float *xyz, size_t n, float radius, size_t min_neighbors, float *out_xyz,
                                    uint32_t *kept_index, size_t *n_out) try {
    bool empty;
    if (tc_status s = radius_validate(ctx, n, radius, min_neighbors, n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return outlier_host(ctx, xyz, n, out_xyz, kept_index, nullptr, n_out, [&](const float *d_xyz, float *d_out, uint32_t *d_kept, float *) {
        return radius_outlier_device(ctx, d_xyz, n, radius, min_neighbors, d_out, d_kept, n_out);
    });
} TC_CATCH_STATUS(ctx)

}  // extern "C"
