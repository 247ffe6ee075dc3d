// fpfh.hip -- FPFH descriptors (threecrate-algorithms/src/features.rs:173-259): per point three 11-bin histograms of the Darboux
// frame angles (alpha, phi, theta) of its pairs, SPFH(p) + the 1 / dist weighted mean of its neighbours' SPFH, renormalised.
//
//   index     the grid index of grid.hip (cell edge ~ r / 2, like cluster.hip), the normals gathered into cell-sorted order;
//   spfh      one lane per sorted point walks its ball (scan_pruned, j != p, d2_nc <= r^2) and counts the pair bins into a column
//             of LDS counters (dynamic bin indices: registers would go to scratch); a point whose ball holds fewer than k others is
//             appended to the fallback list instead;
//   fallback  launch_knn(k + 1) at the fallback points, self dropped, the first k kept (find_neighbors, features.rs:131-159);
//             the same SPFH counting over those lists;
//   sum       one lane per point walks the same neighbour set again and accumulates w * SPFH(j) in 33 registers (static indices),
//             then renormalises; row `orig` of the output.
// SPFH rows are (float)count * (1.0f / valid): the reference's `h *= scale` over integer counts, so bit-identical.  No float atomics
// anywhere: descriptors are bit-identical from run to run.  Every operation of the pair features is the reference's f32 operation in
// the reference's order (-ffp-contract=off, correctly rounded sqrtf and division, nalgebra's component formulas).
//
// Lane per point against wave per point (one 64-lane wave per point walking each span of the ball together, LDS integer atomics for
// the SPFH counts, a fixed shuffle tree for the 34 sums), device call in ms, 1x MI355X, median of 5 (tools/fpfh_bench.py):
//   workload                       lane    wave      (SPFH + sum, lane / wave)
//   KITTI-shaped 120 k, r 0.5      1.49    1.21      1.39 / 1.06
//   KITTI-shaped 120 k, r 1.0      4.18    2.08      4.03 / 1.99
//   uniform 100 k, r 0.1 (~400)    2.19    1.57      2.08 / 1.45
//   uniform 1 M, r 0.023 (~30)     2.54   13.86      2.26 / 13.07
//   TUM-shaped 1 M, r 0.02         7.54   12.46      7.25 / 12.17
// A wave per point wins by 1.2-2x on the 100 k-point clouds with large balls and loses by 2-5x at a million points, where the
// per-wave row walk and the reduction cost more than the ball's records: lane per point is kept.  A per-point split (a wave for
// the points whose ball count, known after the SPFH walk, is large) is the way to take both.
#include "tc_internal.h"
#include "knn_list.h"

#include <cmath>

namespace tc {

constexpr int kFpfhBins = 11;
constexpr int kFpfhRow = 36;            // an SPFH row: 33 floats padded to nine float4
constexpr int kFpfhBlock = 256;         // 33 u32 LDS counters per lane: 33 KiB per block
constexpr size_t kFpfhKnnEntries = size_t(1) << 25;     // k-NN lists held at once (u32 index + f32 distance each)

// to_bin (features.rs:74-78): `as usize` saturates (NaN and negative values -> 0), then min(n_bins - 1)
__device__ __forceinline__ int fpfh_bin(float value, float lo, float hi) {
    const float t = (value - lo) / (hi - lo) * (float)kFpfhBins;
    return !(t > 0.0f) ? 0 : (t >= (float)(kFpfhBins - 1) ? kFpfhBins - 1 : (int)t);
}

// compute_pair_features (features.rs:38-70) + the three bins; false: the pair is skipped (dist < 1e-10 or |n_s x d| < 1e-10).
// nalgebra: cross = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x); dot = a0 b0 + a1 b1 + a2 b2, left to right, no
// leading zero; magnitude = sqrt(0 + (x x + y y + z z)) (the zero is exact for a sum of squares); vector / scalar per component.
__device__ __forceinline__ bool fpfh_pair(const float4 &ps, const float4 &ns, const float4 &pt, const float4 &nt, int &ba, int &bp,
                                          int &bt) {
    const float dx = pt.x - ps.x, dy = pt.y - ps.y, dz = pt.z - ps.z;
    const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
    if (dist < 1e-10f) return false;
    const float d0 = dx / dist, d1 = dy / dist, d2 = dz / dist;
    const float vx = ns.y * d2 - ns.z * d1, vy = ns.z * d0 - ns.x * d2, vz = ns.x * d1 - ns.y * d0;
    const float vm = sqrtf(vx * vx + vy * vy + vz * vz);
    if (vm < 1e-10f) return false;
    const float ux = vx / vm, uy = vy / vm, uz = vz / vm;
    const float wx = ns.y * uz - ns.z * uy, wy = ns.z * ux - ns.x * uz, wz = ns.x * uy - ns.y * ux;
    const float alpha = ux * nt.x + uy * nt.y + uz * nt.z;
    const float phi = ns.x * d0 + ns.y * d1 + ns.z * d2;
    const float theta = atan2f(wx * nt.x + wy * nt.y + wz * nt.z, ns.x * nt.x + ns.y * nt.y + ns.z * nt.z);
    const float pi = 3.14159265358979323846f;                // std::f32::consts::PI
    ba = fpfh_bin(alpha, -1.0f, 1.0f);
    bp = kFpfhBins + fpfh_bin(phi, -1.0f, 1.0f);
    bt = 2 * kFpfhBins + fpfh_bin(theta, -pi, pi);
    return true;
}

__device__ __forceinline__ void fpfh_hist_clear(uint32_t *h) {
#pragma unroll
    for (int b = 0; b < 3 * kFpfhBins; ++b) h[b * kFpfhBlock] = 0u;
}

// the SPFH row of sorted point p: count * (1.0f / valid) (features.rs:115-121); all zero without a valid pair
__device__ __forceinline__ void fpfh_hist_store(const uint32_t *h, uint32_t valid, float *__restrict__ row) {
    const float scale = valid ? 1.0f / (float)valid : 0.0f;
    float4 *r4 = reinterpret_cast<float4 *>(row);
#pragma unroll
    for (int q = 0; q < kFpfhRow / 4; ++q) {
        float v[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int b = 4 * q + c;
            v[c] = b < 3 * kFpfhBins ? (float)h[b * kFpfhBlock] * scale : 0.0f;
        }
        r4[q] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

__global__ void __launch_bounds__(256) fpfh_split_kernel(const float *__restrict__ np6, uint32_t n, float *__restrict__ xyz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyz[3 * (size_t)i] = np6[6 * (size_t)i];
    xyz[3 * (size_t)i + 1] = np6[6 * (size_t)i + 1];
    xyz[3 * (size_t)i + 2] = np6[6 * (size_t)i + 2];
}

__global__ void __launch_bounds__(256) fpfh_rank_kernel(const float4 *__restrict__ pts, uint32_t n, uint32_t *__restrict__ sorted_of) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) sorted_of[__float_as_uint(pts[p].w)] = p;
}

// SPFH of the radius neighbourhood (find_neighbors' first branch + compute_spfh), one lane per finite sorted point.  mode[p]:
// 0 = radius list, 1 = fallback (listed in fb_pos / fb_xyz), 2 = inert (a non-finite point: all-zero descriptor)
template <bool EXT>
__global__ void __launch_bounds__(kFpfhBlock) fpfh_spfh_kernel(GridView gv, const float4 *__restrict__ nrm, uint32_t n, float r2, int R,
                                                               uint32_t k, float *__restrict__ spfh, uint32_t *__restrict__ mode,
                                                               uint32_t *__restrict__ fb_count, uint32_t *__restrict__ fb_pos,
                                                               float *__restrict__ fb_xyz) {
    __shared__ uint32_t hist[3 * kFpfhBins * kFpfhBlock];
    const uint32_t p = blockIdx.x * kFpfhBlock + threadIdx.x;
    if (p >= n) return;
    const float4 q = gv.pts[p];
    if (p >= gv.cell_start[gv.g.ncell] || !finite_query(q.x, q.y, q.z)) { mode[p] = 2u; return; }
    const QueryPlace pl = place_query<EXT>(gv.g, q);
    const float4 nq = nrm[p];
    uint32_t *h = hist + threadIdx.x;
    fpfh_hist_clear(h);
    uint32_t cnt = 0, valid = 0;
    scan_pruned<EXT>(gv, q, pl.cx, pl.cy, pl.cz, -1, R, r2, [&](uint32_t j, const float4 &c) {
        if (j != p && d2_nc(c.x, c.y, c.z, q.x, q.y, q.z) <= r2) {       // nearest_neighbor.rs:271, features.rs:141-145
            ++cnt;
            int ba, bp, bt;
            if (fpfh_pair(q, nq, c, nrm[j], ba, bp, bt)) {
                ++h[ba * kFpfhBlock]; ++h[bp * kFpfhBlock]; ++h[bt * kFpfhBlock];
                ++valid;
            }
        }
    });
    if (cnt < k) {                                                        // features.rs:147-158
        const uint32_t s = atomicAdd(fb_count, 1u);
        fb_pos[s] = p;
        fb_xyz[3 * (size_t)s] = q.x; fb_xyz[3 * (size_t)s + 1] = q.y; fb_xyz[3 * (size_t)s + 2] = q.z;
        mode[p] = 1u;
        return;
    }
    mode[p] = 0u;
    fpfh_hist_store(h, valid, spfh + (size_t)kFpfhRow * p);
}

// the fallback list of query s: launch_knn's k + 1 nearest (original indices, ascending), the query itself dropped, the first k kept;
// visits the sorted positions
template <typename F>
__device__ __forceinline__ void fpfh_fb_list(const uint32_t *__restrict__ idx, uint32_t m, uint32_t k, uint32_t self,
                                             const uint32_t *__restrict__ sorted_of, F &&f) {
    uint32_t taken = 0;
    for (uint32_t e = 0; e < m && taken < k; ++e) {
        const uint32_t o = idx[e];
        if (o == self) continue;
        ++taken;
        f(sorted_of[o]);
    }
}

__global__ void __launch_bounds__(kFpfhBlock) fpfh_spfh_fb_kernel(const float4 *__restrict__ pts, const float4 *__restrict__ nrm, uint32_t nf,
                                                                  const uint32_t *__restrict__ fb_pos, const uint32_t *__restrict__ idx,
                                                                  const uint32_t *__restrict__ cnt, uint32_t k1, uint32_t k,
                                                                  const uint32_t *__restrict__ sorted_of, float *__restrict__ spfh) {
    __shared__ uint32_t hist[3 * kFpfhBins * kFpfhBlock];
    const uint32_t s = blockIdx.x * kFpfhBlock + threadIdx.x;
    if (s >= nf) return;
    const uint32_t p = fb_pos[s];
    const float4 q = pts[p], nq = nrm[p];
    uint32_t *h = hist + threadIdx.x;
    fpfh_hist_clear(h);
    uint32_t valid = 0;
    fpfh_fb_list(idx + (size_t)s * k1, cnt[s], k, __float_as_uint(q.w), sorted_of, [&](uint32_t j) {
        int ba, bp, bt;
        if (fpfh_pair(q, nq, pts[j], nrm[j], ba, bp, bt)) {
            ++h[ba * kFpfhBlock]; ++h[bp * kFpfhBlock]; ++h[bt * kFpfhBlock];
            ++valid;
        }
    });
    fpfh_hist_store(h, valid, spfh + (size_t)kFpfhRow * p);
}

// features.rs:221-255 for one point: acc += (1 / dist) * SPFH(j) over the list, then SPFH(p) + acc / weight_sum, each sub-histogram
// divided by its sum
struct FpfhAcc {
    float acc[3 * kFpfhBins];
    float wsum = 0.0f;
    uint32_t nb = 0;
    __device__ __forceinline__ FpfhAcc() {
#pragma unroll
        for (int b = 0; b < 3 * kFpfhBins; ++b) acc[b] = 0.0f;
    }
    __device__ __forceinline__ void add(const float4 &pi, const float4 &pj, const float *__restrict__ row) {
        ++nb;
        const float dx = pj.x - pi.x, dy = pj.y - pi.y, dz = pj.z - pi.z;
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (dist < 1e-10f) return;
        const float w = 1.0f / dist;
        wsum += w;
        const float4 *r4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
        for (int q = 0; q < kFpfhRow / 4; ++q) {
            const float4 v = r4[q];
            if (4 * q + 0 < 3 * kFpfhBins) acc[4 * q + 0] += w * v.x;
            if (4 * q + 1 < 3 * kFpfhBins) acc[4 * q + 1] += w * v.y;
            if (4 * q + 2 < 3 * kFpfhBins) acc[4 * q + 2] += w * v.z;
            if (4 * q + 3 < 3 * kFpfhBins) acc[4 * q + 3] += w * v.w;
        }
    }
    __device__ __forceinline__ void finish(const float *__restrict__ own, float *__restrict__ out) {
        float d[3 * kFpfhBins];
#pragma unroll
        for (int b = 0; b < 3 * kFpfhBins; ++b) d[b] = own[b];
        if (nb && wsum > 0.0f) {
            const float inv_w = 1.0f / wsum;
#pragma unroll
            for (int b = 0; b < 3 * kFpfhBins; ++b) d[b] += inv_w * acc[b];
#pragma unroll
            for (int part = 0; part < 3; ++part) {
                float sum = 0.0f;
#pragma unroll
                for (int b = 0; b < kFpfhBins; ++b) sum += d[part * kFpfhBins + b];
                if (sum > 0.0f) {
#pragma unroll
                    for (int b = 0; b < kFpfhBins; ++b) d[part * kFpfhBins + b] /= sum;
                }
            }
        }
#pragma unroll
        for (int b = 0; b < 3 * kFpfhBins; ++b) out[b] = d[b];
    }
};

// the radius points (mode 0) and the inert ones (mode 2: zeros); the fallback points are fpfh_sum_fb_kernel's
template <bool EXT>
__global__ void __launch_bounds__(128) fpfh_sum_kernel(GridView gv, uint32_t n, float r2, int R, const uint32_t *__restrict__ mode,
                                                      const float *__restrict__ spfh, float *__restrict__ out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t md = mode[p];
    if (md == 1u) return;
    const float4 q = gv.pts[p];
    float *o = out + 3 * kFpfhBins * (size_t)__float_as_uint(q.w);
    if (md == 2u) {
#pragma unroll
        for (int b = 0; b < 3 * kFpfhBins; ++b) o[b] = 0.0f;
        return;
    }
    const QueryPlace pl = place_query<EXT>(gv.g, q);
    FpfhAcc a;
    scan_pruned<EXT>(gv, q, pl.cx, pl.cy, pl.cz, -1, R, r2, [&](uint32_t j, const float4 &c) {
        if (j != p && d2_nc(c.x, c.y, c.z, q.x, q.y, q.z) <= r2) a.add(q, c, spfh + (size_t)kFpfhRow * j);
    });
    a.finish(spfh + (size_t)kFpfhRow * p, o);
}

__global__ void __launch_bounds__(128) fpfh_sum_fb_kernel(const float4 *__restrict__ pts, uint32_t nf, const uint32_t *__restrict__ fb_pos,
                                                         const uint32_t *__restrict__ idx, const uint32_t *__restrict__ cnt, uint32_t k1,
                                                         uint32_t k, const uint32_t *__restrict__ sorted_of, const float *__restrict__ spfh,
                                                         float *__restrict__ out) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nf) return;
    const uint32_t p = fb_pos[s];
    const float4 q = pts[p];
    const uint32_t orig = __float_as_uint(q.w);
    FpfhAcc a;
    fpfh_fb_list(idx + (size_t)s * k1, cnt[s], k, orig, sorted_of, [&](uint32_t j) { a.add(q, pts[j], spfh + (size_t)kFpfhRow * j); });
    a.finish(spfh + (size_t)kFpfhRow * p, out + 3 * kFpfhBins * (size_t)orig);
}

tc_status fpfh_device(tc_context *ctx, const float *d_np6, size_t n, float radius, size_t k, float *d_out) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    const float r2 = radius * radius;                                   // nearest_neighbor.rs:259
    const bool ball = r2 <= r2;                                         // a NaN radius: no radius neighbour, every point falls back
    const bool finite_ball = ball && r2 <= 3.0e38f;
    auto &B = ctx->fpfh;            // (what each slot holds: enum FpfhSlot, tc_internal.h)
    const std::pair<FpfhSlot, size_t> need[] = {{FPFH_XYZ, n * 3 * sizeof(float)}, {FPFH_SPFH, n * kFpfhRow * sizeof(float)}, {FPFH_MODE, n * sizeof(uint32_t)},
                                                {FPFH_FB_POS, n * sizeof(uint32_t)}, {FPFH_FB_XYZ, n * 3 * sizeof(float)},
                                                {FPFH_SORTED_OF, n * sizeof(uint32_t)}, {FPFH_FB_COUNT, 4 * sizeof(uint32_t)}};
    for (const auto &[slot, bytes] : need) if (tc_status s = ensure(ctx, B[slot], bytes)) return s;
    float *xyz = (float *)B[FPFH_XYZ].p, *spfh = (float *)B[FPFH_SPFH].p, *fb_xyz = (float *)B[FPFH_FB_XYZ].p;
    uint32_t *mode = (uint32_t *)B[FPFH_MODE].p, *fb_pos = (uint32_t *)B[FPFH_FB_POS].p, *sorted_of = (uint32_t *)B[FPFH_SORTED_OF].p, *fb_count = (uint32_t *)B[FPFH_FB_COUNT].p;
    const unsigned nb = (unsigned)((n + 255) / 256);

    DeviceIndex &ix = ctx->tgt_index;
    {
        ProfScope ps(ctx, "fpfh_index");
        hipLaunchKernelGGL(fpfh_split_kernel, dim3(nb), dim3(256), 0, st, d_np6, n32, xyz);
        TC_HIP_TRY(ctx, hipMemsetAsync(fb_count, 0, sizeof(uint32_t), st));
    }
    if (tc_status s = build_index(ctx, ix, xyz, n, ball_grid(radius, true))) return s;
    {
        ProfScope ps(ctx, "fpfh_index");
        if (tc_status s = gather_normals(ctx, ix, d_np6 + 3, 6)) return s;
        hipLaunchKernelGGL(fpfh_rank_kernel, dim3(nb), dim3(256), 0, st, (const float4 *)ix.pts.p, n32, sorted_of);
    }
    const GridView gv = view_of(ix);
    const float4 *nrm = (const float4 *)ix.normals.p;
    // cells further than R from the query's (clamped) cell hold no point of the ball; R = -1: no cell at all (NaN radius)
    const int gmax = std::max(gv.g.gx, std::max(gv.g.gy, gv.g.gz));
    const int R = !ball ? -1 : !finite_ball ? gmax : ball_rings(gv.g, radius);
    const uint32_t k32 = (uint32_t)k;
    {
        ProfScope ps(ctx, "fpfh_spfh");
        with_clamped(gv, [&](auto ext) {
            hipLaunchKernelGGL(fpfh_spfh_kernel<decltype(ext)::value>, dim3(nb), dim3(kFpfhBlock), 0, st, gv, nrm, n32, r2, R, k32, spfh, mode, fb_count, fb_pos, fb_xyz);
        });
    }
    uint32_t nf = 0;
    if (k) {
        if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, fb_count, sizeof(uint32_t))) return s;
        nf = pinned_host(ctx)->count;
    }
    // the fallback lists: launch_knn(k + 1) in chunks of at most kFpfhKnnEntries entries; with more than one chunk the lists are
    // searched again for the sum pass (every SPFH has to be there before any sum starts)
    const size_t k1 = k + 1;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(nf, kFpfhKnnEntries / k1));
    const bool one_chunk = chunk >= nf;
    if (nf) {
        if (tc_status s = ensure(ctx, B[FPFH_KNN_IDX], chunk * k1 * sizeof(uint32_t))) return s;
        if (tc_status s = ensure(ctx, B[FPFH_KNN_DIST], chunk * k1 * sizeof(float))) return s;
        if (tc_status s = ensure(ctx, B[FPFH_KNN_COUNT], chunk * sizeof(uint32_t))) return s;
    }
    uint32_t *kidx = (uint32_t *)B[FPFH_KNN_IDX].p, *kcnt = (uint32_t *)B[FPFH_KNN_COUNT].p;
    float *kdist = (float *)B[FPFH_KNN_DIST].p;
    for (size_t c0 = 0; c0 < nf; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, nf - c0);
        ProfScope ps(ctx, "fpfh_knn_fallback");
        if (tc_status s = launch_knn(ctx, ix, fb_xyz + 3 * c0, m, k1, kidx, kdist, kcnt)) return s;
        hipLaunchKernelGGL(fpfh_spfh_fb_kernel, dim3((m + kFpfhBlock - 1) / kFpfhBlock), dim3(kFpfhBlock), 0, st, (const float4 *)ix.pts.p, nrm, m,
                           (const uint32_t *)fb_pos + c0, (const uint32_t *)kidx, (const uint32_t *)kcnt, (uint32_t)k1, k32,
                           (const uint32_t *)sorted_of, spfh);
    }
    {
        ProfScope ps(ctx, "fpfh_sum");
        const dim3 grid((n32 + 127) / 128), block(128);
        with_clamped(gv, [&](auto ext) {
            hipLaunchKernelGGL(fpfh_sum_kernel<decltype(ext)::value>, grid, block, 0, st, gv, n32, r2, R, (const uint32_t *)mode, (const float *)spfh, d_out);
        });
    }
    for (size_t c0 = 0; c0 < nf; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, nf - c0);
        if (!one_chunk) {
            ProfScope ps(ctx, "fpfh_knn_fallback");
            if (tc_status s = launch_knn(ctx, ix, fb_xyz + 3 * c0, m, k1, kidx, kdist, kcnt)) return s;
        }
        ProfScope ps(ctx, "fpfh_sum");
        hipLaunchKernelGGL(fpfh_sum_fb_kernel, dim3((m + 127) / 128), dim3(128), 0, st, (const float4 *)ix.pts.p, m, (const uint32_t *)fb_pos + c0,
                           (const uint32_t *)kidx, (const uint32_t *)kcnt, (uint32_t)k1, k32, (const uint32_t *)sorted_of, (const float *)spfh, d_out);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- extract_fpfh_features[_with_normals] (features.rs:173-285; the wheel's extract_fpfh_features, lib.rs:1222-1245) ----------
// checks in the reference's order (:177-185); then the limits of this implementation
static tc_status fpfh_validate(tc_context *ctx, size_t n, float radius, size_t k, bool *empty) {
    *empty = false;
    if (!ctx) return TC_INVALID_DATA;
    if (n == 0) { *empty = true; return TC_OK; }
    if (radius <= 0.0f) return fail(ctx, TC_INVALID_DATA, "search_radius must be positive");
    if (k > kMaxK - 1) return fail(ctx, TC_UNSUPPORTED, "extract_fpfh_features: k_neighbors > 2047 is not supported by the HIP backend");
    return check_point_count(ctx, n);
}

// the wheel: estimate_normals(cloud, k) (normals.rs:238-247, its k >= 3 check first), then the descriptors with (radius, k)
static tc_status fpfh_xyz_validate(tc_context *ctx, size_t n, float radius, size_t k, bool *empty) {
    *empty = false;
    if (!ctx) return TC_INVALID_DATA;
    if (n == 0) { *empty = true; return TC_OK; }
    if (k < 3) return fail(ctx, TC_INVALID_DATA, "k_neighbors must be at least 3");
    return fpfh_validate(ctx, n, radius, k, empty);
}

static tc_status fpfh_from_xyz(tc_context *ctx, const float *d_xyz, size_t n, float radius, size_t k, float *d_out) {
    tc_normal_config cfg;
    tc_normal_config_default(&cfg);
    cfg.k_neighbors = k;
    if (tc_status s = ensure(ctx, ctx->fpfh_np, n * 6 * sizeof(float))) return s;
    // the normals' index (cell edge for k neighbours) is rebuilt by fpfh_device for the radius: the normals stay on the device
    if (tc_status s = normals_on_index(ctx, ctx->tgt_index, true, 0.0f, d_xyz, n, &cfg, (float *)ctx->fpfh_np.p, 0, (size_t)-1, false, nullptr)) return s;
    return fpfh_device(ctx, (const float *)ctx->fpfh_np.p, n, radius, k, d_out);
}

extern "C" {
tc_status tc_extract_fpfh_features_with_normals_device(tc_context *ctx, const float *d_normal_points, size_t n, float search_radius,
                                                       size_t k_neighbors, float *d_out) try {
    bool empty;
    if (tc_status s = fpfh_validate(ctx, n, search_radius, k_neighbors, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = fpfh_device(ctx, d_normal_points, n, search_radius, k_neighbors, d_out)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_extract_fpfh_features_with_normals(tc_context *ctx, const float *normal_points, size_t n, float search_radius,
                                                size_t k_neighbors, float *out) try {
    bool empty;
    if (tc_status s = fpfh_validate(ctx, n, search_radius, k_neighbors, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->out_a, n * TC_FPFH_DIM * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_a, normal_points, n * 6 * sizeof(float))) return s;
    if (tc_status s = fpfh_device(ctx, (const float *)ctx->in_a.p, n, search_radius, k_neighbors, (float *)ctx->out_a.p)) return s;
    return stage_out(ctx, out, ctx->out_a.p, n * TC_FPFH_DIM * sizeof(float));
} TC_CATCH_STATUS(ctx)

tc_status tc_extract_fpfh_features_device(tc_context *ctx, const float *d_xyz, size_t n, float search_radius, size_t k_neighbors,
                                          float *d_out) try {
    bool empty;
    if (tc_status s = fpfh_xyz_validate(ctx, n, search_radius, k_neighbors, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = fpfh_from_xyz(ctx, d_xyz, n, search_radius, k_neighbors, d_out)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_extract_fpfh_features(tc_context *ctx, const float *xyz, size_t n, float search_radius, size_t k_neighbors, float *out) try {
    bool empty;
    if (tc_status s = fpfh_xyz_validate(ctx, n, search_radius, k_neighbors, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->out_a, n * TC_FPFH_DIM * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = fpfh_from_xyz(ctx, (const float *)ctx->in_a.p, n, search_radius, k_neighbors, (float *)ctx->out_a.p)) return s;
    return stage_out(ctx, out, ctx->out_a.p, n * TC_FPFH_DIM * sizeof(float));
} TC_CATCH_STATUS(ctx)
}  // extern "C"
