// alpha.hip -- alpha-shape surface reconstruction, a point cloud to triangles (alpha_shape_reconstruction, the quality road of
// threecrate-reconstruction/src/alpha_shape.rs); the entry points of include/threecrate_hip_alpha.h, which pins the arithmetic and the order
// of everything.  This unit is the whole of the companion library libthreecrate_hip_alpha.so; the host layer of tc_internal.h (ensure,
// stage_in, read_back, build_index, group_by_key, sort_pairs, exclusive_scan_u32, ProfScope) resolves from libthreecrate_hip.so.
//   The lists, one profile row (alpha_lists):
//   alpha_pack        a thread per point: its 16-byte record; a coordinate that is not finite raises the flag
//   build_index       the cloud in ball_grid(alpha), original indices kept in the records
//   alpha_walk<count> a lane per cell-sorted record: the ball walk of grid_scan.h, counting the j > i with sqrtf(d2) <= alpha; the pair total
//   exclusive_scan_u32   the CSR offsets, by original index
//   -- one read-back: the finite flag and the pair total --
//   alpha_walk<fill>  the same walk: key i << b | j and value j at the point's offset, in walk order
//   sort_pairs        on all 2 b key bits: every list ascending in j, the lists where their offsets say.  One road for every list length and
//                     no threshold, where ordering a list inside a kernel is O(m^2) dependent steps for the one lane that owns a long list
//   The triples, one profile row (alpha_triples): THE HOT PATH, O(n m^2)
//   alpha_triple<W, count>   a sub-group of W lanes per point: the point's neighbour records staged once in LDS (lists of at most kAlphaStage),
//                     its pairs dealt across the lanes in (j, k) order, a ballot prefix giving every candidate its rank inside the point.
//                     Longer lists go row by row, a row's k dealt across the lanes in chunks of W straight from memory: the same order, the
//                     same ranks.  W = 16 packs four points into a wave (short lists), W = 64 gives a point a wave
//   exclusive_scan_u32   over the per-point counts: the global rank of a point's first candidate
//   -- one read-back: the candidate total --
//   alpha_triple<W, emit>    the same enumeration: candidate r = base + rank is written as (i, j, k) with its R2 <= alpha^2 bit, when r is below
//                     the cap.  No triangle is ever sorted
//   The edges, one profile row (alpha_edges): alpha_edge_emit (3 keys lo << b | hi per candidate, value = the candidate), group_by_key,
//   alpha_boundary (a run of one flags its candidate; every writer stores the same word)
//   The write-out, one profile row (alpha_write): alpha_flag (+ the boundary count), exclusive_scan_u32, -- one read-back: the counts --,
//   alpha_write_faces
// Atomics: integer only (atomicOr of the flag, atomicAdd of the three totals: each result is the same whatever the order).
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "knn_list.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_alpha.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// Neighbour records a sub-group stages in LDS per point (16 bytes each): with W = 16 a block of 256 threads serves 16 points and holds
// 16 x 128 x 16 B = 32 KiB, five blocks or 20 waves per CU.  Lists longer than this take the row road.  Not A/B-timed (STATE.md).
constexpr uint32_t kAlphaStage = 128;
// A call whose mean list length (pairs / points) is below this packs four points into a wave (W = 16), else a point has a wave.  Not A/B-timed.
constexpr uint32_t kAlphaPackBelow = 24;
constexpr float kAlphaWalkSlack = 1.000004f;    // the walk's bound on d2 above alpha^2: sqrtf(d2) <= alpha holds for d2 up to alpha^2 (1 + 2^-23)
constexpr uint32_t kAlphaNotFinite = 1u;        // AlphaOut::flags

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void __launch_bounds__(256) alpha_pack_kernel(const float *__restrict__ xyz, uint32_t n, float4 *__restrict__ rec, uint32_t *__restrict__ flags) {
    pack_xyz_records<true>(xyz, n, rec, flags, kAlphaNotFinite);
}

// the header's (1) for the record at sorted position p; FILL: at the point's offset, else counted
template <bool EXT, bool FILL>
__global__ void __launch_bounds__(128) alpha_walk_kernel(GridView gv, uint32_t n, float alpha, int R, float lim, uint32_t *__restrict__ cnt,
                                                        const uint32_t *__restrict__ off, uint32_t b, uint64_t *__restrict__ keys,
                                                        uint32_t *__restrict__ vals, unsigned long long *__restrict__ pairs) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t c = 0;
    if (p < n && p < gv.cell_start[gv.g.ncell]) {               // (a record behind the finite ones: the call fails on the flag)
        const float4 q = gv.pts[p];
        const uint32_t i = __float_as_uint(q.w);
        const QueryPlace pl = place_query<EXT>(gv.g, q);
        uint32_t base = 0, end = 0;
        if (FILL) { base = off[i]; end = off[i + 1]; }
        scan_pruned<EXT>(gv, q, pl.cx, pl.cy, pl.cz, -1, R, lim, [&](uint32_t, const float4 &r) {
            const uint32_t j = __float_as_uint(r.w);
            if (j <= i) return;
            const float dx = q.x - r.x, dy = q.y - r.y, dz = q.z - r.z;
            const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
            if (!(sqrtf((xx + yy) + zz) <= alpha)) return;
            if (FILL && base + c < end) { keys[base + c] = ((uint64_t)i << b) | (uint64_t)j; vals[base + c] = j; }
            ++c;
        });
        if (!FILL) cnt[i] = c;
    }
    if (!FILL) {
        const unsigned long long sum = wave_sum_u64(c);
        if ((threadIdx.x & 63u) == 0u && sum) atomicAdd(pairs, sum);
    }
}

// the header's (3); r2_ok = the R2 half of (6)
__device__ __forceinline__ bool alpha_candidate(const float4 &pi, const float4 &pj, const float4 &pk, float min_area, float alpha2, bool &r2_ok) {
    const float ux = pj.x - pi.x, uy = pj.y - pi.y, uz = pj.z - pi.z;
    const float vx = pk.x - pj.x, vy = pk.y - pj.y, vz = pk.z - pj.z;
    const float wx = pi.x - pk.x, wy = pi.y - pk.y, wz = pi.z - pk.z;
    const float uxx = ux * ux, uyy = uy * uy, uzz = uz * uz, vxx = vx * vx, vyy = vy * vy, vzz = vz * vz, wxx = wx * wx, wyy = wy * wy, wzz = wz * wz;
    const float a2 = (uxx + uyy) + uzz, b2 = (vxx + vyy) + vzz, c2 = (wxx + wyy) + wzz;
    if (!(a2 >= 1e-20f && b2 >= 1e-20f && c2 >= 1e-20f)) return false;
    const float ex = pk.x - pi.x, ey = pk.y - pi.y, ez = pk.z - pi.z;
    const float p0 = uy * ez, p1 = uz * ey, p2 = uz * ex, p3 = ux * ez, p4 = ux * ey, p5 = uy * ex;
    const float cx = p0 - p1, cy = p2 - p3, cz = p4 - p5;
    const float cxx = cx * cx, cyy = cy * cy, czz = cz * cz;
    const float X = (cxx + cyy) + czz;
    const float area_sq = X * 0.25f;
    if (!(area_sq >= 1e-20f)) return false;
    const float R2 = ((a2 * b2) * c2) / (16.0f * area_sq);
    if (R2 == INFINITY) return false;
    const float area = sqrtf(X) * 0.5f;
    if (!(area >= min_area)) return false;
    const float per = (sqrtf(a2) + sqrtf(b2)) + sqrtf(c2);
    if (!(per >= 1e-10f)) return false;
    if (!((4.0f * area) / (per * per) > 0.01f)) return false;
    r2_ok = R2 <= alpha2;
    return true;
}

// pair number t of a list of m (2 <= m <= kAlphaStage, t < m (m - 1) / 2) in lexicographic order: a < b < m
__device__ __forceinline__ void alpha_pair(uint32_t t, uint32_t m, uint32_t &a, uint32_t &b) {
    auto row = [&](uint32_t x) { return x * (2u * m - x - 1u) / 2u; };       // pairs before row x
    const float f = (float)(2u * m - 1u);
    int g = (int)((f - __builtin_amdgcn_sqrtf(fmaxf(f * f - 8.0f * (float)t, 0.0f))) * 0.5f);
    uint32_t x = (uint32_t)min(max(g, 0), (int)m - 2);
    while (x > 0u && row(x) > t) --x;
    while (x + 2u < m && row(x + 1u) <= t) ++x;
    a = x;
    b = min(x + 1u + (t - row(x)), m - 1u);
}

struct AlphaLists {
    const float4 *rec;          // per point, original order
    const uint32_t *off;        // n + 1
    const uint32_t *nbr;        // the lists, ascending
    uint32_t n;
    float min_area, alpha2;
};

// The header's (2) and (3) for point i = the sub-group's number.  EMIT = false: cnt[i] = its candidates, *total += them.  EMIT = true: the
// candidates of global rank base[i] + rank < limit are written.
template <int W, bool EMIT>
__global__ void __launch_bounds__(256) alpha_triple_kernel(AlphaLists a, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ total,
                                                          const uint32_t *__restrict__ base, uint32_t limit, uint32_t *__restrict__ tri,
                                                          uint8_t *__restrict__ ok) {
    constexpr int G = 256 / W;
    __shared__ float4 stage[G][kAlphaStage];
    const uint32_t lane = threadIdx.x & 63u, sl = threadIdx.x % W, sg = threadIdx.x / W;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t mine = W == 64 ? ~0ull : (((1ull << (W & 63)) - 1ull) << (lane - sl));
    const uint64_t i64 = (uint64_t)blockIdx.x * G + sg;
    const uint32_t i = (uint32_t)i64;
    uint32_t s = 0, m = 0;
    if (i64 < a.n) { s = a.off[i]; m = a.off[i + 1] - s; }
    uint64_t gbase = 0;
    if (EMIT && m) { gbase = base[i]; if (gbase >= limit) m = 0; }            // every candidate of the point lies behind the cap
    unsigned long long c = 0;                                   // candidates of the point so far: the same in every lane of the sub-group
    // one trip: `cand` of this lane's pair (j, k); the ranks of the trip's candidates follow the lanes
    auto visit = [&](bool cand, uint32_t j, uint32_t k, bool r2_ok) {
        const uint64_t bal = __ballot(cand) & mine;
        if (EMIT && cand) {
            const uint64_t r = gbase + c + (uint64_t)__popcll(bal & below);
            if (r < limit) {
                tri[3 * r] = i; tri[3 * r + 1] = j; tri[3 * r + 2] = k;
                ok[r] = r2_ok ? 1 : 0;
            }
        }
        c += (unsigned long long)__popcll(bal);
    };
    if (m >= 2u) {
        const float4 pi = a.rec[i];
        if (m <= kAlphaStage) {
            for (uint32_t l = sl; l < m; l += W) {
                const uint32_t j = a.nbr[s + l];
                const float4 r = a.rec[j];
                stage[sg][l] = make_float4(r.x, r.y, r.z, __uint_as_float(j));
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");         // the sub-group's lanes read each other's records: one wave, no barrier
            __builtin_amdgcn_wave_barrier();
            const uint32_t T = m * (m - 1u) / 2u;
            for (uint32_t t0 = 0; t0 < T; t0 += W) {
                if (EMIT && gbase + c >= limit) break;
                const uint32_t t = t0 + sl;
                const bool valid = t < T;
                uint32_t x, y;
                alpha_pair(valid ? t : T - 1u, m, x, y);
                const float4 pj = stage[sg][x], pk = stage[sg][y];
                bool r2_ok = false;
                const bool cand = valid && alpha_candidate(pi, pj, pk, a.min_area, a.alpha2, r2_ok);
                visit(cand, __float_as_uint(pj.w), __float_as_uint(pk.w), r2_ok);
            }
        } else {
            for (uint32_t x = 0; x + 1u < m; ++x) {
                if (EMIT && gbase + c >= limit) break;
                const uint32_t j = a.nbr[s + x];
                const float4 pj = a.rec[j];
                for (uint32_t y0 = x + 1u; y0 < m; y0 += W) {
                    const uint32_t y = y0 + sl;
                    const bool valid = y < m;
                    const uint32_t k = a.nbr[s + (valid ? y : m - 1u)];
                    const float4 pk = a.rec[k];
                    bool r2_ok = false;
                    const bool cand = valid && alpha_candidate(pi, pj, pk, a.min_area, a.alpha2, r2_ok);
                    visit(cand, j, k, r2_ok);
                }
            }
        }
    }
    if (!EMIT) {
        if (i64 < a.n && sl == 0u) cnt[i] = (uint32_t)c;        // (below 2^32 wherever the total is: the host checks the total first)
        const unsigned long long sum = wave_sum_u64(sl == 0u ? c : 0ull);
        if (lane == 0u && sum) atomicAdd(total, sum);
    }
}

__global__ void __launch_bounds__(256) alpha_edge_emit_kernel(const uint32_t *__restrict__ tri, uint32_t t, uint32_t b, uint64_t *__restrict__ keys,
                                                             uint32_t *__restrict__ vals) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= t) return;
    const uint64_t i = tri[3 * (size_t)c], j = tri[3 * (size_t)c + 1], k = tri[3 * (size_t)c + 2];          // i < j < k
    keys[3 * (size_t)c] = (i << b) | j; keys[3 * (size_t)c + 1] = (j << b) | k; keys[3 * (size_t)c + 2] = (i << b) | k;
    vals[3 * (size_t)c] = c; vals[3 * (size_t)c + 1] = c; vals[3 * (size_t)c + 2] = c;
}

// a run of one: the edge's only candidate is a boundary candidate
__global__ void __launch_bounds__(256) alpha_boundary_kernel(const uint32_t *__restrict__ head, const uint32_t *__restrict__ order, uint32_t nk, uint32_t t,
                                                            uint32_t *__restrict__ boundary) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nk || !head[p]) return;
    if (!(p + 1u >= nk || head[p + 1u])) return;
    const uint32_t c = order[p];
    if (c < t) boundary[c] = 1u;                                // every writer stores the same word
}

__global__ void __launch_bounds__(256) alpha_flag_kernel(const uint8_t *__restrict__ ok, const uint32_t *__restrict__ boundary, uint32_t t, uint32_t full,
                                                        uint32_t *__restrict__ flag, uint32_t *__restrict__ n_boundary) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    bool bnd = false;
    if (c < t) {
        bnd = boundary[c] != 0u;
        flag[c] = (ok[c] && (full || bnd)) ? 1u : 0u;
    }
    const uint64_t bal = __ballot(bnd);
    if (bal != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(n_boundary, (uint32_t)__popcll(bal));
}

__global__ void alpha_counts_kernel(const uint32_t *__restrict__ fpos_end, AlphaOut *__restrict__ out) { out->faces = *fpos_end; }

__global__ void __launch_bounds__(256) alpha_write_faces_kernel(const uint32_t *__restrict__ tri, uint32_t t, const uint32_t *__restrict__ flag,
                                                               const uint32_t *__restrict__ fpos, uint32_t *__restrict__ out_faces) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= t || !flag[c]) return;
    const size_t o = fpos[c];                                   // < the count the host has checked the capacity against
#pragma unroll
    for (int e = 0; e < 3; ++e) out_faces[3 * o + e] = tri[3 * (size_t)c + e];
}

// ---- host side -------------------------------------------------------------------------------------------------------------
template <bool EMIT>
static void launch_triples(hipStream_t st, bool pack, const AlphaLists &lists, uint32_t *cnt, unsigned long long *total, const uint32_t *base, uint32_t limit,
                           uint32_t *tri, uint8_t *ok) {
    const size_t n = lists.n;
    if (pack) hipLaunchKernelGGL((alpha_triple_kernel<16, EMIT>), dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, lists, cnt, total, base, limit, tri, ok);
    else hipLaunchKernelGGL((alpha_triple_kernel<64, EMIT>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, lists, cnt, total, base, limit, tri, ok);
}

// a validated call (the header's checks 1 to 5 made); device pointers.  own_faces: the host road's output, sized here once the count is known
static tc_status alpha_on_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_alpha_config &cfg, uint32_t *out_faces, size_t cap_faces,
                                 ScopedBuf *own_faces, tc_alpha_stats *stats) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n;
    const unsigned b = bits_for_value(n - 1);                   // <= 32: a pair key and an edge key have 2 b <= 64 bits
    const float alpha = cfg.alpha, alpha2 = alpha * alpha;
    ScopedBuf counters, rec, cnt, off, blocksum;
    {
        const std::pair<ScopedBuf *, size_t> need[] = {{&counters, sizeof(AlphaOut)}, {&rec, n * sizeof(float4)}, {&cnt, n * sizeof(uint32_t)},
                                                       {&off, (n + 1) * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    AlphaOut *d_out = (AlphaOut *)counters.p;
    float4 *d_rec = (float4 *)rec.p;
    uint32_t *d_cnt = (uint32_t *)cnt.p, *d_off = (uint32_t *)off.p;
    TC_HIP_TRY(ctx, hipMemsetAsync(d_out, 0, sizeof(AlphaOut), st));
    TC_HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, n * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "alpha_lists");
        hipLaunchKernelGGL(alpha_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_xyz, n32, d_rec, &d_out->flags);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    DeviceIndex &ix = ctx->tgt_index;
    if (tc_status s = build_index(ctx, ix, d_xyz, n, ball_grid(alpha, true))) return s;
    const GridView gv = view_of(ix);
    const int R = ball_rings(gv.g, alpha);
    const float lim = alpha2 * kAlphaWalkSlack;
    const dim3 walk_grid((unsigned)((n + 127) / 128)), walk_block(128);
    {
        ProfScope ps(ctx, "alpha_lists");
        with_clamped(gv, [&](auto ext) {
            hipLaunchKernelGGL((alpha_walk_kernel<decltype(ext)::value, false>), walk_grid, walk_block, 0, st, gv, n32, alpha, R, lim, d_cnt, (const uint32_t *)nullptr,
                               (uint32_t)b, (uint64_t *)nullptr, (uint32_t *)nullptr, (unsigned long long *)&d_out->pairs);
        });
        if (tc_status s = exclusive_scan_u32(ctx, d_cnt, n32, d_off, blocksum)) return s;
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    AlphaOut *h = &pinned_host(ctx)->alpha_out;
    if (tc_status s = read_back(ctx, h, d_out, sizeof(AlphaOut))) return s;             // the first wait: the finite flag and the pair total
    if (h->flags & kAlphaNotFinite) return fail(ctx, TC_INVALID_DATA, "alpha_shape: a coordinate is not finite");
    const uint64_t pairs = h->pairs;
    if (pairs >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "alpha_shape: 2^32 - 16 or more neighbour pairs");
    if (pairs < 2) return fail(ctx, TC_ALGORITHM, "No candidate triangles generated");   // no point has two neighbours above it

    ScopedBuf keys, keys_sorted, vals, vals_sorted, sort_temp;
    {
        const std::pair<ScopedBuf *, size_t> need[] = {{&keys, pairs * sizeof(uint64_t)}, {&keys_sorted, pairs * sizeof(uint64_t)}, {&vals, pairs * sizeof(uint32_t)},
                                                       {&vals_sorted, pairs * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    {
        ProfScope ps(ctx, "alpha_lists");
        with_clamped(gv, [&](auto ext) {
            hipLaunchKernelGGL((alpha_walk_kernel<decltype(ext)::value, true>), walk_grid, walk_block, 0, st, gv, n32, alpha, R, lim, (uint32_t *)nullptr,
                               (const uint32_t *)d_off, (uint32_t)b, (uint64_t *)keys.p, (uint32_t *)vals.p, (unsigned long long *)nullptr);
        });
        if (tc_status s = sort_pairs(ctx, (const uint64_t *)keys.p, (uint64_t *)keys_sorted.p, (const uint32_t *)vals.p, (uint32_t *)vals_sorted.p, (size_t)pairs, 2u * b,
                                     sort_temp)) return s;
    }
    TC_HIP_TRY(ctx, hipGetLastError());

    // the count pass over the triples; cnt is free again (the offsets hold the lists), its scan goes where the walk's keys were not: a buffer of its own
    const AlphaLists lists{d_rec, d_off, (const uint32_t *)vals_sorted.p, n32, cfg.min_triangle_area, alpha2};
    const bool pack = pairs / n < kAlphaPackBelow;
    ScopedBuf base;
    if (tc_status s = ensure(ctx, base, (n + 1) * sizeof(uint32_t))) return s;
    uint32_t *d_base = (uint32_t *)base.p;
    {
        ProfScope ps(ctx, "alpha_triples");
        launch_triples<false>(st, pack, lists, d_cnt, (unsigned long long *)&d_out->candidates, nullptr, 0u, nullptr, nullptr);
        if (tc_status s = exclusive_scan_u32(ctx, d_cnt, n32, d_base, blocksum)) return s;
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = read_back(ctx, h, d_out, sizeof(AlphaOut))) return s;             // the second wait: the candidate total
    const uint64_t total = h->candidates;
    if (total >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "alpha_shape: 2^32 - 16 or more candidate triangles");
    const uint64_t t64 = cfg.max_triangles ? std::min<uint64_t>(total, cfg.max_triangles) : total;
    if (3 * t64 >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "alpha_shape: three times the candidate triangles is 2^32 - 16 or more");
    if (t64 == 0) return fail(ctx, TC_ALGORITHM, "No candidate triangles generated");
    const size_t t = (size_t)t64, nk = 3 * t;
    const uint32_t t32 = (uint32_t)t;

    ScopedBuf tri, ok, ekeys, evals, ekeys_sorted, evals_sorted, head, runpos, rstart, boundary, flag, fpos;
    const GroupBufs group{ekeys_sorted, evals_sorted, head, runpos, rstart, sort_temp, blocksum};
    {
        const std::pair<ScopedBuf *, size_t> need[] = {{&tri, nk * sizeof(uint32_t)}, {&ok, t}, {&ekeys, nk * sizeof(uint64_t)}, {&evals, nk * sizeof(uint32_t)},
                                                       {&boundary, t * sizeof(uint32_t)}, {&flag, t * sizeof(uint32_t)}, {&fpos, (t + 1) * sizeof(uint32_t)},
                                                       // group_by_key's buffers, which it would grow itself: sized here, outside the profile rows
                                                       {&ekeys_sorted, nk * sizeof(uint64_t)}, {&evals_sorted, nk * sizeof(uint32_t)}, {&head, nk * sizeof(uint32_t)},
                                                       {&runpos, (nk + 1) * sizeof(uint32_t)}, {&rstart, (nk + 1) * sizeof(uint32_t)}};
        for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    }
    uint32_t *d_tri = (uint32_t *)tri.p, *d_boundary = (uint32_t *)boundary.p, *d_flag = (uint32_t *)flag.p, *d_fpos = (uint32_t *)fpos.p;
    {
        ProfScope ps(ctx, "alpha_triples");
        launch_triples<true>(st, pack, lists, nullptr, nullptr, (const uint32_t *)d_base, t32, d_tri, (uint8_t *)ok.p);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    TC_HIP_TRY(ctx, hipMemsetAsync(d_boundary, 0, t * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "alpha_edges");
        hipLaunchKernelGGL(alpha_edge_emit_kernel, dim3(blocks_for(t)), dim3(256), 0, st, (const uint32_t *)d_tri, t32, (uint32_t)b, (uint64_t *)ekeys.p, (uint32_t *)evals.p);
        KeyGroups runs;
        if (tc_status s = group_by_key(ctx, (const uint64_t *)ekeys.p, (const uint32_t *)evals.p, nk, 2u * b, group, runs)) return s;
        hipLaunchKernelGGL(alpha_boundary_kernel, dim3(blocks_for(nk)), dim3(256), 0, st, (const uint32_t *)runs.head, runs.order, (uint32_t)nk, t32, d_boundary);
    }
    {
        ProfScope ps(ctx, "alpha_write");
        hipLaunchKernelGGL(alpha_flag_kernel, dim3(blocks_for(t)), dim3(256), 0, st, (const uint8_t *)ok.p, (const uint32_t *)d_boundary, t32,
                           cfg.mode == TC_ALPHA_FULL ? 1u : 0u, d_flag, &d_out->boundary);
        if (tc_status s = exclusive_scan_u32(ctx, d_flag, t32, d_fpos, blocksum)) return s;
        hipLaunchKernelGGL(alpha_counts_kernel, dim3(1), dim3(1), 0, st, (const uint32_t *)(d_fpos + t), d_out);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = read_back(ctx, h, d_out, sizeof(AlphaOut))) return s;             // the third wait: the boundary and face counts
    const size_t nf = h->faces;
    if (nf == 0) return fail(ctx, TC_ALGORITHM, "No triangles survived alpha filtering");
    stats->candidates = t64; stats->boundary_candidates = h->boundary; stats->faces = nf; stats->capped = total > t64 ? 1u : 0u;
    if (!out_faces && !own_faces) return TC_OK;                 // the counts alone
    if (cap_faces < nf) return fail(ctx, TC_INVALID_DATA, "alpha_shape: cap_faces is smaller than the number of output faces");
    if (own_faces) {
        if (tc_status s = ensure(ctx, *own_faces, nf * 3 * sizeof(uint32_t))) return s;
        out_faces = (uint32_t *)own_faces->p;
    }
    {
        ProfScope ps(ctx, "alpha_write");
        hipLaunchKernelGGL(alpha_write_faces_kernel, dim3(blocks_for(t)), dim3(256), 0, st, (const uint32_t *)d_tri, t32, (const uint32_t *)d_flag, (const uint32_t *)d_fpos,
                           out_faces);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_alpha.h) ---------------------------------------------------------------------------
// the header's checks (1) to (5), in its order
static tc_status alpha_check(tc_context *ctx, const float *points, size_t n, const tc_alpha_config *cfg, const tc_alpha_stats *stats) {
    if (!ctx) return TC_INVALID_DATA;
    if (!points) return fail(ctx, TC_INVALID_DATA, "alpha_shape: points is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "alpha_shape: config is NULL");
    if (!stats) return fail(ctx, TC_INVALID_DATA, "alpha_shape: stats is NULL");
    if (n == 0) return fail(ctx, TC_INVALID_DATA, "Point cloud is empty");                                       // alpha_shape.rs:125-127
    if (n < 3) return fail(ctx, TC_INVALID_DATA, "Need at least 3 points for triangulation");                    // :152-156
    if (cfg->mode > TC_ALPHA_FULL) return fail(ctx, TC_INVALID_DATA, "alpha_shape: mode is neither TC_ALPHA_BOUNDARY_ONLY nor TC_ALPHA_FULL");
    if (!(cfg->alpha > 0.0f && cfg->alpha <= 3.4028234664e38f)) return fail(ctx, TC_INVALID_DATA, "alpha_shape: alpha is NaN, infinite or not positive");
    if (!(cfg->min_triangle_area >= 0.0f)) return fail(ctx, TC_INVALID_DATA, "alpha_shape: min_triangle_area is negative or NaN");
    if (n >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "alpha_shape: n is 2^32 - 16 or more");
    return TC_OK;
}

extern "C" {

void tc_alpha_config_default(float alpha, tc_alpha_config *cfg) try {
    if (!cfg) return;
    cfg->alpha = alpha;
    cfg->mode = TC_ALPHA_BOUNDARY_ONLY;
    cfg->min_triangle_area = 1e-8f;
    cfg->max_triangles = 50000u;
} TC_CATCH_VOID

tc_status tc_alpha_shape_device(tc_context *ctx, const float *points, size_t n, const tc_alpha_config *cfg, uint32_t *out_faces, size_t cap_faces,
                                tc_alpha_stats *stats) try {
    if (tc_status s = alpha_check(ctx, points, n, cfg, stats)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return alpha_on_device(ctx, points, n, *cfg, out_faces, cap_faces, nullptr, stats);
} TC_CATCH_STATUS(ctx)

tc_status tc_alpha_shape(tc_context *ctx, const float *points, size_t n, const tc_alpha_config *cfg, uint32_t *out_faces, size_t cap_faces,
                         tc_alpha_stats *stats) try {
    if (tc_status s = alpha_check(ctx, points, n, cfg, stats)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, points, n * 3 * sizeof(float))) return s;
    ScopedBuf o_faces;
    if (tc_status s = alpha_on_device(ctx, (const float *)ctx->in_a.p, n, *cfg, nullptr, cap_faces, out_faces ? &o_faces : nullptr, stats)) return s;
    if (!out_faces) return TC_OK;
    TC_HIP_TRY(ctx, hipMemcpyAsync(out_faces, o_faces.p, (size_t)stats->faces * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);                                         // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

}  // extern "C"
