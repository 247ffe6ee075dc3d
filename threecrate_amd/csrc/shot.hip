// shot.hip -- SHOT and USC descriptors with their local reference frame (extract_shot_features_with_normals,
// threecrate-algorithms/src/features.rs:287-645); the entry points of include/threecrate_hip_shot.h, which pins the rule, the arithmetic and
// the deviations.  This unit is the whole of the companion library libthreecrate_hip_shot.so; the host layer of tc_internal.h (ensure,
// stage_in, read_back, build_index, gather_normals, launch_knn, ProfScope) resolves from libthreecrate_hip.so.
//   index          the grid index of grid.hip in ball_grid(radius), the normals gathered into cell-sorted order (FPFH's first stage)
//   shot_ball      THE HOT PATH.  A 64-lane wave per sorted point, four points to a block.  A row has 352 counters (USC: 128), so FPFH's
//                  lane-per-point column of LDS counters does not fit; and FPFH's own table (fpfh.hip) has the wave ahead of the lane from a
//                  few hundred neighbours, which is where the workloads of this descriptor sit (KITTI-shaped at r 0.5 and 1.0, uniform
//                  100 k at r 0.1).  At ~30 neighbours the wave loses there by 2-5x; no packed road for short lists is built (STATE.md).
//                  The wave walks the rows of cells its ball reaches, 64 records a trip.  Two walks of the neighbour set:
//                    walk 1  the count, the z votes and the six covariance sums (f64 per lane, then a fixed xor-shuffle tree), and the
//                            neighbours' dv and sorted position compacted into the wave's LDS stage (ballot + prefix count) while they
//                            fit (kShotStage).  A ball of fewer than k points goes onto the fallback list and the wave leaves
//                    frame   every lane solves the same 3 x 3 eigen-problem (sym3_eigen.h): no broadcast
//                    walk 2  over the stage, or over the grid again for a longer list: the x votes and the bins, integer LDS atomics into
//                            the wave's histogram.  The azimuth is taken with the canonical eigenvector; when the vote negates it the
//                            row is read out four sectors on (the header's deviation), so the vote need not precede the binning
//                    row     a bin per lane and trip: the f64 normalisations, one rounding to f32
//   shot_fallback  the same per-point routine over launch_knn(k + 1)'s list (the query dropped, the first k kept), in chunks of at most
//                  kShotKnnEntries list entries
// Atomics: integer only.  f64 without FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS),
// and the pragma below holds even if a build drops the flag.
#include "tc_internal.h"
#include "grid_scan.h"
#include "knn_list.h"
#include "sym3_eigen.h"
#include "../../include/threecrate_hip_shot.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// Lanes that serve one point: a whole wave.  Not A/B-timed against a part of a wave (STATE.md)
constexpr uint32_t kShotWave = 64;
// Neighbours of a point a wave keeps in LDS between its two walks: 16 bytes each, 8 KiB a wave, 32 KiB a block; a longer list walks the
// grid (or the k-NN list) a second time.  Not A/B-timed (STATE.md)
constexpr uint32_t kShotStage = 512;
constexpr uint32_t kShotWavesPerBlock = 4;
constexpr uint32_t kShotHist = TC_SHOT_DIM + 32;        // the bins, then SHOT's 32 volume totals
constexpr size_t kShotKnnEntries = size_t(1) << 25;     // k-NN list entries held at once (u32 index + f32 distance each): FPFH's figure

struct ShotArgs {
    const float4 *pts, *nrm;    // cell-sorted records (w = the original index's bits) and normals
    float radius;
    float *out, *lrf;           // n x dim; n x 9 or null
    uint32_t *flags;            // n or null
};

__device__ __forceinline__ double shot_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t shot_wave_sum(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o);
    return v;
}
// one wave: its LDS operations are in order, nothing to wait for but the compiler
__device__ __forceinline__ void shot_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// min((usize)t, n - 1) with Rust's saturating cast: NaN and negative values give 0
__device__ __forceinline__ uint32_t shot_sat(double t, uint32_t n) { return !(t > 0.0) ? 0u : (t >= (double)(n - 1u) ? n - 1u : (uint32_t)t); }
__device__ __forceinline__ double shot_clamp(double v) { return fmin(fmax(v, -1.0), 1.0); }      // a NaN gives -1: bin 0, where the saturating cast sends a NaN

// The rows of cells the ball of q reaches (scan_pruned's row logic, Rin = -1), walked by the whole wave: every lane calls
// f(in, j, record) once per trip, `in` = record j is a neighbour of sorted point p.  The trip count is the same in every lane.
template <bool EXT, typename F>
__device__ __forceinline__ void shot_ball_walk(const GridView &gv, const float4 &q, const QueryPlace &pl, int R, float r2, uint32_t p, uint32_t lane, F &&f) {
    const GridGeom &g = gv.g;
    const int x0 = max(pl.cx - R, 0), x1 = min(pl.cx + R, g.gx - 1);
    const int y0 = max(pl.cy - R, 0), y1 = min(pl.cy + R, g.gy - 1);
    const int z0 = max(pl.cz - R, 0), z1 = min(pl.cz + R, g.gz - 1);
    if (x0 > x1) return;                                        // R = -1: no cell at all
    for (int z = z0; z <= z1; ++z) {
        const float gz = axis_gap_n<EXT>(q.z, g.minz, g.h, z, g.gz - 1);
        for (int y = y0; y <= y1; ++y) {
            const float gy = axis_gap_n<EXT>(q.y, g.miny, g.h, y, g.gy - 1);
            const float rg = gy * gy + gz * gz;
            if (rg > r2) continue;
            const float r = TC_FAST_SQRT(fmaxf(r2 - rg, 0.0f)) + 4e-3f * g.h;
            const float fa = fminf(fmaxf((q.x - r - g.minx) * g.inv_h, 0.0f), (float)(g.gx - 1));
            const float fb = fmaxf(fminf((q.x + r - g.minx) * g.inv_h, (float)(g.gx - 1)), 0.0f);
            const int xa = max(x0, (int)fa), xb = min(x1, (int)fb);
            if (xa > xb) continue;
            const uint32_t row = ((uint32_t)z * g.gy + y) * g.gx;
            const uint32_t s = gv.cell_start[row + xa], e = gv.cell_start[row + xb + 1];
            for (uint32_t j0 = s; j0 < e; j0 += kShotWave) {
                const uint32_t j = j0 + lane;
                float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                bool in = false;
                if (j < e) {
                    c = gv.pts[j];
                    in = j != p && d2_nc(c.x, c.y, c.z, q.x, q.y, q.z) <= r2;           // nearest_neighbor.rs:271, features.rs:360-365
                }
                f(in, j, c);
            }
        }
    }
}

// One point, by one wave: the header's (2) to (5) over the list that `walk` visits (walk(f): f(in, j, record) in every lane, the same
// number of times).  Returns false, with nothing written, when the list has fewer than k_min entries (the ball road's way to the fallback).
template <bool USC, typename W>
__device__ __forceinline__ bool shot_point(const ShotArgs &a, const float4 &q, const float4 &nq, uint32_t road, uint32_t k_min, W &&walk, float4 *stage,
                                           uint32_t *hist, uint32_t lane) {
    constexpr uint32_t DIM = USC ? TC_USC_DIM : TC_SHOT_DIM;
    constexpr uint32_t TRIPS = (DIM + kShotWave - 1) / kShotWave;
    const double PI = 3.14159265358979323846;
    const float radius = a.radius;
    const size_t orig = __float_as_uint(q.w);
    // z from the normal
    double zx = 0.0, zy = 0.0, zz = 1.0;
    if (sqrtf((nq.x * nq.x + nq.y * nq.y) + nq.z * nq.z) > 1e-10f) {
        const double m = sqrt(((double)nq.x * (double)nq.x + (double)nq.y * (double)nq.y) + (double)nq.z * (double)nq.z);
        zx = (double)nq.x / m; zy = (double)nq.y / m; zz = (double)nq.z / m;
    }
    // walk 1: the count, the z votes, the covariance; the list into the stage while it fits
    double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0, c4 = 0.0, c5 = 0.0;
    uint32_t zpos = 0, cnt = 0;
    walk([&](bool in, uint32_t j, const float4 &c) {
        const unsigned long long b = __ballot(in);
        if (in) {
            const float dx = c.x - q.x, dy = c.y - q.y, dz = c.z - q.z;
            const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
            const double w = fmax((double)radius - (double)dist, 0.0), X = dx, Y = dy, Z = dz;
            c0 += w * X * X; c1 += w * X * Y; c2 += w * X * Z; c3 += w * Y * Y; c4 += w * Y * Z; c5 += w * Z * Z;
            zpos += ((zx * X + zy * Y) + zz * Z) >= 0.0 ? 1u : 0u;
            const uint32_t slot = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (slot < kShotStage) stage[slot] = make_float4(dx, dy, dz, __uint_as_float(j));
        }
        cnt += (uint32_t)__popcll(b);
    });
    if (cnt < k_min) return false;
    float *row = a.out + orig * DIM;
    if (cnt == 0u) {                                            // features.rs:462, :531
        for (uint32_t b = lane; b < DIM; b += kShotWave) row[b] = 0.0f;
        if (a.lrf && lane < 9u) a.lrf[orig * 9 + lane] = 0.0f;
        if (a.flags && lane == 0u) a.flags[orig] = road | TC_SHOT_EMPTY;
        return true;
    }
    c0 = shot_wave_sum(c0); c1 = shot_wave_sum(c1); c2 = shot_wave_sum(c2); c3 = shot_wave_sum(c3); c4 = shot_wave_sum(c4); c5 = shot_wave_sum(c5);
    zpos = shot_wave_sum(zpos);
    if (2u * zpos < cnt) { zx = -zx; zy = -zy; zz = -zz; }
    // the eigenvector, in every lane alike
    uint32_t fl = road;
    double ex = 1.0, ey = 0.0, ez = 0.0;
    if (!((c0 + c3) + c5 > 0.0)) {
        fl |= TC_SHOT_ZERO_COV;
    } else {
        const double m[6] = {c0, c1, c2, c3, c4, c5};
        double w[3], v[9];
        sym3_eigen(m, w, v);
        ex = v[6]; ey = v[7]; ez = v[8];
        const double ax = fabs(ex), ay = fabs(ey), az = fabs(ez);
        const double lead = (ax >= ay && ax >= az) ? ex : (ay >= az ? ey : ez);
        if (lead < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
    }
    // x with the canonical sign
    double xx, xy, xz;
    bool projected = true;
    {
        const double d = (zx * ex + zy * ey) + zz * ez;
        double px = ex - zx * d, py = ey - zy * d, pz = ez - zz * d;
        double len = sqrt((px * px + py * py) + pz * pz);
        if (!(len > 1e-10)) {
            projected = false;
            px = 1.0 - zx * zx; py = 0.0 - zy * zx; pz = 0.0 - zz * zx;
            len = sqrt((px * px + py * py) + pz * pz);
            if (!(len > 1e-10)) {
                px = 0.0 - zx * zy; py = 1.0 - zy * zy; pz = 0.0 - zz * zy;
                len = sqrt((px * px + py * py) + pz * pz);
            }
        }
        xx = px / len; xy = py / len; xz = pz / len;
    }
    double yx = zy * xz - zz * xy, yy = zz * xx - zx * xz, yz = zx * xy - zy * xx;
    // walk 2: the x votes and the bins
    for (uint32_t b = lane; b < kShotHist; b += kShotWave) hist[b] = 0u;
    shot_wave_sync();
    uint32_t xpos = 0, binned = 0;
    auto visit = [&](float dx, float dy, float dz, uint32_t j) {
        const float dist = sqrtf((dx * dx + dy * dy) + dz * dz);
        const double X = dx, Y = dy, Z = dz;
        xpos += ((ex * X + ey * Y) + ez * Z) >= 0.0 ? 1u : 0u;
        if (dist < 1e-10f || dist > radius) return;
        const double lx = (xx * X + xy * Y) + xz * Z, ly = (yx * X + yy * Y) + yz * Z, lz = (zx * X + zy * Y) + zz * Z;
        const uint32_t ab = shot_sat((atan2(ly, lx) + PI) / (2.0 * PI) * 8.0, 8u);
        if (USC) {
            const uint32_t eb = shot_sat((shot_clamp(lz / (double)dist) - -1.0) / (1.0 - -1.0) * 4.0, 4u);
            const float t = dist / radius * 4.0f;
            const uint32_t rb = !(t > 0.0f) ? 0u : (t >= 3.0f ? 3u : (uint32_t)t);
            atomicAdd(&hist[ab * 16u + eb * 4u + rb], 1u);
        } else {
            const uint32_t rb = dist <= radius * 0.5f ? 0u : 1u, eb = lz < 0.0 ? 0u : 1u;
            const uint32_t vol = rb * 16u + eb * 8u + ab;
            const float4 nj = a.nrm[j];
            const double cs = shot_clamp((zx * (double)nj.x + zy * (double)nj.y) + zz * (double)nj.z);
            atomicAdd(&hist[vol * 11u + shot_sat((cs - -1.0) / (1.0 - -1.0) * 11.0, 11u)], 1u);
            atomicAdd(&hist[TC_SHOT_DIM + vol], 1u);
        }
        ++binned;
    };
    if (cnt <= kShotStage) {
        shot_wave_sync();                                       // (the stage was written by other lanes)
        for (uint32_t t = lane; t < cnt; t += kShotWave) {
            const float4 s = stage[t];
            visit(s.x, s.y, s.z, __float_as_uint(s.w));
        }
    } else {
        walk([&](bool in, uint32_t j, const float4 &c) { if (in) visit(c.x - q.x, c.y - q.y, c.z - q.z, j); });
    }
    shot_wave_sync();
    xpos = shot_wave_sum(xpos);
    binned = shot_wave_sum(binned);
    if (2u * xpos == cnt) fl |= TC_SHOT_X_TIE;
    uint32_t shift = 0;
    if (2u * xpos < cnt && projected) {                         // e is negated: x and y change sign, the azimuth moves by PI
        xx = -xx; xy = -xy; xz = -xz; yx = -yx; yy = -yy; yz = -yz;
        shift = 4u;
    }
    // the row: output azimuth sector s holds what was counted in sector (s + shift) mod 8
    double v[TRIPS], ss = 0.0;
#pragma unroll
    for (uint32_t t = 0; t < TRIPS; ++t) {
        const uint32_t b = lane + t * kShotWave;
        v[t] = 0.0;
        if (b < DIM) {
            if (USC) {
                const uint32_t src = ((((b >> 4) + shift) & 7u) << 4) | (b & 15u);
                v[t] = binned ? (double)hist[src] / (double)binned : 0.0;
            } else {
                const uint32_t vol = b / 11u, src = (vol & ~7u) | ((vol + shift) & 7u);
                const uint32_t total = hist[TC_SHOT_DIM + src];
                v[t] = total ? (double)hist[src * 11u + (b - vol * 11u)] / (double)total : 0.0;
            }
            ss += v[t] * v[t];
        }
    }
    const double norm = sqrt(shot_wave_sum(ss));
#pragma unroll
    for (uint32_t t = 0; t < TRIPS; ++t) {
        const uint32_t b = lane + t * kShotWave;
        if (b < DIM) row[b] = (float)(norm > 1e-10 ? v[t] / norm : v[t]);
    }
    if (lane == 0u) {
        if (a.lrf) {
            float *f = a.lrf + orig * 9;
            f[0] = (float)xx; f[1] = (float)xy; f[2] = (float)xz; f[3] = (float)yx; f[4] = (float)yy; f[5] = (float)yz;
            f[6] = (float)zx; f[7] = (float)zy; f[8] = (float)zz;
        }
        if (a.flags) a.flags[orig] = fl;
    }
    return true;
}

__global__ void __launch_bounds__(256) shot_split_kernel(const float *__restrict__ np6, uint32_t n, float *__restrict__ xyz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyz[3 * (size_t)i] = np6[6 * (size_t)i];
    xyz[3 * (size_t)i + 1] = np6[6 * (size_t)i + 1];
    xyz[3 * (size_t)i + 2] = np6[6 * (size_t)i + 2];
}

__global__ void __launch_bounds__(256) shot_rank_kernel(const float4 *__restrict__ pts, uint32_t n, uint32_t *__restrict__ sorted_of) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) sorted_of[__float_as_uint(pts[p].w)] = p;
}

// The ball road: a wave per sorted point.  An inert point gets its zero row here; a ball of fewer than k points goes onto the fallback list
template <bool USC, bool EXT>
__global__ void __launch_bounds__(kShotWave *kShotWavesPerBlock) shot_ball_kernel(GridView gv, ShotArgs a, uint32_t n, float r2, int R, uint32_t k,
                                                                                 uint32_t *__restrict__ fb_count, uint32_t *__restrict__ fb_pos,
                                                                                 float *__restrict__ fb_xyz) {
    __shared__ float4 stage[kShotWavesPerBlock][kShotStage];
    __shared__ uint32_t hist[kShotWavesPerBlock][kShotHist];
    constexpr uint32_t DIM = USC ? TC_USC_DIM : TC_SHOT_DIM;
    const uint32_t wave = threadIdx.x / kShotWave, lane = threadIdx.x % kShotWave;
    const uint32_t p = blockIdx.x * kShotWavesPerBlock + wave;
    if (p >= n) return;                                         // the whole wave leaves
    const float4 q = gv.pts[p];
    if (p >= gv.cell_start[gv.g.ncell] || !finite_query(q.x, q.y, q.z)) {
        const size_t orig = __float_as_uint(q.w);
        for (uint32_t b = lane; b < DIM; b += kShotWave) a.out[orig * DIM + b] = 0.0f;
        if (a.lrf && lane < 9u) a.lrf[orig * 9 + lane] = 0.0f;
        if (a.flags && lane == 0u) a.flags[orig] = TC_SHOT_ROAD_INERT;
        return;
    }
    const QueryPlace pl = place_query<EXT>(gv.g, q);
    auto walk = [&](auto &&f) { shot_ball_walk<EXT>(gv, q, pl, R, r2, p, lane, f); };
    if (shot_point<USC>(a, q, a.nrm[p], TC_SHOT_ROAD_BALL, k, walk, stage[wave], hist[wave], lane)) return;
    if (lane == 0u) {                                           // features.rs:367-377
        const uint32_t s = atomicAdd(fb_count, 1u);
        fb_pos[s] = p;
        fb_xyz[3 * (size_t)s] = q.x; fb_xyz[3 * (size_t)s + 1] = q.y; fb_xyz[3 * (size_t)s + 2] = q.z;
    }
}

// The fallback road: a wave per fallback query s; its list is launch_knn's k + 1 nearest (original indices, ascending in (d2, index)),
// the query itself dropped, the first k kept
template <bool USC>
__global__ void __launch_bounds__(kShotWave *kShotWavesPerBlock) shot_fallback_kernel(ShotArgs a, uint32_t nf, const uint32_t *__restrict__ fb_pos,
                                                                                     const uint32_t *__restrict__ idx, const uint32_t *__restrict__ cnt, uint32_t k1,
                                                                                     uint32_t k, const uint32_t *__restrict__ sorted_of) {
    __shared__ float4 stage[kShotWavesPerBlock][kShotStage];
    __shared__ uint32_t hist[kShotWavesPerBlock][kShotHist];
    const uint32_t wave = threadIdx.x / kShotWave, lane = threadIdx.x % kShotWave;
    const uint32_t s = blockIdx.x * kShotWavesPerBlock + wave;
    if (s >= nf) return;
    const uint32_t p = fb_pos[s];
    const float4 q = a.pts[p];
    const uint32_t self = __float_as_uint(q.w), m = min(cnt[s], k1);
    const uint32_t *list = idx + (size_t)s * k1;
    // where the query sits in its own list (once at most: the entries are distinct indices), m if nowhere
    uint32_t self_at = m;
    for (uint32_t e = lane; e < m; e += kShotWave)
        if (list[e] == self) self_at = e;
#pragma unroll
    for (int o = 32; o; o >>= 1) self_at = min(self_at, (uint32_t)__shfl_xor((int)self_at, o));
    auto walk = [&](auto &&f) {
        for (uint32_t e0 = 0; e0 < m; e0 += kShotWave) {
            const uint32_t e = e0 + lane;
            float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint32_t j = 0;
            bool in = false;
            if (e < m && e != self_at && e - (e > self_at ? 1u : 0u) < k) {
                j = sorted_of[list[e]];
                c = a.pts[j];
                in = true;
            }
            f(in, j, c);
        }
    };
    shot_point<USC>(a, q, a.nrm[p], TC_SHOT_ROAD_FALLBACK, 0u, walk, stage[wave], hist[wave], lane);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// a validated call with n >= 1; device pointers, lrf and flags may be null
static tc_status shot_on_device(tc_context *ctx, const float *d_np6, size_t n, const tc_shot_config &cfg, float *d_out, float *d_lrf, uint32_t *d_flags) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n, k32 = (uint32_t)cfg.k_neighbors;
    const float radius = cfg.search_radius, r2 = radius * radius;      // nearest_neighbor.rs:259
    const bool finite_ball = r2 <= 3.0e38f;                             // r * r may overflow: every finite point is in every ball
    const bool usc = cfg.variant == TC_SHOT_VARIANT_USC;
    // one block of scratch, carved
    ScopedBuf arena, kidx, kdist, kcnt;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_xyz = carve(n * 3 * sizeof(float)), o_fb_xyz = carve(n * 3 * sizeof(float)), o_fb_pos = carve(n * sizeof(uint32_t)),
                 o_sorted_of = carve(n * sizeof(uint32_t)), o_count = carve(4 * sizeof(uint32_t));
    if (tc_status s = ensure(ctx, arena, off)) return s;
    char *base = (char *)arena.p;
    float *xyz = (float *)(base + o_xyz), *fb_xyz = (float *)(base + o_fb_xyz);
    uint32_t *fb_pos = (uint32_t *)(base + o_fb_pos), *sorted_of = (uint32_t *)(base + o_sorted_of), *fb_count = (uint32_t *)(base + o_count);

    DeviceIndex &ix = ctx->tgt_index;
    {
        ProfScope ps(ctx, "shot_index");
        hipLaunchKernelGGL(shot_split_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_np6, n32, xyz);
        TC_HIP_TRY(ctx, hipMemsetAsync(fb_count, 0, sizeof(uint32_t), st));
    }
    if (tc_status s = build_index(ctx, ix, xyz, n, ball_grid(radius, true))) return s;
    {
        ProfScope ps(ctx, "shot_index");
        if (tc_status s = gather_normals(ctx, ix, d_np6 + 3, 6)) return s;
        hipLaunchKernelGGL(shot_rank_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const float4 *)ix.pts.p, n32, sorted_of);
    }
    const GridView gv = view_of(ix);
    const int gmax = std::max(gv.g.gx, std::max(gv.g.gy, gv.g.gz));
    const int R = finite_ball ? ball_rings(gv.g, radius) : gmax;
    const ShotArgs a{(const float4 *)ix.pts.p, (const float4 *)ix.normals.p, radius, d_out, d_lrf, d_flags};
    const dim3 block(kShotWave * kShotWavesPerBlock);
    {
        ProfScope ps(ctx, "shot_ball");
        const dim3 grid((unsigned)((n + kShotWavesPerBlock - 1) / kShotWavesPerBlock));
        with_clamped(gv, [&](auto ext) {
            constexpr bool EXT = decltype(ext)::value;
            if (usc) hipLaunchKernelGGL((shot_ball_kernel<true, EXT>), grid, block, 0, st, gv, a, n32, r2, R, k32, fb_count, fb_pos, fb_xyz);
            else hipLaunchKernelGGL((shot_ball_kernel<false, EXT>), grid, block, 0, st, gv, a, n32, r2, R, k32, fb_count, fb_pos, fb_xyz);
        });
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    uint32_t nf = 0;
    if (k32) {                                                  // (with k = 0 no ball is too small)
        if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, fb_count, sizeof(uint32_t))) return s;     // the wait: the fallback points
        nf = pinned_host(ctx)->count;
    }
    if (!nf) return TC_OK;
    // the fallback lists: launch_knn(k + 1) in chunks of at most kShotKnnEntries entries
    const size_t k1 = cfg.k_neighbors + 1;
    const size_t chunk = std::max<size_t>(1, std::min<size_t>(nf, kShotKnnEntries / k1));
    if (tc_status s = ensure(ctx, kidx, chunk * k1 * sizeof(uint32_t))) return s;
    if (tc_status s = ensure(ctx, kdist, chunk * k1 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, kcnt, chunk * sizeof(uint32_t))) return s;
    for (size_t c0 = 0; c0 < nf; c0 += chunk) {
        const uint32_t m = (uint32_t)std::min(chunk, nf - c0);
        {
            ProfScope ps(ctx, "shot_knn_fallback");
            if (tc_status s = launch_knn(ctx, ix, fb_xyz + 3 * c0, m, k1, (uint32_t *)kidx.p, (float *)kdist.p, (uint32_t *)kcnt.p)) return s;
        }
        ProfScope ps(ctx, "shot_fallback");
        const dim3 grid((m + kShotWavesPerBlock - 1) / kShotWavesPerBlock);
        if (usc) hipLaunchKernelGGL((shot_fallback_kernel<true>), grid, block, 0, st, a, m, (const uint32_t *)fb_pos + c0, (const uint32_t *)kidx.p,
                                    (const uint32_t *)kcnt.p, (uint32_t)k1, k32, (const uint32_t *)sorted_of);
        else hipLaunchKernelGGL((shot_fallback_kernel<false>), grid, block, 0, st, a, m, (const uint32_t *)fb_pos + c0, (const uint32_t *)kidx.p,
                                (const uint32_t *)kcnt.p, (uint32_t)k1, k32, (const uint32_t *)sorted_of);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_shot.h) ----------------------------------------------------------------------------
static size_t shot_dim(int variant) { return variant == TC_SHOT_VARIANT_SHOT ? TC_SHOT_DIM : variant == TC_SHOT_VARIANT_USC ? TC_USC_DIM : 0; }

// the header's checks (1) to (5), in its order; *empty: check (4) held
static tc_status shot_check(tc_context *ctx, const float *normal_points, size_t n, const tc_shot_config *cfg, const float *out, bool *empty) {
    *empty = false;
    if (!ctx) return TC_INVALID_DATA;
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "shot: config is NULL");
    if (!normal_points && n != 0) return fail(ctx, TC_INVALID_DATA, "shot: normal_points is NULL");
    if (!out) return fail(ctx, TC_INVALID_DATA, "shot: out is NULL");
    if (!shot_dim(cfg->variant)) return fail(ctx, TC_INVALID_DATA, "shot: variant is neither SHOT (0) nor USC (1)");
    if (!(cfg->search_radius > 0.0f) || !(cfg->search_radius <= 3.0e38f)) return fail(ctx, TC_INVALID_DATA, "search_radius must be positive");
    if (n == 0) { *empty = true; return TC_OK; }
    if (n > kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "shot: n is above 2^32 - 16");
    if (cfg->k_neighbors > kMaxK - 1) return fail(ctx, TC_UNSUPPORTED, "extract_shot_features: k_neighbors > 2047 is not supported by the HIP backend");
    return TC_OK;
}

extern "C" {

void tc_shot_config_default(tc_shot_config *cfg) try {
    if (!cfg) return;
    *cfg = tc_shot_config{};
    cfg->search_radius = 0.2f;
    cfg->k_neighbors = 10;
    cfg->variant = TC_SHOT_VARIANT_SHOT;
} TC_CATCH_VOID

size_t tc_shot_dim(int variant) try {
    return shot_dim(variant);
} TC_CATCH_VALUE(0)

tc_status tc_extract_shot_features_with_normals_device(tc_context *ctx, const float *normal_points, size_t n, const tc_shot_config *cfg, float *out,
                                                       float *lrf, uint32_t *flags) try {
    bool empty;
    if (tc_status s = shot_check(ctx, normal_points, n, cfg, out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = shot_on_device(ctx, normal_points, n, *cfg, out, lrf, flags)) return s;
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
} TC_CATCH_STATUS(ctx)

tc_status tc_extract_shot_features_with_normals(tc_context *ctx, const float *normal_points, size_t n, const tc_shot_config *cfg, float *out,
                                                float *lrf, uint32_t *flags) try {
    bool empty;
    if (tc_status s = shot_check(ctx, normal_points, n, cfg, out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, normal_points, n * 6 * sizeof(float))) return s;
    // the outputs, carved from one block: the rows, the frames, the flags
    ScopedBuf res;
    const size_t dim = shot_dim(cfg->variant);
    const size_t row_bytes = (n * dim * sizeof(float) + 255) / 256 * 256, lrf_bytes = lrf ? (n * 9 * sizeof(float) + 255) / 256 * 256 : 0;
    if (tc_status s = ensure(ctx, res, row_bytes + lrf_bytes + (flags ? n * sizeof(uint32_t) : 0))) return s;
    char *base = (char *)res.p;
    float *d_lrf = lrf ? (float *)(base + row_bytes) : nullptr;
    uint32_t *d_flags = flags ? (uint32_t *)(base + row_bytes + lrf_bytes) : nullptr;
    if (tc_status s = shot_on_device(ctx, (const float *)ctx->in_a.p, n, *cfg, (float *)base, d_lrf, d_flags)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(out, base, n * dim * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (d_lrf) TC_HIP_TRY(ctx, hipMemcpyAsync(lrf, d_lrf, n * 9 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (d_flags) TC_HIP_TRY(ctx, hipMemcpyAsync(flags, d_flags, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);                                         // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

}  // extern "C"
