// poisson.hip -- Poisson surface reconstruction on a dense grid: an oriented cloud to an indicator field and to a welded mesh; the entry
// points of include/threecrate_hip_poisson.h, which pins the arithmetic and lists the deviation from the reference (its solver).
// This unit is the whole of the companion library libthreecrate_hip_poisson.so; the host layer of tc_internal.h (ensure, stage_in,
// read_back, group_by_key, ProfScope) resolves from libthreecrate_hip.so, tc_marching_cubes_device from libthreecrate_hip_mc.so.
//   poisson_check        one pass over the cloud: the finiteness and magnitude rules and the bounding box, block partials, one folding
//                        block                                   -- read-back 1: the flag and the box; the host makes the grid (f32) --
//   poisson_splat_key    a thread per point: its eight (node, record) pairs and their weights; group_by_key (grid.hip) sorts them stably,
//                        so a node's records stay in input order
//   poisson_splat_fold   a thread per run: f64 sums of w n and w in that order (fold_run_lane); runs above kPoissonLongRun are listed
//                                                                -- read-back 2: the number of long runs --
//   poisson_fold_long    a wave per listed run (fold_run_wave): the same bits.  Launched only when there is such a run
//   poisson_rhs          b from V by central differences, r = b, the occupied nodes, the partials of b.b; poisson_fold: bb, the state
//   the loop, four launches a round, no host wait inside a chunk of kPoissonChunk rounds (alpha, beta and the stop flag live in the
//   device's PoissonState; a round after the stop returns at once):
//     poisson_stencil    p' = r + beta p on the fly (p is double-buffered), q = A p', the partials of p'.q: four nodes of an x row per
//                        lane as one 16-byte access, the +-y and +-z rows read directly (coalesced, served by the caches)
//     poisson_fold       alpha                                     (one block)
//     poisson_update     chi += alpha p', r -= alpha q, the partials of r.r
//     poisson_fold       iterations, rel_residual, the stop flag, beta
//                                                                -- read-back per chunk: the state --
//   poisson_iso          a thread per point: its trilinear sample in f64; one wave adds them in input order (fold_run_wave)
// Inner products are f64 and deterministic: a fixed grid, every lane adds its own nodes in ascending order, a fixed tree in LDS, then
// one block folds the block partials the same way.  No floating-point atomics anywhere.
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_poisson.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// A node with more records than this is folded by a wave.  Not measured for this record (16 bytes gathered through two indices):
// mesh.hip's folds crossed between 96 and 192 items and were level up to a few hundred, and the road is meant for the thousands of records
// a dense scan puts on one node, not for the ~160 of a 4 000-point cloud on an 8^3 grid.
constexpr uint32_t kPoissonLongRun = 256;
constexpr int kPoissonLongBlocks = 1024;        // the wave-per-run kernel's grid is capped; its waves stride over the list
constexpr int kPoissonMaxBlocks = 2048;         // grid of the passes over the nodes: 8 blocks per CU, the rest by stride
constexpr int kPoissonCheckBlocks = 1024;       // grid of the pass over the points
// Rounds enqueued between two looks at the stop flag.  Not measured: a look is one stream synchronisation (~10 us), a round after the
// stop four empty launches.
constexpr uint32_t kPoissonChunk = 16;

// the device-resident state of a call, which is also what every read-back brings
struct PoissonState {
    double   bb, rr, pq, tolerance;
    float    alpha, beta, rel, iso;
    uint32_t iterations, max_iterations, occupied, n_long;
    int32_t  done;
    uint32_t bad;               // bit 0: a coordinate is not finite; bit 1: a normal fails the magnitude rule
    float    mn[3], mx[3];
};
static_assert(sizeof(PoissonState) <= sizeof(PinnedBlock::reserved), "the state is read back into the pinned block's free region");

struct PoissonGrid {
    float ox, oy, oz, h;
    uint32_t depth;             // N = 1 << depth
};

struct PoissonCell { uint32_t ix, iy, iz; float fx, fy, fz; };

// the header's step 3 for one point
__device__ __forceinline__ PoissonCell poisson_cell(const PoissonGrid &g, float px, float py, float pz) {
    const int top = (int)(1u << g.depth) - 2;
    const float gx = (px - g.ox) / g.h, gy = (py - g.oy) / g.h, gz = (pz - g.oz) / g.h;
    int ix = gx >= 0.0f ? (int)floorf(gx) : 0, iy = gy >= 0.0f ? (int)floorf(gy) : 0, iz = gz >= 0.0f ? (int)floorf(gz) : 0;
    ix = ix > top ? top : ix; iy = iy > top ? top : iy; iz = iz > top ? top : iz;
    return PoissonCell{(uint32_t)ix, (uint32_t)iy, (uint32_t)iz, gx - (float)ix, gy - (float)iy, gz - (float)iz};
}
__device__ __forceinline__ float poisson_weight(const PoissonCell &c, int corner) {
    const float wx = (corner & 1) ? c.fx : 1.0f - c.fx, wy = (corner & 2) ? c.fy : 1.0f - c.fy, wz = (corner & 4) ? c.fz : 1.0f - c.fz;
    return (wx * wy) * wz;
}
__device__ __forceinline__ uint32_t poisson_node(const PoissonCell &c, int corner, uint32_t depth) {
    const uint32_t x = c.ix + (uint32_t)(corner & 1), y = c.iy + (uint32_t)((corner >> 1) & 1), z = c.iz + (uint32_t)(corner >> 2);
    return (((z << depth) + y) << depth) + x;
}

// the sum of the block's 256 values, in a fixed tree; every thread of the block calls it
__device__ __forceinline__ double poisson_block_sum(double v, double *sh) {
    const uint32_t t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {
        if (t < s) sh[t] = sh[t] + sh[t + s];
        __syncthreads();
    }
    const double out = sh[0];
    __syncthreads();
    return out;
}
// one block: the sum of `count` partials, thread t adding t, t + 256, ... in that order, then the tree
__device__ __forceinline__ double poisson_fold_partials(const double *__restrict__ partials, uint32_t count, double *sh) {
    double acc = 0.0;
    for (uint32_t k = threadIdx.x; k < count; k += 256u) acc = acc + partials[k];
    return poisson_block_sum(acc, sh);
}

// ---- the check and the box --------------------------------------------------------------------------------------------------
// a box and the bad bits of the block's 256 threads into row 0 of sh (a fixed tree); every thread of the block calls it
__device__ __forceinline__ void poisson_box_reduce(const float mn[3], const float mx[3], uint32_t bad, float (*sh)[256]) {
    const uint32_t t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) { sh[k][t] = mn[k]; sh[3 + k][t] = mx[k]; }
    sh[6][t] = __uint_as_float(bad);
    __syncthreads();
    for (uint32_t s = 128u; s > 0u; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) { sh[k][t] = fminf(sh[k][t], sh[k][t + s]); sh[3 + k][t] = fmaxf(sh[3 + k][t], sh[3 + k][t + s]); }
            sh[6][t] = __uint_as_float(__float_as_uint(sh[6][t]) | __float_as_uint(sh[6][t + s]));
        }
        __syncthreads();
    }
}

// partial b: 8 floats: min x y z, max x y z, the bad bits, free
__global__ void __launch_bounds__(256) poisson_check_kernel(const float *__restrict__ pts, const float *__restrict__ nrm, uint32_t n, float *__restrict__ partials) {
    __shared__ float sh[7][256];
    const uint32_t t = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t bad = 0u;
    for (uint32_t i = blockIdx.x * 256u + t; i < n; i += gridDim.x * 256u) {
        const float p[3] = {pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]};
        const float x = nrm[3 * (size_t)i], y = nrm[3 * (size_t)i + 1], z = nrm[3 * (size_t)i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!(fabsf(p[k]) <= 3.4028234664e38f)) bad |= 1u;
            mn[k] = fminf(mn[k], p[k]); mx[k] = fmaxf(mx[k], p[k]);
        }
        const float mag = sqrtf((x * x + y * y) + z * z);
        if (!(mag >= 1e-6f) || !(fabsf(mag - 1.0f) <= 0.1f)) bad |= 2u;
    }
    poisson_box_reduce(mn, mx, bad, sh);
    if (t < 7u) partials[8 * (size_t)blockIdx.x + t] = sh[t][0];
}

// one block: the partials of `blocks` blocks into the state, which it also clears
__global__ void __launch_bounds__(256) poisson_check_fold_kernel(const float *__restrict__ partials, uint32_t blocks, PoissonState *__restrict__ st) {
    __shared__ float sh[7][256];
    const uint32_t t = threadIdx.x;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t bad = 0u;
    for (uint32_t b = t; b < blocks; b += 256u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { mn[k] = fminf(mn[k], partials[8 * (size_t)b + k]); mx[k] = fmaxf(mx[k], partials[8 * (size_t)b + 3 + k]); }
        bad |= __float_as_uint(partials[8 * (size_t)b + 6]);
    }
    poisson_box_reduce(mn, mx, bad, sh);
    if (t == 0u) {
        PoissonState s{};
        for (int k = 0; k < 3; ++k) { s.mn[k] = sh[k][0]; s.mx[k] = sh[3 + k][0]; }
        s.bad = __float_as_uint(sh[6][0]);
        *st = s;
    }
}

// ---- the splat ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) poisson_key_kernel(const float *__restrict__ pts, uint32_t n, PoissonGrid g, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ vals, float *__restrict__ wts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PoissonCell c = poisson_cell(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t rec = 8u * i + (uint32_t)k;              // n < 2^29
        keys[rec] = poisson_node(c, k, g.depth);
        vals[rec] = rec;
        wts[rec] = poisson_weight(c, k);
    }
}

// a record of the fold: the weight and the normal of its point
struct PoissonSum {
    double x = 0.0, y = 0.0, z = 0.0, w = 0.0;
    __device__ __forceinline__ void add(const float4 &r) {
        const double w64 = (double)r.x;
        x = x + w64 * (double)r.y; y = y + w64 * (double)r.z; z = z + w64 * (double)r.w; w = w + w64;
    }
};
struct PoissonSplat {
    const uint32_t *order;      // record numbers, run by run
    const float *wts, *nrm;
    float *vx, *vy, *vz, *w;    // N^3 each, zeroed
    __device__ __forceinline__ float4 load(uint32_t j) const {
        const uint32_t rec = order[j];
        const size_t p = rec >> 3;
        return make_float4(wts[rec], nrm[3 * p], nrm[3 * p + 1], nrm[3 * p + 2]);
    }
    __device__ __forceinline__ void store(uint32_t node, const PoissonSum &s) const {
        vx[node] = (float)s.x; vy[node] = (float)s.y; vz[node] = (float)s.z; w[node] = (float)s.w;
    }
};

__global__ void __launch_bounds__(256) poisson_splat_fold_kernel(PoissonSplat a, const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ rstart,
                                                                const uint32_t *__restrict__ n_runs, uint32_t *__restrict__ long_list, uint32_t list_cap,
                                                                uint32_t *__restrict__ n_long) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *n_runs) return;
    const uint32_t s = rstart[r], e = rstart[r + 1];
    if (e - s > kPoissonLongRun) { append_long_run(long_list, list_cap, n_long, r); return; }
    PoissonSum sum;
    fold_run_lane<4>(s, e, [&](uint32_t j) { return a.load(j); }, [&](const float4 &rec) { sum.add(rec); });
    a.store((uint32_t)keys_sorted[s], sum);                     // a key is a node number below N^3
}

__global__ void __launch_bounds__(256) poisson_fold_long_kernel(PoissonSplat a, const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ rstart,
                                                               const uint32_t *__restrict__ long_list, uint32_t n_long) {
    const uint32_t lane = threadIdx.x & 63u;
    for_each_listed_run(long_list, n_long, [&](uint32_t r) {
        const uint32_t s = rstart[r], e = rstart[r + 1];
        PoissonSum sum;                                         // every lane runs the same chain
        fold_run_wave(s, e, lane, [&](uint32_t j) { return a.load(j); }, [&](const float4 &rec) { sum.add(rec); });
        if (lane == 0u) a.store((uint32_t)keys_sorted[s], sum);
    });
}

// ---- the right-hand side ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) poisson_rhs_kernel(const float *__restrict__ vx, const float *__restrict__ vy, const float *__restrict__ vz,
                                                         const float *__restrict__ w, uint32_t depth, float h, float *__restrict__ r,
                                                         double *__restrict__ partials, PoissonState *__restrict__ st) {
    __shared__ double sh[256];
    __shared__ uint32_t occ;
    if (threadIdx.x == 0u) occ = 0u;
    __syncthreads();
    const uint32_t N = 1u << depth, total = 1u << (3u * depth), top = N - 1u;
    const float c = -0.5f * h;
    double acc = 0.0;
    uint32_t mine = 0u;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
        const uint32_t x = i & top, y = (i >> depth) & top, z = i >> (2u * depth);
        const float xm = x > 0u ? vx[i - 1u] : 0.0f, xp = x < top ? vx[i + 1u] : 0.0f;
        const float ym = y > 0u ? vy[i - N] : 0.0f, yp = y < top ? vy[i + N] : 0.0f;
        const float zm = z > 0u ? vz[i - N * N] : 0.0f, zp = z < top ? vz[i + N * N] : 0.0f;
        const float b = c * (((xp - xm) + (yp - ym)) + (zp - zm));
        r[i] = b;
        acc = acc + (double)b * (double)b;
        mine += w[i] > 0.0f ? 1u : 0u;
    }
    if (mine) atomicAdd(&occ, mine);
    const double sum = poisson_block_sum(acc, sh);              // (its barriers also order the LDS count)
    if (threadIdx.x == 0u) {
        partials[blockIdx.x] = sum;
        if (occ) atomicAdd(&st->occupied, occ);
    }
}

enum PoissonFold { POISSON_FOLD_BB, POISSON_FOLD_PQ, POISSON_FOLD_RR };

// one block between two passes: the inner product and what the loop decides from it (the header's step 6)
template <int KIND>
__global__ void __launch_bounds__(256) poisson_fold_kernel(const double *__restrict__ partials, uint32_t count, PoissonState *__restrict__ st) {
    __shared__ double sh[256];
    if (KIND != POISSON_FOLD_BB && st->done) return;
    const double sum = poisson_fold_partials(partials, count, sh);
    if (threadIdx.x != 0u) return;
    if constexpr (KIND == POISSON_FOLD_BB) {
        st->bb = sum; st->rr = sum;
        st->alpha = 0.0f; st->beta = 0.0f;
        st->iterations = 0u;
        st->rel = sum == 0.0 ? 0.0f : 1.0f;
        st->done = (sum == 0.0 || st->max_iterations == 0u) ? 1 : 0;
    } else if constexpr (KIND == POISSON_FOLD_PQ) {
        st->pq = sum;
        if (!(sum > 0.0)) { st->done = 1; return; }
        st->alpha = (float)(st->rr / sum);
    } else {
        const double rel = sqrt(sum / st->bb);
        const uint32_t it = st->iterations + 1u;
        st->iterations = it;
        st->rel = (float)rel;
        if (rel <= st->tolerance || it >= st->max_iterations) { st->done = 1; return; }
        st->beta = (float)(sum / st->rr);
        st->rr = sum;
    }
}

// ---- the loop's two passes --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 poisson_dir4(const float *__restrict__ r, const float *__restrict__ p, uint32_t i, float beta) {
    const float4 a = *reinterpret_cast<const float4 *>(r + i), b = *reinterpret_cast<const float4 *>(p + i);
    return make_float4(a.x + beta * b.x, a.y + beta * b.y, a.z + beta * b.z, a.w + beta * b.w);
}

// Lane v serves nodes 4 v .. 4 v + 3 of one x row (N >= 4 is a multiple of 4: they never straddle a row and are 16-byte aligned).
// p_old and p_new are different arrays: a neighbour's p_old may be read after its owner has stored p_new.
template <bool SCREEN>
__global__ void __launch_bounds__(256) poisson_stencil_kernel(const PoissonState *__restrict__ st, const float *__restrict__ r, const float *__restrict__ p_old,
                                                             float *__restrict__ p_new, float *__restrict__ q, const float *__restrict__ w, float point_weight,
                                                             uint32_t depth, double *__restrict__ partials) {
    __shared__ double sh[256];
    if (st->done) return;                                       // (block-uniform)
    const float beta = st->beta;
    const uint32_t N = 1u << depth, quads = 1u << (3u * depth - 2u), top = N - 1u, NN = N * N;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    double acc = 0.0;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < quads; v += gridDim.x * 256u) {
        const uint32_t i = v << 2, x = i & top, y = (i >> depth) & top, z = i >> (2u * depth);
        const float4 c = poisson_dir4(r, p_old, i, beta);
        const float4 ym = y > 0u ? poisson_dir4(r, p_old, i - N, beta) : zero, yp = y < top ? poisson_dir4(r, p_old, i + N, beta) : zero;
        const float4 zm = z > 0u ? poisson_dir4(r, p_old, i - NN, beta) : zero, zp = z < top ? poisson_dir4(r, p_old, i + NN, beta) : zero;
        const float xl = x > 0u ? r[i - 1u] + beta * p_old[i - 1u] : 0.0f;
        const float xr = x + 4u < N ? r[i + 4u] + beta * p_old[i + 4u] : 0.0f;
        float4 a;
        a.x = 6.0f * c.x - (((((xl + c.y) + ym.x) + yp.x) + zm.x) + zp.x);
        a.y = 6.0f * c.y - (((((c.x + c.z) + ym.y) + yp.y) + zm.y) + zp.y);
        a.z = 6.0f * c.z - (((((c.y + c.w) + ym.z) + yp.z) + zm.z) + zp.z);
        a.w = 6.0f * c.w - (((((c.z + xr) + ym.w) + yp.w) + zm.w) + zp.w);
        if constexpr (SCREEN) {
            const float4 ww = *reinterpret_cast<const float4 *>(w + i);
            a.x = a.x + (point_weight * ww.x) * c.x; a.y = a.y + (point_weight * ww.y) * c.y;
            a.z = a.z + (point_weight * ww.z) * c.z; a.w = a.w + (point_weight * ww.w) * c.w;
        }
        *reinterpret_cast<float4 *>(p_new + i) = c;
        *reinterpret_cast<float4 *>(q + i) = a;
        acc = acc + (double)c.x * (double)a.x; acc = acc + (double)c.y * (double)a.y;
        acc = acc + (double)c.z * (double)a.z; acc = acc + (double)c.w * (double)a.w;
    }
    const double sum = poisson_block_sum(acc, sh);
    if (threadIdx.x == 0u) partials[blockIdx.x] = sum;
}

__global__ void __launch_bounds__(256) poisson_update_kernel(const PoissonState *__restrict__ st, const float *__restrict__ p, const float *__restrict__ q,
                                                            float *__restrict__ chi, float *__restrict__ r, uint32_t depth, double *__restrict__ partials) {
    __shared__ double sh[256];
    if (st->done) return;
    const float alpha = st->alpha;
    const uint32_t quads = 1u << (3u * depth - 2u);
    double acc = 0.0;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < quads; v += gridDim.x * 256u) {
        const uint32_t i = v << 2;
        const float4 p4 = *reinterpret_cast<const float4 *>(p + i), q4 = *reinterpret_cast<const float4 *>(q + i);
        float4 c4 = *reinterpret_cast<const float4 *>(chi + i), r4 = *reinterpret_cast<const float4 *>(r + i);
        c4.x = c4.x + alpha * p4.x; c4.y = c4.y + alpha * p4.y; c4.z = c4.z + alpha * p4.z; c4.w = c4.w + alpha * p4.w;
        r4.x = r4.x - alpha * q4.x; r4.y = r4.y - alpha * q4.y; r4.z = r4.z - alpha * q4.z; r4.w = r4.w - alpha * q4.w;
        *reinterpret_cast<float4 *>(chi + i) = c4;
        *reinterpret_cast<float4 *>(r + i) = r4;
        acc = acc + (double)r4.x * (double)r4.x; acc = acc + (double)r4.y * (double)r4.y;
        acc = acc + (double)r4.z * (double)r4.z; acc = acc + (double)r4.w * (double)r4.w;
    }
    const double sum = poisson_block_sum(acc, sh);
    if (threadIdx.x == 0u) partials[blockIdx.x] = sum;
}

// ---- the iso value ----------------------------------------------------------------------------------------------------------------
struct PoissonSample { double v; };

__global__ void __launch_bounds__(256) poisson_sample_kernel(const float *__restrict__ pts, uint32_t n, PoissonGrid g, const float *__restrict__ chi,
                                                            PoissonSample *__restrict__ samples) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PoissonCell c = poisson_cell(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2]);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = s + (double)poisson_weight(c, k) * (double)chi[poisson_node(c, k, g.depth)];
    samples[i].v = s;
}

// one wave: the samples added in input order
__global__ void __launch_bounds__(64) poisson_iso_kernel(const PoissonSample *__restrict__ samples, uint32_t n, PoissonState *__restrict__ st) {
    double sum = 0.0;
    fold_run_wave(0u, n, threadIdx.x, [&](uint32_t j) { return samples[j]; }, [&](const PoissonSample &s) { sum = sum + s.v; });
    if (threadIdx.x == 0u) st->iso = (float)(sum / (double)n);
}

__global__ void __launch_bounds__(256) poisson_valid_kernel(const float *__restrict__ density, uint32_t total, float min_density, uint8_t *__restrict__ valid) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) valid[i] = density[i] >= min_density ? 1 : 0;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// the field of a call, on the device; released when the call returns
struct PoissonField {
    ScopedBuf chi, density;
    tc_mc_grid grid{};
    tc_poisson_stats stats{};
    size_t nodes = 0;
};

static PoissonState *poisson_host_state(tc_context *ctx) { return reinterpret_cast<PoissonState *>(pinned_host(ctx)->reserved); }

// a validated call (the header's checks up to the point count); device pointers
static tc_status poisson_field_on_device(tc_context *ctx, const float *d_pts, const float *d_nrm, size_t n, const tc_poisson_config &cfg, PoissonField &F) {
    hipStream_t st = ctx->stream;
    const uint32_t depth = cfg.depth, N = 1u << depth;
    const size_t nodes = (size_t)1 << (3u * depth), nk = 8 * n;
    const size_t b_node = nodes * sizeof(float);
    const unsigned node_blocks = (unsigned)std::min<size_t>(blocks_for(nodes), kPoissonMaxBlocks);
    const unsigned quad_blocks = (unsigned)std::min<size_t>(blocks_for(nodes / 4), kPoissonMaxBlocks);
    const unsigned check_blocks = (unsigned)std::min<size_t>(blocks_for(n), kPoissonCheckBlocks);
    const size_t list_cap = nk / ((size_t)kPoissonLongRun + 1) + 1;

    ScopedBuf state, partials, check_partials;
    if (tc_status s = ensure(ctx, state, sizeof(PoissonState))) return s;
    if (tc_status s = ensure(ctx, partials, (size_t)kPoissonMaxBlocks * sizeof(double))) return s;
    if (tc_status s = ensure(ctx, check_partials, (size_t)check_blocks * 8 * sizeof(float))) return s;
    PoissonState *d_state = (PoissonState *)state.p, *h = poisson_host_state(ctx);
    double *d_partials = (double *)partials.p;
    {
        ProfScope ps(ctx, "poisson_check");
        hipLaunchKernelGGL(poisson_check_kernel, dim3(check_blocks), dim3(256), 0, st, d_pts, d_nrm, (uint32_t)n, (float *)check_partials.p);
        hipLaunchKernelGGL(poisson_check_fold_kernel, dim3(1), dim3(256), 0, st, (const float *)check_partials.p, (uint32_t)check_blocks, d_state);
    }
    if (tc_status s = read_back(ctx, h, d_state, sizeof(PoissonState))) return s;
    if (h->bad & 1u) return fail(ctx, TC_INVALID_DATA, "poisson: a coordinate is not finite");
    if (h->bad & 2u) return fail(ctx, TC_INVALID_DATA, "Invalid normal: magnitude below 1e-6 or further than 0.1 from 1");

    // the header's step 2
    float ext = 0.0f, origin[3];
    for (int k = 0; k < 3; ++k) ext = std::max(ext, h->mx[k] - h->mn[k]);
    if (!(ext > 0.0f)) return fail(ctx, TC_INVALID_DATA, "poisson: the bounding box has no extent");
    const float side = cfg.scale * ext, hh = side / (float)(N - 1u);
    for (int k = 0; k < 3; ++k) { const float c = 0.5f * (h->mn[k] + h->mx[k]); origin[k] = c - 0.5f * side; }
    if (!std::isfinite(side) || !(hh > 0.0f) || !std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(ctx, TC_INVALID_DATA, "poisson: the grid of this bounding box is not finite");
    const PoissonGrid g{origin[0], origin[1], origin[2], hh, depth};

    // V (three arrays) and W; after the right-hand side the three of V serve as p | p' | q
    ScopedBuf keys, vals, wts, keys_sorted, vals_sorted, head, runpos, rstart, sort_temp, blocksum, long_list, v[3], r;
    const std::pair<ScopedBuf *, size_t> need[] = {{&keys, nk * sizeof(uint64_t)}, {&vals, nk * sizeof(uint32_t)}, {&wts, nk * sizeof(float)},
                                                   {&long_list, list_cap * sizeof(uint32_t)}, {&v[0], b_node}, {&v[1], b_node}, {&v[2], b_node},
                                                   {&r, b_node}, {&F.chi, b_node}, {&F.density, b_node}};
    for (const auto &[buf, bytes] : need) if (tc_status s = ensure(ctx, *buf, bytes)) return s;
    float *vx = (float *)v[0].p, *vy = (float *)v[1].p, *vz = (float *)v[2].p, *w = (float *)F.density.p, *chi = (float *)F.chi.p, *res = (float *)r.p;
    for (float *a : {vx, vy, vz, w, chi}) TC_HIP_TRY(ctx, hipMemsetAsync(a, 0, b_node, st));
    KeyGroups grp;
    {
        ProfScope ps(ctx, "poisson_splat_key");
        hipLaunchKernelGGL(poisson_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_pts, (uint32_t)n, g, (uint64_t *)keys.p, (uint32_t *)vals.p, (float *)wts.p);
        if (tc_status s = group_by_key(ctx, (const uint64_t *)keys.p, (const uint32_t *)vals.p, nk, 3u * depth,
                                       GroupBufs{keys_sorted, vals_sorted, head, runpos, rstart, sort_temp, blocksum}, grp)) return s;
    }
    const PoissonSplat splat{grp.order, (const float *)wts.p, d_nrm, vx, vy, vz, w};
    {
        ProfScope ps(ctx, "poisson_splat_fold");
        hipLaunchKernelGGL(poisson_splat_fold_kernel, dim3(blocks_for(nk)), dim3(256), 0, st, splat, grp.keys_sorted, grp.rstart, grp.n_runs,
                           (uint32_t *)long_list.p, (uint32_t)list_cap, &d_state->n_long);
    }
    if (tc_status s = read_back(ctx, h, d_state, sizeof(PoissonState))) return s;
    const size_t n_long = std::min<size_t>(h->n_long, list_cap);
    if (n_long) {
        ProfScope ps(ctx, "poisson_fold_long");
        const unsigned blocks = (unsigned)std::min<size_t>((n_long + 3) / 4, kPoissonLongBlocks);
        hipLaunchKernelGGL(poisson_fold_long_kernel, dim3(blocks), dim3(256), 0, st, splat, grp.keys_sorted, grp.rstart, (const uint32_t *)long_list.p,
                           (uint32_t)n_long);
    }
    // the loop's parameters go up with the state the device already holds (the box, the long-run count)
    h->max_iterations = cfg.max_iterations;
    h->tolerance = (double)cfg.tolerance;
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_state, h, sizeof(PoissonState), hipMemcpyHostToDevice, st));
    {
        ProfScope ps(ctx, "poisson_rhs");
        hipLaunchKernelGGL(poisson_rhs_kernel, dim3(node_blocks), dim3(256), 0, st, (const float *)vx, (const float *)vy, (const float *)vz, (const float *)w, depth, hh,
                           res, d_partials, d_state);
        hipLaunchKernelGGL(poisson_fold_kernel<POISSON_FOLD_BB>, dim3(1), dim3(256), 0, st, (const double *)d_partials, (uint32_t)node_blocks, d_state);
    }
    TC_HIP_TRY(ctx, hipMemsetAsync(vx, 0, b_node, st));         // p = 0 (in the stream's order: behind the right-hand side's reads of V)
    float *p[2] = {vx, vy}, *q = vz;
    const bool screen = cfg.point_weight > 0.0f;
    for (uint32_t it = 0; it < cfg.max_iterations;) {
        const uint32_t end = std::min(cfg.max_iterations, it + kPoissonChunk);
        for (; it < end; ++it) {
            float *p_old = p[it & 1u], *p_new = p[(it + 1u) & 1u];
            {
                ProfScope ps(ctx, "poisson_stencil");
                if (screen)
                    hipLaunchKernelGGL(poisson_stencil_kernel<true>, dim3(quad_blocks), dim3(256), 0, st, (const PoissonState *)d_state, (const float *)res,
                                       (const float *)p_old, p_new, q, (const float *)w, cfg.point_weight, depth, d_partials);
                else
                    hipLaunchKernelGGL(poisson_stencil_kernel<false>, dim3(quad_blocks), dim3(256), 0, st, (const PoissonState *)d_state, (const float *)res,
                                       (const float *)p_old, p_new, q, (const float *)w, cfg.point_weight, depth, d_partials);
            }
            hipLaunchKernelGGL(poisson_fold_kernel<POISSON_FOLD_PQ>, dim3(1), dim3(256), 0, st, (const double *)d_partials, (uint32_t)quad_blocks, d_state);
            {
                ProfScope ps(ctx, "poisson_update");
                hipLaunchKernelGGL(poisson_update_kernel, dim3(quad_blocks), dim3(256), 0, st, (const PoissonState *)d_state, (const float *)p_new, (const float *)q, chi,
                                   res, depth, d_partials);
            }
            hipLaunchKernelGGL(poisson_fold_kernel<POISSON_FOLD_RR>, dim3(1), dim3(256), 0, st, (const double *)d_partials, (uint32_t)quad_blocks, d_state);
        }
        if (tc_status s = read_back(ctx, h, d_state, sizeof(PoissonState))) return s;
        if (h->done) break;
    }
    {
        ProfScope ps(ctx, "poisson_iso");
        PoissonSample *samples = (PoissonSample *)keys.p;       // 8 n u64 of room; the keys are done with
        hipLaunchKernelGGL(poisson_sample_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_pts, (uint32_t)n, g, (const float *)chi, samples);
        hipLaunchKernelGGL(poisson_iso_kernel, dim3(1), dim3(64), 0, st, (const PoissonSample *)samples, (uint32_t)n, d_state);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = read_back(ctx, h, d_state, sizeof(PoissonState))) return s;       // (the call's scratch is released on return: the device is done with it)
    F.nodes = nodes;
    F.grid = tc_mc_grid{{N, N, N}, {hh, hh, hh}, {origin[0], origin[1], origin[2]}, TC_MC_X_FASTEST};
    F.stats = tc_poisson_stats{h->iterations, h->rel, h->iso, h->occupied};
    return TC_OK;
}

// field, then the welded surface; vertices / faces are device arrays (or NULL).  d_valid is scratch of the caller's scope
static tc_status poisson_surface_on_device(tc_context *ctx, const PoissonField &F, const tc_poisson_config &cfg, ScopedBuf &valid, float *d_vertices,
                                           uint32_t *d_faces, size_t vertex_capacity, size_t face_capacity, size_t *n_vertices, size_t *n_faces) {
    const uint8_t *d_valid = nullptr;
    if (cfg.min_density > 0.0f) {
        if (tc_status s = ensure(ctx, valid, F.nodes)) return s;
        hipLaunchKernelGGL(poisson_valid_kernel, dim3(blocks_for(F.nodes)), dim3(256), 0, ctx->stream, (const float *)F.density.p, (uint32_t)F.nodes, cfg.min_density,
                           (uint8_t *)valid.p);
        d_valid = (const uint8_t *)valid.p;
    }
    const tc_mc_config mc{F.stats.iso_value, TC_MC_WELD};
    return tc_marching_cubes_device(ctx, &F.grid, (const float *)F.chi.p, d_valid, &mc, d_vertices, nullptr, d_faces, vertex_capacity, face_capacity, n_vertices,
                                    n_faces);
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_poisson.h) ------------------------------------------------------------------------------
static bool poisson_nonneg(float x) { return x >= 0.0f; }      // false for a NaN

// the header's checks up to the point count, in its order; `outs`: the call's own required outputs
static tc_status poisson_check(tc_context *ctx, const char *who, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg,
                               const tc_poisson_stats *stats, std::initializer_list<const void *> outs) {
    if (!ctx) return TC_INVALID_DATA;
    if (!points) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": points is NULL");
    if (!normals) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": normals is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": config is NULL");
    if (!stats) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": stats is NULL");
    for (const void *o : outs) if (!o) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": grid, n_vertices or n_faces is NULL");
    if (n == 0) return fail(ctx, TC_INVALID_DATA, "Point cloud is empty");                                                             // poisson.rs:57-59
    if (n < TC_POISSON_MIN_POINTS) return fail(ctx, TC_INVALID_DATA, "Point cloud too small for Poisson reconstruction (minimum 10 points)");  // :62-66
    if (cfg->depth < TC_POISSON_MIN_DEPTH || cfg->depth > TC_POISSON_MAX_DEPTH) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": depth must be in 2 .. 8");
    if (!(cfg->scale >= 1.0f) || !std::isfinite(cfg->scale)) return fail(ctx, TC_INVALID_DATA, std::string(who) + ": scale must be finite and at least 1");
    if (!poisson_nonneg(cfg->point_weight) || !poisson_nonneg(cfg->tolerance) || !poisson_nonneg(cfg->min_density))
        return fail(ctx, TC_INVALID_DATA, std::string(who) + ": point_weight, tolerance and min_density must not be negative");
    if (n >= ((size_t)1 << 29)) return fail(ctx, TC_UNSUPPORTED, std::string(who) + ": 2^29 points or more");
    return TC_OK;
}

// what tc_poisson_field hands out; chi / density are the caller's arrays (device, or -- on_host -- host), each optional
static tc_status poisson_field_out(tc_context *ctx, const PoissonField &F, tc_mc_grid *grid, float *chi, float *density, tc_poisson_stats *stats, bool on_host) {
    const hipMemcpyKind kind = on_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (chi) TC_HIP_TRY(ctx, hipMemcpyAsync(chi, F.chi.p, F.nodes * sizeof(float), kind, ctx->stream));
    if (density) TC_HIP_TRY(ctx, hipMemcpyAsync(density, F.density.p, F.nodes * sizeof(float), kind, ctx->stream));
    if (tc_status s = synced(ctx)) return s;
    *grid = F.grid;
    *stats = F.stats;
    return TC_OK;
}

extern "C" {

void tc_poisson_config_default(tc_poisson_config *cfg) try {
    if (!cfg) return;
    cfg->depth = 6;
    cfg->scale = 1.1f;
    cfg->point_weight = 0.0f;
    cfg->max_iterations = 200;
    cfg->tolerance = 1e-5f;
    cfg->min_density = 0.0f;
} TC_CATCH_VOID

tc_status tc_poisson_field_device(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg, tc_mc_grid *grid,
                                  float *chi, float *density, tc_poisson_stats *stats) try {
    if (tc_status s = poisson_check(ctx, "poisson_field", points, normals, n, cfg, stats, {grid})) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    PoissonField F;
    if (tc_status s = poisson_field_on_device(ctx, points, normals, n, *cfg, F)) return s;
    return poisson_field_out(ctx, F, grid, chi, density, stats, false);
} TC_CATCH_STATUS(ctx)

tc_status tc_poisson_field(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg, tc_mc_grid *grid,
                           float *chi, float *density, tc_poisson_stats *stats) try {
    if (tc_status s = poisson_check(ctx, "poisson_field", points, normals, n, cfg, stats, {grid})) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, points, n * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, normals, n * 3 * sizeof(float))) return s;
    PoissonField F;
    if (tc_status s = poisson_field_on_device(ctx, (const float *)ctx->in_a.p, (const float *)ctx->in_b.p, n, *cfg, F)) return s;
    return poisson_field_out(ctx, F, grid, chi, density, stats, true);
} TC_CATCH_STATUS(ctx)

tc_status tc_poisson_reconstruct_device(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg,
                                        float *vertices, uint32_t *faces, size_t vertex_capacity, size_t face_capacity, size_t *n_vertices,
                                        size_t *n_faces, tc_poisson_stats *stats) try {
    if (tc_status s = poisson_check(ctx, "poisson_reconstruct", points, normals, n, cfg, stats, {n_vertices, n_faces})) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    PoissonField F;
    ScopedBuf valid;
    if (tc_status s = poisson_field_on_device(ctx, points, normals, n, *cfg, F)) return s;
    if (tc_status s = poisson_surface_on_device(ctx, F, *cfg, valid, vertices, faces, vertex_capacity, face_capacity, n_vertices, n_faces)) return s;
    if (tc_status s = synced(ctx)) return s;
    *stats = F.stats;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

tc_status tc_poisson_reconstruct(tc_context *ctx, const float *points, const float *normals, size_t n, const tc_poisson_config *cfg,
                                 float *vertices, uint32_t *faces, size_t vertex_capacity, size_t face_capacity, size_t *n_vertices, size_t *n_faces,
                                 tc_poisson_stats *stats) try {
    if (tc_status s = poisson_check(ctx, "poisson_reconstruct", points, normals, n, cfg, stats, {n_vertices, n_faces})) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, points, n * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, normals, n * 3 * sizeof(float))) return s;
    PoissonField F;
    ScopedBuf valid, d_vertices, d_faces;
    if (tc_status s = poisson_field_on_device(ctx, (const float *)ctx->in_a.p, (const float *)ctx->in_b.p, n, *cfg, F)) return s;
    size_t nv = 0, nf = 0;
    if (tc_status s = poisson_surface_on_device(ctx, F, *cfg, valid, nullptr, nullptr, 0, 0, &nv, &nf)) return s;
    *n_vertices = nv;
    *n_faces = nf;
    if (!vertices && !faces) { *stats = F.stats; return TC_OK; }
    if (vertex_capacity < nv || face_capacity < nf) return fail(ctx, TC_INVALID_DATA, "poisson_reconstruct: a capacity is smaller than its count");
    if (nv && nf) {
        if (tc_status s = ensure(ctx, d_vertices, nv * 3 * sizeof(float))) return s;
        if (tc_status s = ensure(ctx, d_faces, nf * 3 * sizeof(uint32_t))) return s;
        if (tc_status s = poisson_surface_on_device(ctx, F, *cfg, valid, (float *)d_vertices.p, (uint32_t *)d_faces.p, nv, nf, &nv, &nf)) return s;
        if (vertices) TC_HIP_TRY(ctx, hipMemcpyAsync(vertices, d_vertices.p, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        if (faces) TC_HIP_TRY(ctx, hipMemcpyAsync(faces, d_faces.p, nf * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (tc_status s = synced(ctx)) return s;
    *stats = F.stats;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

}  // extern "C"
