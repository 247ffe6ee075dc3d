// ndt.hip -- NDT registration (threecrate-algorithms/src/ndt_registration.rs); the entry points of include/threecrate_hip_ndt.h, which
// pins the arithmetic and names the deviations.
//   ndt_range        the key range of the finite target points (integer min / max: the same bits on every run)
//   ndt_keys         keys relative to the range's minimum packed into 64 bits, then the stable radix sort of (key, index) (sort_pairs, grid.hip): a
//                    voxel is a run of the sorted list and keeps input order; run starts (key_runs, grid.hip), survivors -> scan -> voxel numbers
//   ndt_stats        per surviving run: mean, centred covariance + 1e-4 I, its inverse, all f64 in a fixed order; a thread per run of up
//                    to kNdtLongRun points, a block per longer run.  The 48-byte record: mean 3, inverse 6 (xx xy xz yy yz zz), count, pad
//   ndt_table        voxel number by key: a dense table over the key box (up to kNdtDenseCells cells) or an open-addressing table
//   ndt_evaluate     the hot path, one launch per iteration: a lane per source point, one record gather, 28 sums + the hit count
//                    reduced lane -> wave -> block in f64 into one row per block
//   ndt_finalize     one block, one launch per iteration: the rows folded in f64, the 6 x 6 solve, clamp, convergence, pose update
// The loop's state lives on the device; the host enqueues (evaluate, finalize) pairs in chunks of kNdtChunk and reads the state back after each.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_ndt.h"

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace tc {

constexpr uint32_t kNdtLongRun = 128;                   // runs of more points than this get a block each (tests/test_gpu_ndt.py uses the number)
constexpr uint64_t kNdtDenseCells = 1ull << 24;         // key boxes up to this many cells get the dense table (64 MiB of u32)
constexpr int kNdtBlock = 256;
constexpr int kNdtMaxRows = 1024;                       // blocks of the evaluation = rows the finalize kernel folds
constexpr int kNdtTerms = 28;                           // score, g (6), the upper triangle of H (21)
constexpr int kNdtRowStride = 32;                       // 28 sums, the hit count, 3 spare
constexpr size_t kNdtChunk = 64;                        // iterations enqueued between two reads of the state
constexpr uint32_t kNdtNone = 0xFFFFFFFFu;

struct NdtGeom {
    float    res;
    int32_t  kmin[3], kmax[3];
    int      sy, sz;            // packed key = rx << sy | ry << sz | rz (r = key - kmin)
    uint32_t gy, gz;            // dense table: cell = (rx * gy + ry) * gz + rz
    uint32_t dense;             // 1: `table` is u32 per cell; 0: NdtSlot per hash slot
    uint32_t mask;              // hash capacity - 1
};
struct alignas(16) NdtSlot { uint64_t key; uint32_t val, pad; };       // val == kNdtNone: free
struct alignas(16) NdtRecord { float mean[3], inv[6]; uint32_t count; float pad[2]; };
static_assert(sizeof(NdtRecord) == 48 && sizeof(NdtSlot) == 16, "");

// :61-67, `as i32` saturating; x finite, res finite and > 0 (x / res may overflow to +-inf)
__device__ __forceinline__ int32_t ndt_key(float x, float res) {
    const float f = floorf(x / res);
    return f >= 2147483648.0f ? INT32_MAX : (f <= -2147483648.0f ? INT32_MIN : (int32_t)f);
}
__device__ __forceinline__ bool ndt_finite3(float x, float y, float z) { return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY; }
__device__ __forceinline__ uint64_t ndt_pack(const NdtGeom &g, int32_t kx, int32_t ky, int32_t kz) {
    const uint64_t rx = (uint64_t)((int64_t)kx - g.kmin[0]), ry = (uint64_t)((int64_t)ky - g.kmin[1]), rz = (uint64_t)((int64_t)kz - g.kmin[2]);
    return (rx << g.sy) | (ry << g.sz) | rz;
}
__device__ __forceinline__ uint32_t ndt_hash(uint64_t k, uint32_t mask) {
    k ^= k >> 30; k *= 0xBF58476D1CE4E5B9ull; k ^= k >> 27; k *= 0x94D049BB133111EBull; k ^= k >> 31;
    return (uint32_t)k & mask;
}

__global__ void ndt_build_init_kernel(NdtBuildOut *bo) {
    for (int c = 0; c < 3; ++c) { bo->kmin[c] = INT32_MAX; bo->kmax[c] = INT32_MIN; }
    bo->n_finite = 0u; bo->n_runs = 0u; bo->n_voxels = 0u;
}

__global__ void __launch_bounds__(256) ndt_range_kernel(const float *__restrict__ xyz, uint32_t n, float res, NdtBuildOut *__restrict__ bo,
                                                        uint32_t *__restrict__ finite) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    bool ok = false;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        ok = ndt_finite3(x, y, z);
        finite[i] = ok ? 1u : 0u;
        if (ok) { lo[0] = hi[0] = ndt_key(x, res); lo[1] = hi[1] = ndt_key(y, res); lo[2] = hi[2] = ndt_key(z, res); }
    }
    const unsigned long long live = __ballot(ok);
    if (!live) return;                                          // wave-uniform
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], __shfl_xor(lo[c], off)); hi[c] = max(hi[c], __shfl_xor(hi[c], off)); }
    }
    if ((threadIdx.x & 63u) == 0u) {
        for (int c = 0; c < 3; ++c) { atomicMin(&bo->kmin[c], lo[c]); atomicMax(&bo->kmax[c], hi[c]); }
        atomicAdd(&bo->n_finite, (uint32_t)__popcll(live));
    }
}

// pick: the finite points' indices in input order, or null when every point is finite
__global__ void __launch_bounds__(256) ndt_key_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ pick, uint32_t nf, NdtGeom g,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nf) return;
    const uint32_t i = pick ? pick[j] : j;
    keys[j] = ndt_pack(g, ndt_key(xyz[3 * (size_t)i], g.res), ndt_key(xyz[3 * (size_t)i + 1], g.res), ndt_key(xyz[3 * (size_t)i + 2], g.res));
    idx[j] = i;
}

// a run survives with at least min_points points (:87); entries behind the last run are zero (the scan runs over n entries)
__global__ void __launch_bounds__(256) ndt_survive_kernel(uint32_t n, const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ rstart,
                                                          uint64_t min_points, uint32_t *__restrict__ keep) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    keep[r] = (r < runpos[n] && (uint64_t)(rstart[r + 1] - rstart[r]) >= min_points) ? 1u : 0u;
}

__global__ void ndt_counts_kernel(uint32_t n, const uint32_t *__restrict__ runpos, const uint32_t *__restrict__ vpos, NdtBuildOut *__restrict__ bo,
                                  uint32_t *__restrict__ long_count) {
    bo->n_runs = runpos[n]; bo->n_voxels = vpos[n];
    *long_count = 0u;
}

// cov + 1e-4 I inverted (closed form, symmetric), everything f64; the record is what the evaluation reads
__device__ __forceinline__ void ndt_store_record(NdtRecord *__restrict__ rec, const double m[3], const double c[6], uint32_t count) {
    const double inv_n = 1.0 / (double)count;
    const double xx = c[0] * inv_n + 1e-4, xy = c[1] * inv_n, xz = c[2] * inv_n, yy = c[3] * inv_n + 1e-4, yz = c[4] * inv_n, zz = c[5] * inv_n + 1e-4;
    const double a = yy * zz - yz * yz, b = xz * yz - xy * zz, d = xy * yz - xz * yy;           // first column of the adjugate
    const double inv_det = 1.0 / (xx * a + xy * b + xz * d);
    NdtRecord r;
    r.mean[0] = (float)m[0]; r.mean[1] = (float)m[1]; r.mean[2] = (float)m[2];
    r.inv[0] = (float)(a * inv_det); r.inv[1] = (float)(b * inv_det); r.inv[2] = (float)(d * inv_det);
    r.inv[3] = (float)((xx * zz - xz * xz) * inv_det); r.inv[4] = (float)((xy * xz - xx * yz) * inv_det); r.inv[5] = (float)((xx * yy - xy * xy) * inv_det);
    r.count = count; r.pad[0] = 0.0f; r.pad[1] = 0.0f;
    *rec = r;
}

// a thread per run: the survivors' keys, and the records of the short ones in sorted = input order (:93-101); the long ones are listed
__global__ void __launch_bounds__(256) ndt_stats_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ order, const uint64_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ rstart, const uint32_t *__restrict__ keep,
                                                        const uint32_t *__restrict__ vpos, uint32_t n_runs, NdtRecord *__restrict__ rec,
                                                        uint64_t *__restrict__ vkey, uint32_t *__restrict__ long_list, uint32_t list_cap,
                                                        uint32_t *__restrict__ long_count) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs || !keep[r]) return;
    const uint32_t v = vpos[r], s = rstart[r], e = rstart[r + 1];
    vkey[v] = keys[s];
    if (e - s > kNdtLongRun) { append_long_run(long_list, list_cap, long_count, r); return; }
    double sum[3] = {0.0, 0.0, 0.0};
    for (uint32_t j = s; j < e; ++j) {
        const size_t i = order[j];
        sum[0] += (double)xyz[3 * i]; sum[1] += (double)xyz[3 * i + 1]; sum[2] += (double)xyz[3 * i + 2];
    }
    const double n = (double)(e - s);
    const double m[3] = {sum[0] / n, sum[1] / n, sum[2] / n};
    double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t j = s; j < e; ++j) {
        const size_t i = order[j];
        const double dx = (double)xyz[3 * i] - m[0], dy = (double)xyz[3 * i + 1] - m[1], dz = (double)xyz[3 * i + 2] - m[2];
        c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
    }
    ndt_store_record(rec + v, m, c, e - s);
}

// the block's 256 partial sums of NV values folded by a fixed tree; every thread gets the totals
template <int NV>
__device__ __forceinline__ void ndt_block_fold(double (*sh)[6], double v[NV]) {
    const uint32_t t = threadIdx.x;
    __syncthreads();                                            // the previous fold's readers are through
#pragma unroll
    for (int k = 0; k < NV; ++k) sh[t][k] = v[k];
    __syncthreads();
    for (uint32_t s = 128; s >= 1; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < NV; ++k) sh[t][k] += sh[t + s][k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = sh[0][k];
}

// a block per listed run: thread t sums the points s + t, s + t + 256, ... in that order, then the tree: a fixed order
__global__ void __launch_bounds__(256) ndt_stats_long_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ order,
                                                             const uint32_t *__restrict__ rstart, const uint32_t *__restrict__ vpos,
                                                             const uint32_t *__restrict__ long_list, const uint32_t *__restrict__ long_count,
                                                             NdtRecord *__restrict__ rec) {
    __shared__ double sh[256][6];
    const uint32_t total = *long_count;
    for (uint32_t entry = blockIdx.x; entry < total; entry += gridDim.x) {
        const uint32_t r = long_list[entry];
        const uint32_t s = rstart[r], e = rstart[r + 1];
        double sum[3] = {0.0, 0.0, 0.0};
        for (uint32_t j = s + threadIdx.x; j < e; j += 256u) {
            const size_t i = order[j];
            sum[0] += (double)xyz[3 * i]; sum[1] += (double)xyz[3 * i + 1]; sum[2] += (double)xyz[3 * i + 2];
        }
        ndt_block_fold<3>(sh, sum);
        const double n = (double)(e - s);
        const double m[3] = {sum[0] / n, sum[1] / n, sum[2] / n};
        double c[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t j = s + threadIdx.x; j < e; j += 256u) {
            const size_t i = order[j];
            const double dx = (double)xyz[3 * i] - m[0], dy = (double)xyz[3 * i + 1] - m[1], dz = (double)xyz[3 * i + 2] - m[2];
            c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz; c[3] += dy * dy; c[4] += dy * dz; c[5] += dz * dz;
        }
        ndt_block_fold<6>(sh, c);
        if (threadIdx.x == 0) ndt_store_record(rec + vpos[r], m, c, e - s);
    }
}

__device__ __forceinline__ void ndt_unpack(const NdtGeom &g, uint64_t key, uint32_t &rx, uint32_t &ry, uint32_t &rz) {
    rz = (uint32_t)(key & ((1ull << g.sz) - 1ull));
    ry = (uint32_t)((key >> g.sz) & ((1ull << (g.sy - g.sz)) - 1ull));
    rx = (uint32_t)(key >> g.sy);
}

// a thread per voxel.  The hash table's slot is claimed on its value word (no key is kept aside as a "free" mark), then the key is written:
// nobody reads the table before the kernel has ended
__global__ void __launch_bounds__(256) ndt_table_kernel(const uint64_t *__restrict__ vkey, uint32_t nv, NdtGeom g, void *__restrict__ table) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint64_t key = vkey[v];
    if (g.dense) {
        uint32_t rx, ry, rz;
        ndt_unpack(g, key, rx, ry, rz);
        ((uint32_t *)table)[((size_t)rx * g.gy + ry) * g.gz + rz] = v;
        return;
    }
    NdtSlot *slots = (NdtSlot *)table;
    for (uint32_t h = ndt_hash(key, g.mask);; h = (h + 1u) & g.mask) {          // capacity >= 2 nv: a free slot exists
        if (atomicCAS(&slots[h].val, kNdtNone, v) == kNdtNone) { slots[h].key = key; return; }
    }
}

// voxel number of a key, kNdtNone when there is none; a key outside the box on any axis is a miss without a read
__device__ __forceinline__ uint32_t ndt_lookup(const NdtGeom &g, const void *__restrict__ table, int32_t kx, int32_t ky, int32_t kz) {
    if (kx < g.kmin[0] || kx > g.kmax[0] || ky < g.kmin[1] || ky > g.kmax[1] || kz < g.kmin[2] || kz > g.kmax[2]) return kNdtNone;
    if (g.dense) {
        const uint32_t rx = (uint32_t)((int64_t)kx - g.kmin[0]), ry = (uint32_t)((int64_t)ky - g.kmin[1]), rz = (uint32_t)((int64_t)kz - g.kmin[2]);
        return ((const uint32_t *)table)[((size_t)rx * g.gy + ry) * g.gz + rz];
    }
    const uint64_t key = ndt_pack(g, kx, ky, kz);
    const uint4 *slots = (const uint4 *)table;
    for (uint32_t h = ndt_hash(key, g.mask);; h = (h + 1u) & g.mask) {          // load factor <= 1/2: a free slot ends every probe
        const uint4 s = slots[h];                                               // key (x, y), value (z): one 16-byte read
        if (s.z == kNdtNone) return kNdtNone;
        if ((((uint64_t)s.y << 32) | s.x) == key) return s.z;
    }
}

// nalgebra's to_rotation_matrix of q = (i j k w), row-major
__device__ __forceinline__ void ndt_rotation(const float q[4], float m[9]) {
    const float i = q[0], j = q[1], k = q[2], w = q[3];
    const float ww = w * w, ii = i * i, jj = j * j, kk = k * k;
    const float ij = i * j * 2.0f, wk = w * k * 2.0f, wj = w * j * 2.0f, ik = i * k * 2.0f, jk = j * k * 2.0f, wi = w * i * 2.0f;
    m[0] = ww + ii - jj - kk; m[1] = ij - wk; m[2] = wj + ik;
    m[3] = wk + ij; m[4] = ww - ii + jj - kk; m[5] = jk - wi;
    m[6] = ik - wj; m[7] = wi + jk; m[8] = ww - ii - jj + kk;
}

struct NdtInit { float pose[7], step_size, epsilon; };
__global__ void ndt_state_init_kernel(NdtState *st, NdtInit in) {
    NdtState s = {};
    for (int c = 0; c < 4; ++c) s.q[c] = in.pose[c];
    for (int c = 0; c < 3; ++c) s.t[c] = in.pose[4 + c];
    ndt_rotation(s.q, s.rot);
    s.step_size = in.step_size; s.epsilon = in.epsilon;
    *st = s;
}

// The hot path (:117-176).  Per point: 12 bytes of source, one table word or probe, three 16-byte reads of the record.  The per-point terms
// are formed and summed in f64 (lane, then wave by shuffles, then block through LDS): a lane's f64 work is a fraction of the gather's
// latency, and neither the order of the sums nor the terms' rounding then has a say in the result's accuracy.  H = [[A, AK], [., K^T A K]] and g = [c; K^T c]
// with K = -[rs]x: no 3 x 6 Jacobian is formed.
__global__ void __launch_bounds__(kNdtBlock) ndt_evaluate_kernel(const float *__restrict__ src, uint32_t ns, const NdtState *__restrict__ st, NdtGeom g,
                                                                 const float4 *__restrict__ rec, const void *__restrict__ table,
                                                                 double *__restrict__ rows) {
    if (st->done) return;
    __shared__ double red[kNdtBlock / 64][kNdtRowStride];
    float q[4], t[3], R[9];
#pragma unroll
    for (int c = 0; c < 4; ++c) q[c] = st->q[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = st->t[c];
#pragma unroll
    for (int c = 0; c < 9; ++c) R[c] = st->rot[c];
    double acc[kNdtTerms];
#pragma unroll
    for (int k = 0; k < kNdtTerms; ++k) acc[k] = 0.0;
    uint32_t hits = 0u;
    for (size_t i = (size_t)blockIdx.x * kNdtBlock + threadIdx.x; i < ns; i += (size_t)gridDim.x * kNdtBlock) {
        const float x = src[3 * i], y = src[3 * i + 1], z = src[3 * i + 2];
        float px, py, pz;
        isometry_apply(q, t, x, y, z, px, py, pz);
        if (!ndt_finite3(px, py, pz)) continue;
        const uint32_t v = ndt_lookup(g, table, ndt_key(px, g.res), ndt_key(py, g.res), ndt_key(pz, g.res));
        if (v == kNdtNone) continue;
        const float4 r0 = rec[3 * (size_t)v], r1 = rec[3 * (size_t)v + 1], r2 = rec[3 * (size_t)v + 2];
        // the transform, rs and the record are f32 values; everything formed from them is f64.  In f32 the terms' rounding leaves g a component
        // outside the range of H (rank 3 per point), which the solve amplifies by up to 1e6 when few points hit (the 1e-6 I is all that holds it)
        const double a00 = r0.w, a01 = r1.x, a02 = r1.y, a11 = r1.z, a12 = r1.w, a22 = r2.x;
        const double rx = (R[0] * x + R[1] * y) + R[2] * z, ry = (R[3] * x + R[4] * y) + R[5] * z, rz = (R[6] * x + R[7] * y) + R[8] * z;
        const double dx = (double)px - (double)r0.x, dy = (double)py - (double)r0.y, dz = (double)pz - (double)r0.z;
        const double cx = (a00 * dx + a01 * dy) + a02 * dz, cy = (a01 * dx + a11 * dy) + a12 * dz, cz = (a02 * dx + a12 * dy) + a22 * dz;
        const double e = (double)expf((float)(-0.5 * ((dx * cx + dy * cy) + dz * cz)));
        // M = A K by rows, N = K^T M
        const double m00 = ry * a02 - rz * a01, m01 = rz * a00 - rx * a02, m02 = rx * a01 - ry * a00;
        const double m10 = ry * a12 - rz * a11, m11 = rz * a01 - rx * a12, m12 = rx * a11 - ry * a01;
        const double m20 = ry * a22 - rz * a12, m21 = rz * a02 - rx * a22, m22 = rx * a12 - ry * a02;
        const double n00 = ry * m20 - rz * m10, n01 = ry * m21 - rz * m11, n02 = ry * m22 - rz * m12;
        const double n11 = rz * m01 - rx * m21, n12 = rz * m02 - rx * m22;
        const double n22 = rx * m12 - ry * m02;
        ++hits;
        acc[0] += e;
        acc[1] += e * cx; acc[2] += e * cy; acc[3] += e * cz;
        acc[4] += e * (ry * cz - rz * cy); acc[5] += e * (rz * cx - rx * cz); acc[6] += e * (rx * cy - ry * cx);
        acc[7] += e * a00; acc[8] += e * a01; acc[9] += e * a02;
        acc[10] += e * m00; acc[11] += e * m01; acc[12] += e * m02;
        acc[13] += e * a11; acc[14] += e * a12;
        acc[15] += e * m10; acc[16] += e * m11; acc[17] += e * m12;
        acc[18] += e * a22;
        acc[19] += e * m20; acc[20] += e * m21; acc[21] += e * m22;
        acc[22] += e * n00; acc[23] += e * n01; acc[24] += e * n02;
        acc[25] += e * n11; acc[26] += e * n12;
        acc[27] += e * n22;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
        for (int k = 0; k < kNdtTerms; ++k) acc[k] += __shfl_down(acc[k], off);
        hits += __shfl_down(hits, off);
    }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < kNdtTerms; ++k) red[w][k] = acc[k];
        red[w][kNdtTerms] = (double)hits;
    }
    __syncthreads();
    if (threadIdx.x < kNdtRowStride) {
        double sum = 0.0;
        if (threadIdx.x <= kNdtTerms) {
#pragma unroll
            for (int w2 = 0; w2 < kNdtBlock / 64; ++w2) sum += red[w2][threadIdx.x];
        }
        rows[(size_t)blockIdx.x * kNdtRowStride + threadIdx.x] = sum;
    }
}

// :216-252 from the solve on.  The rows are folded in row order inside eight contiguous segments, the segments in order.
__global__ void __launch_bounds__(256) ndt_finalize_kernel(NdtState *__restrict__ st, const double *__restrict__ rows, uint32_t nrows) {
    if (st->done) return;
    __shared__ double part[8][kNdtRowStride];
    __shared__ double S[kNdtRowStride];
    __shared__ double H[6][7];                                  // the augmented system: dynamic indices stay out of scratch
    const uint32_t c = threadIdx.x & 31u, seg = threadIdx.x >> 5;
    const uint32_t per = (nrows + 7u) / 8u, r0 = seg * per, r1 = min(r0 + per, nrows);
    double sum = 0.0;
    for (uint32_t r = r0; r < r1; ++r) sum += rows[(size_t)r * kNdtRowStride + c];
    part[seg][c] = sum;
    __syncthreads();
    if (threadIdx.x < kNdtRowStride) {
        double s = 0.0;
        for (int k = 0; k < 8; ++k) s += part[k][threadIdx.x];
        S[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    st->iterations += 1u;
    st->score = (float)S[0];
    st->n_hits = (uint32_t)S[kNdtTerms];
    int k = 7;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j, ++k) { H[i][j] = S[k]; H[j][i] = S[k]; }
    for (int i = 0; i < 6; ++i) { H[i][i] += 1e-6; H[i][6] = -S[1 + i]; }
    // LU with partial pivoting on the augmented rows; a pivot that is zero or not finite: the reference's `None => break`
    for (int col = 0; col < 6; ++col) {
        int piv = col;
        double best = fabs(H[col][col]);
        for (int r = col + 1; r < 6; ++r) { const double a = fabs(H[r][col]); if (a > best) { best = a; piv = r; } }
        if (!(best > 0.0) || !(best < INFINITY)) { st->done = 1; return; }
        if (piv != col)
            for (int j = 0; j < 7; ++j) { const double tmp = H[col][j]; H[col][j] = H[piv][j]; H[piv][j] = tmp; }
        for (int r = col + 1; r < 6; ++r) {
            const double f = H[r][col] / H[col][col];
            for (int j = col; j < 7; ++j) H[r][j] -= f * H[col][j];
        }
    }
    for (int i = 5; i >= 0; --i) {
        double s = H[i][6];
        for (int j = i + 1; j < 6; ++j) s -= H[i][j] * H[j][6];
        H[i][6] = s / H[i][i];
    }
    float d0 = (float)H[0][6], d1 = (float)H[1][6], d2 = (float)H[2][6], d3 = (float)H[3][6], d4 = (float)H[4][6], d5 = (float)H[5][6];
    float norm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 + d4 * d4 + d5 * d5);
    if (norm > st->step_size) {                                 // :234-239
        const float f = st->step_size / norm;
        d0 *= f; d1 *= f; d2 *= f; d3 *= f; d4 *= f; d5 *= f;
        norm = sqrtf(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3 + d4 * d4 + d5 * d5);
    }
    if (norm < st->epsilon) { st->converged = 1; st->done = 1; return; }       // :242-245: the pose stays
    // from_euler_angles(roll = d3, pitch = d4, yaw = d5)
    float sr, cr, sp, cp, sy, cy;
    sincosf(d3 * 0.5f, &sr, &cr); sincosf(d4 * 0.5f, &sp, &cp); sincosf(d5 * 0.5f, &sy, &cy);
    const float dw = cr * cp * cy + sr * sp * sy, di = sr * cp * cy - cr * sp * sy, dj = cr * sp * cy + sr * cp * sy, dk = cr * cp * sy - sr * sp * cy;
    const float dq[4] = {di, dj, dk, dw}, zero[3] = {0.0f, 0.0f, 0.0f};
    const float qi = st->q[0], qj = st->q[1], qk = st->q[2], qw = st->q[3];
    float nt[3];
    isometry_apply(dq, zero, st->t[0], st->t[1], st->t[2], nt[0], nt[1], nt[2]);       // dq * t
    st->t[0] = d0 + nt[0]; st->t[1] = d1 + nt[1]; st->t[2] = d2 + nt[2];
    st->q[3] = dw * qw - di * qi - dj * qj - dk * qk;                                     // dq * q
    st->q[0] = dw * qi + di * qw + dj * qk - dk * qj;
    st->q[1] = dw * qj - di * qk + dj * qw + dk * qi;
    st->q[2] = dw * qk + di * qj - dj * qi + dk * qw;
    float q[4] = {st->q[0], st->q[1], st->q[2], st->q[3]}, m[9];
    ndt_rotation(q, m);
    for (int i = 0; i < 9; ++i) st->rot[i] = m[i];
}

__global__ void __launch_bounds__(256) ndt_export_kernel(const NdtRecord *__restrict__ rec, const uint64_t *__restrict__ vkey, uint32_t nv, NdtGeom g,
                                                         int32_t *__restrict__ keys, uint32_t *__restrict__ counts, float *__restrict__ mean,
                                                         float *__restrict__ inv_cov) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const NdtRecord r = rec[v];
    if (keys) {
        uint32_t rx, ry, rz;
        ndt_unpack(g, vkey[v], rx, ry, rz);
        keys[3 * (size_t)v] = (int32_t)((int64_t)g.kmin[0] + rx); keys[3 * (size_t)v + 1] = (int32_t)((int64_t)g.kmin[1] + ry);
        keys[3 * (size_t)v + 2] = (int32_t)((int64_t)g.kmin[2] + rz);
    }
    if (counts) counts[v] = r.count;
    if (mean) for (int c = 0; c < 3; ++c) mean[3 * (size_t)v + c] = r.mean[c];
    if (inv_cov) for (int c = 0; c < 6; ++c) inv_cov[6 * (size_t)v + c] = r.inv[c];
}

// ---- host side ------------------------------------------------------------------------------------------------
// the voxel map of one call: every block is a temporary of that call
struct NdtMap {
    NdtGeom g{};
    size_t n_voxels = 0;
    ScopedBuf rec, vkey, table;
};

// a validated call: resolution finite and > 0, nt < kMaxPoints.  n_voxels == 0: no voxel survives (nothing else of the map is set)
static tc_status ndt_build_device(tc_context *ctx, const float *d_target, size_t nt, float resolution, size_t min_points, NdtMap &map) {
    hipStream_t st = ctx->stream;
    map.n_voxels = 0;
    if (nt == 0) return TC_OK;
    const uint32_t n32 = (uint32_t)nt;
    const unsigned nb = (unsigned)((nt + 255) / 256);
    NdtBuildOut *h = &pinned_host(ctx)->ndt_build;
    // one block of words: build record | finite flags, then heads (n) | positions (n + 1) | run positions (n + 1) | run starts (n + 1) |
    // keep (n) | voxel positions (n + 1) | picked / sorted indices (n) | indices (n) | long-run list (n / kNdtLongRun + 1) | long-run count
    ScopedBuf words, keys2, sort_tmp, blocksum;
    const size_t nw = 16 + nt + (nt + 1) * 4 + nt * 3 + nt / kNdtLongRun + 2;
    if (tc_status s = ensure(ctx, words, nw * sizeof(uint32_t))) return s;
    NdtBuildOut *bo = (NdtBuildOut *)words.p;
    uint32_t *flag = (uint32_t *)words.p + 16, *pos = flag + nt, *runpos = pos + nt + 1, *rstart = runpos + nt + 1, *keep = rstart + nt + 1,
             *vpos = keep + nt, *order = vpos + nt + 1, *idx = order + nt, *long_list = idx + nt, *long_count = long_list + nt / kNdtLongRun + 1;
    NdtGeom &g = map.g;
    g = NdtGeom{};
    g.res = resolution;
    {
        ProfScope ps(ctx, "ndt_voxel_keys");
        hipLaunchKernelGGL(ndt_build_init_kernel, dim3(1), dim3(1), 0, st, bo);
        hipLaunchKernelGGL(ndt_range_kernel, dim3(nb), dim3(256), 0, st, d_target, n32, resolution, bo, flag);
    }
    if (tc_status s = read_back(ctx, h, bo, sizeof(NdtBuildOut))) return s;
    const size_t nf = h->n_finite;
    if (nf == 0) return TC_OK;
    uint64_t dims[3];
    int bits[3];
    for (int c = 0; c < 3; ++c) {
        g.kmin[c] = h->kmin[c]; g.kmax[c] = h->kmax[c];
        dims[c] = (uint64_t)((int64_t)h->kmax[c] - (int64_t)h->kmin[c] + 1);
        bits[c] = (int)bits_for_value(dims[c] - 1);
    }
    const int total_bits = bits[0] + bits[1] + bits[2];
    if (total_bits > 64) return fail(ctx, TC_UNSUPPORTED, "ndt: the target's voxel key box needs more than 64 bits");
    g.sz = bits[2]; g.sy = bits[1] + bits[2];
    const uint32_t nf32 = (uint32_t)nf;
    const unsigned nfb = (unsigned)((nf + 255) / 256);
    if (tc_status s = ensure(ctx, keys2, 2 * nf * sizeof(uint64_t))) return s;
    uint64_t *keys = (uint64_t *)keys2.p, *keys_sorted = keys + nf;
    const uint32_t *pick = nullptr;
    if (nf < nt) {                                              // the finite points' indices, in input order
        if (tc_status s = compact_flagged(ctx, d_target, n32, flag, pos, blocksum, nullptr, order)) return s;
        pick = order;
    }
    {
        ProfScope ps(ctx, "ndt_voxel_keys");
        hipLaunchKernelGGL(ndt_key_kernel, dim3(nfb), dim3(256), 0, st, d_target, pick, nf32, g, keys, idx);
    }
    if (tc_status s = sort_pairs(ctx, keys, keys_sorted, idx, order, nf, (unsigned)total_bits, sort_tmp)) return s;
    uint32_t *head = flag;                                      // the finite flags are no longer needed
    if (tc_status s = key_runs(ctx, keys_sorted, nf32, head, runpos, rstart, blocksum)) return s;
    hipLaunchKernelGGL(ndt_survive_kernel, dim3(nfb), dim3(256), 0, st, nf32, (const uint32_t *)runpos, (const uint32_t *)rstart, (uint64_t)min_points, keep);
    if (tc_status s = exclusive_scan_u32(ctx, keep, nf32, vpos, blocksum)) return s;
    hipLaunchKernelGGL(ndt_counts_kernel, dim3(1), dim3(1), 0, st, nf32, (const uint32_t *)runpos, (const uint32_t *)vpos, bo, long_count);
    if (tc_status s = read_back(ctx, h, bo, sizeof(NdtBuildOut))) return s;
    const size_t n_runs = h->n_runs, nv = h->n_voxels;
    if (nv == 0) return TC_OK;
    if (tc_status s = ensure(ctx, map.rec, nv * sizeof(NdtRecord))) return s;
    if (tc_status s = ensure(ctx, map.vkey, nv * sizeof(uint64_t))) return s;
    {
        ProfScope ps(ctx, "ndt_voxel_stats");
        hipLaunchKernelGGL(ndt_stats_kernel, dim3((unsigned)((n_runs + 255) / 256)), dim3(256), 0, st, d_target, (const uint32_t *)order,
                           (const uint64_t *)keys_sorted, (const uint32_t *)rstart, (const uint32_t *)keep, (const uint32_t *)vpos, (uint32_t)n_runs,
                           (NdtRecord *)map.rec.p, (uint64_t *)map.vkey.p, long_list, (uint32_t)(nt / kNdtLongRun + 1), long_count);
        const unsigned nlong = (unsigned)std::min<size_t>(nf / kNdtLongRun + 1, 1024);
        hipLaunchKernelGGL(ndt_stats_long_kernel, dim3(nlong), dim3(256), 0, st, d_target, (const uint32_t *)order, (const uint32_t *)rstart,
                           (const uint32_t *)vpos, (const uint32_t *)long_list, (const uint32_t *)long_count, (NdtRecord *)map.rec.p);
    }
    // cells of the key box: at most 2^24 only when every axis is below 2^24, so the product of three such fits 2^72 -> compare in double
    const double cells = (double)dims[0] * (double)dims[1] * (double)dims[2];
    size_t table_bytes;
    if (cells <= (double)kNdtDenseCells) {
        g.dense = 1u; g.gy = (uint32_t)dims[1]; g.gz = (uint32_t)dims[2];
        table_bytes = (size_t)cells * sizeof(uint32_t);
    } else {
        size_t cap = 2;
        while (cap < 2 * nv) cap <<= 1;
        g.dense = 0u; g.mask = (uint32_t)(cap - 1);
        table_bytes = cap * sizeof(NdtSlot);
    }
    if (tc_status s = ensure(ctx, map.table, table_bytes)) return s;
    {
        ProfScope ps(ctx, "ndt_table");
        TC_HIP_TRY(ctx, hipMemsetAsync(map.table.p, 0xFF, table_bytes, st));
        hipLaunchKernelGGL(ndt_table_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, (const uint64_t *)map.vkey.p, (uint32_t)nv, g, map.table.p);
    }
    // the scratch of this function is released when it returns: the stream must be through with it
    if (tc_status s = synced(ctx)) return s;
    TC_HIP_TRY(ctx, hipGetLastError());
    map.n_voxels = nv;
    return TC_OK;
}

static tc_status ndt_register_device(tc_context *ctx, const float *d_source, size_t ns, const float *d_target, size_t nt, const float *init,
                                     const tc_ndt_config *cfg, tc_ndt_result *result) {
    hipStream_t st = ctx->stream;
    NdtMap map;
    if (tc_status s = ndt_build_device(ctx, d_target, nt, cfg->resolution, cfg->min_points_per_voxel, map)) return s;
    if (map.n_voxels == 0) return fail(ctx, TC_ALGORITHM, "NDT voxel grid is empty — try a larger resolution or lower min_points_per_voxel");
    const unsigned nrows = (unsigned)std::min<size_t>((ns + kNdtBlock - 1) / kNdtBlock, kNdtMaxRows);
    ScopedBuf block;                                            // state | rows
    if (tc_status s = ensure(ctx, block, 128 + (size_t)nrows * kNdtRowStride * sizeof(double))) return s;
    NdtState *state = (NdtState *)block.p;
    double *rows = (double *)((char *)block.p + 128);
    NdtInit in;
    for (int c = 0; c < 7; ++c) in.pose[c] = init ? init[c] : (c == 3 ? 1.0f : 0.0f);
    in.step_size = cfg->step_size; in.epsilon = cfg->epsilon;
    hipLaunchKernelGGL(ndt_state_init_kernel, dim3(1), dim3(1), 0, st, state, in);
    NdtState *h = &pinned_host(ctx)->ndt_state;
    size_t enqueued = 0;
    do {                                                        // no host round trip per iteration: one read per chunk
        const size_t chunk = std::min(kNdtChunk, cfg->max_iterations - enqueued);
        for (size_t k = 0; k < chunk; ++k) {
            {
                ProfScope ps(ctx, "ndt_evaluate");
                hipLaunchKernelGGL(ndt_evaluate_kernel, dim3(nrows), dim3(kNdtBlock), 0, st, d_source, (uint32_t)ns, (const NdtState *)state, map.g,
                                   (const float4 *)map.rec.p, (const void *)map.table.p, rows);
            }
            {
                ProfScope ps(ctx, "ndt_finalize");
                hipLaunchKernelGGL(ndt_finalize_kernel, dim3(1), dim3(256), 0, st, state, (const double *)rows, (uint32_t)nrows);
            }
        }
        enqueued += chunk;
        if (tc_status s = read_back(ctx, h, state, sizeof(NdtState))) return s;
    } while (!h->done && enqueued < cfg->max_iterations);
    for (int c = 0; c < 4; ++c) result->transformation[c] = h->q[c];
    for (int c = 0; c < 3; ++c) result->transformation[4 + c] = h->t[c];
    result->score = h->score;
    result->iterations = h->iterations;
    result->converged = h->converged;
    result->n_voxels = map.n_voxels;
    result->n_hits = h->n_hits;
    return TC_OK;
}

// the map into the caller's device arrays (each optional)
static tc_status ndt_voxels_device(tc_context *ctx, const float *d_target, size_t nt, float resolution, size_t min_points, int32_t *d_keys,
                                   uint32_t *d_counts, float *d_mean, float *d_inv_cov, size_t capacity, size_t *n_voxels) {
    NdtMap map;
    if (tc_status s = ndt_build_device(ctx, d_target, nt, resolution, min_points, map)) return s;
    *n_voxels = map.n_voxels;
    if (map.n_voxels == 0) return TC_OK;
    if (capacity < map.n_voxels) return fail(ctx, TC_INVALID_DATA, "ndt_voxels: capacity is smaller than the number of voxels");
    if (d_keys || d_counts || d_mean || d_inv_cov)
        hipLaunchKernelGGL(ndt_export_kernel, dim3((unsigned)((map.n_voxels + 255) / 256)), dim3(256), 0, ctx->stream, (const NdtRecord *)map.rec.p,
                           (const uint64_t *)map.vkey.p, (uint32_t)map.n_voxels, map.g, d_keys, d_counts, d_mean, d_inv_cov);
    return synced(ctx);                                         // the map is released on return
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_ndt.h) ------------------------------------------------------------
static tc_status ndt_check_resolution(tc_context *ctx, float resolution) {
    return (std::isfinite(resolution) && resolution > 0.0f) ? TC_OK : fail(ctx, TC_INVALID_DATA, "Resolution must be positive and finite");
}

// NULL checks, the resolution, then the reference's checks in its order (:194-201); the third (:204-209) follows the build
static tc_status ndt_validate(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt, const tc_ndt_config *cfg,
                              tc_ndt_result *result) {
    if (!ctx || !result) return TC_INVALID_DATA;
    result->iterations = 0;
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "ndt_registration: config is NULL");
    if ((!source && ns) || (!target && nt)) return fail(ctx, TC_INVALID_DATA, "ndt_registration: a point cloud is NULL");
    if (tc_status s = ndt_check_resolution(ctx, cfg->resolution)) return s;
    if (ns == 0) return fail(ctx, TC_ALGORITHM, "Source point cloud is empty");
    if (nt < cfg->min_points_per_voxel) return fail(ctx, TC_ALGORITHM, "Target point cloud has too few points for NDT voxel grid");
    return check_point_count(ctx, ns, nt);
}

static tc_status ndt_voxels_validate(tc_context *ctx, const float *target, size_t nt, float resolution, size_t *n_voxels) {
    if (!ctx || !n_voxels) return TC_INVALID_DATA;
    *n_voxels = 0;
    if (!target && nt) return fail(ctx, TC_INVALID_DATA, "ndt_voxels: target is NULL");
    if (tc_status s = ndt_check_resolution(ctx, resolution)) return s;
    return check_point_count(ctx, nt);
}

extern "C" {

tc_status tc_ndt_registration_device(tc_context *ctx, const float *d_source, size_t ns, const float *d_target, size_t nt, const float *init,
                                     const tc_ndt_config *cfg, tc_ndt_result *result) try {
    if (tc_status s = ndt_validate(ctx, d_source, ns, d_target, nt, cfg, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ndt_register_device(ctx, d_source, ns, d_target, nt, init, cfg, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_ndt_registration(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt, const float *init,
                              const tc_ndt_config *cfg, tc_ndt_result *result) try {
    if (tc_status s = ndt_validate(ctx, source, ns, target, nt, cfg, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, source, ns * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, target, nt * 3 * sizeof(float))) return s;
    // (the result is a host record filled after the road's last read of the state: nothing is left to copy out)
    return ndt_register_device(ctx, (const float *)ctx->in_a.p, ns, (const float *)ctx->in_b.p, nt, init, cfg, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_ndt_voxels_device(tc_context *ctx, const float *d_target, size_t nt, float resolution, size_t min_points_per_voxel, int32_t *d_keys,
                               uint32_t *d_counts, float *d_mean, float *d_inv_cov, size_t capacity, size_t *n_voxels) try {
    if (tc_status s = ndt_voxels_validate(ctx, d_target, nt, resolution, n_voxels)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ndt_voxels_device(ctx, d_target, nt, resolution, min_points_per_voxel, d_keys, d_counts, d_mean, d_inv_cov, capacity, n_voxels);
} TC_CATCH_STATUS(ctx)

tc_status tc_ndt_voxels(tc_context *ctx, const float *target, size_t nt, float resolution, size_t min_points_per_voxel, int32_t *keys,
                        uint32_t *counts, float *mean, float *inv_cov, size_t capacity, size_t *n_voxels) try {
    if (tc_status s = ndt_voxels_validate(ctx, target, nt, resolution, n_voxels)) return s;
    if (nt == 0) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, target, nt * 3 * sizeof(float))) return s;
    // room for min(capacity, nt) rows of every array the caller wants: keys | counts | mean | inv_cov
    const size_t rows = std::min(capacity, nt);
    if (tc_status s = ensure(ctx, ctx->out_a, rows * 13 * sizeof(uint32_t) + 256)) return s;
    int32_t *d_keys = (int32_t *)ctx->out_a.p;
    uint32_t *d_counts = (uint32_t *)(d_keys + 3 * rows);
    float *d_mean = (float *)(d_counts + rows), *d_inv = d_mean + 3 * rows;
    if (tc_status s = ndt_voxels_device(ctx, (const float *)ctx->in_a.p, nt, resolution, min_points_per_voxel, keys ? d_keys : nullptr,
                                        counts ? d_counts : nullptr, mean ? d_mean : nullptr, inv_cov ? d_inv : nullptr, capacity, n_voxels)) return s;
    const size_t v = *n_voxels;
    if (v == 0) return TC_OK;
    if (keys) TC_HIP_TRY(ctx, hipMemcpyAsync(keys, d_keys, v * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (counts) TC_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, v * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (mean) TC_HIP_TRY(ctx, hipMemcpyAsync(mean, d_mean, v * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (inv_cov) TC_HIP_TRY(ctx, hipMemcpyAsync(inv_cov, d_inv, v * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

}  // extern "C"
