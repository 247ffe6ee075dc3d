// plane.hip -- RANSAC plane segmentation: segment_plane and its family (threecrate-algorithms/src/segmentation.rs:28-91, :117-180;
// the facade's deterministic sampler, threecrate-gpu/src/segmentation.rs:979-1011); the entry points of
// include/threecrate_hip_segmentation.h, which pins the arithmetic.
//   plane_model    a thread per candidate: its triple (from the caller's list, or the LCG jumped ahead to its own three draws),
//                  and the plane through it
//   plane_score    the hot path: point tiles x candidate chunks.  A lane keeps four points in registers, the block walks its chunk
//                  of candidates (wave-uniform records, scalar loads); per candidate and wave the inlier ballots are counted on
//                  the scalar side and added to an LDS counter by one lane, then one integer atomicAdd per block and candidate
//                  to the global counts.  Integer sums: the same bits on every run
//   plane_winner   one block: the greatest count, the lowest index among equals
//   flag, compact_flagged (grid.hip)   the winner's inliers in input order (skipped when the caller wants no list)
#include "tc_internal.h"
#include "../../include/threecrate_hip_segmentation.h"

#include <algorithm>
#include <cmath>

namespace tc {

constexpr int kPlaneBlock = 256;                                    // threads of a scoring block
constexpr int kPlanePerLane = 4;                                    // points a lane keeps in registers
constexpr int kPlanePointsPerBlock = kPlaneBlock * kPlanePerLane;   // 1024: the point tile
constexpr int kPlaneCandChunk = 128;                                // candidates a scoring block walks
static_assert(kPlaneCandChunk <= kPlaneBlock, "one thread flushes one counter");

// A candidate as the scoring pass reads it (24 bytes, scalar loads).  A candidate without a model is valid == 0 with the harmless
// record 0*x + 0*y + 0*z + 1, m = 1: whatever it scores, the winner pass skips it.
struct PlaneCand {
    float a, b, c, d;       // the stored coefficients
    float m;                // sqrt(a*a + b*b + c*c) of the stored coefficients (segmentation.rs:61)
    uint32_t valid;
};
static_assert(sizeof(PlaneCand) == 24, "");

// (multiplier, increment) of `steps` LCG steps at once, by repeated squaring
__device__ __forceinline__ void lcg_jump(uint64_t steps, uint64_t &mult, uint64_t &inc) {
    uint64_t cm = 6364136223846793005ull, ci = 1442695040888963407ull;
    mult = 1; inc = 0;
    for (; steps; steps >>= 1) {
        if (steps & 1) { mult *= cm; inc = inc * cm + ci; }
        ci = (cm + 1) * ci;
        cm *= cm;
    }
}
__device__ __forceinline__ uint32_t lcg_next_index(uint64_t &state, uint32_t n) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 32) % n;
}

__global__ void __launch_bounds__(256) plane_model_kernel(const float *__restrict__ xyz, uint32_t n, const uint32_t *__restrict__ samples,
                                                          uint32_t ns, uint64_t state0, PlaneCand *__restrict__ cand,
                                                          uint32_t *__restrict__ counts) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= ns) return;
    uint32_t i0, i1, i2;
    if (samples) {
        i0 = samples[3 * (size_t)it]; i1 = samples[3 * (size_t)it + 1]; i2 = samples[3 * (size_t)it + 2];
    } else {
        uint64_t mult, inc;
        lcg_jump(3ull * it, mult, inc);
        uint64_t state = state0 * mult + inc;
        i0 = lcg_next_index(state, n); i1 = lcg_next_index(state, n); i2 = lcg_next_index(state, n);
        if (i0 == i1 || i0 == i2 || i1 == i2) {                 // gpu segmentation.rs:988-998 (it < 2^20: no product wraps)
            i0 = it % n; i1 = (it * 37u + 1u) % n; i2 = (it * 101u + 2u) % n;
            while (i1 == i0) i1 = (i1 + 1u) % n;
            while (i2 == i0 || i2 == i1) i2 = (i2 + 1u) % n;
        }
    }
    counts[it] = 0u;
    PlaneCand pc = {0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 0u};
    if (i0 < n && i1 < n && i2 < n) {
        const float p0x = xyz[3 * (size_t)i0], p0y = xyz[3 * (size_t)i0 + 1], p0z = xyz[3 * (size_t)i0 + 2];
        const float v1x = xyz[3 * (size_t)i1] - p0x, v1y = xyz[3 * (size_t)i1 + 1] - p0y, v1z = xyz[3 * (size_t)i1 + 2] - p0z;
        const float v2x = xyz[3 * (size_t)i2] - p0x, v2y = xyz[3 * (size_t)i2 + 1] - p0y, v2z = xyz[3 * (size_t)i2 + 2] - p0z;
        const float cx = v1y * v2z - v1z * v2y, cy = v1z * v2x - v1x * v2z, cz = v1x * v2y - v1y * v2x;
        const float len = sqrtf(cx * cx + cy * cy + cz * cz);
        if (!(len < 1e-8f)) {                                   // :37; a NaN length keeps its (NaN) model, as in Rust: it scores 0
            pc.a = cx / len; pc.b = cy / len; pc.c = cz / len;
            pc.d = -(pc.a * p0x + pc.b * p0y + pc.c * p0z);
            pc.m = sqrtf(pc.a * pc.a + pc.b * pc.b + pc.c * pc.c);
            pc.valid = 1u;
        }
    }
    cand[it] = pc;
}

// :59-73 and `<= threshold` (:79), the division included
__device__ __forceinline__ bool plane_inlier_exact(float as, float m, float thr) {
    const float dist = (m < 1e-8f) ? INFINITY : as / m;
    return dist <= thr;
}

__global__ void __launch_bounds__(kPlaneBlock) plane_score_kernel(const float *__restrict__ xyz, uint32_t n, const PlaneCand *__restrict__ cand,
                                                                  uint32_t ns, float thr, uint32_t *__restrict__ counts) {
    __shared__ uint32_t sh[kPlaneCandChunk];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const size_t base = (size_t)blockIdx.x * kPlanePointsPerBlock;
    float x[kPlanePerLane], y[kPlanePerLane], z[kPlanePerLane];
    unsigned long long live[kPlanePerLane];                     // the lanes of this wave that hold a point: wave-uniform masks
#pragma unroll
    for (int k = 0; k < kPlanePerLane; ++k) {
        const size_t i = base + (size_t)k * kPlaneBlock + tid;
        const bool in_range = i < n;
        x[k] = in_range ? xyz[3 * i] : 0.0f; y[k] = in_range ? xyz[3 * i + 1] : 0.0f; z[k] = in_range ? xyz[3 * i + 2] : 0.0f;
        live[k] = __ballot(in_range);
    }
    if (tid < kPlaneCandChunk) sh[tid] = 0u;
    __syncthreads();
    const uint32_t c0 = blockIdx.y * kPlaneCandChunk, c1 = min(c0 + (uint32_t)kPlaneCandChunk, ns);
    for (uint32_t j = c0; j < c1; ++j) {
        const PlaneCand pc = cand[j];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < kPlanePerLane; ++k) {
            const float as = fabsf(pc.a * x[k] + pc.b * y[k] + pc.c * z[k] + pc.d);
            const unsigned long long in = __ballot(plane_inlier_exact(as, pc.m, thr));      // the division, for every point
            cnt += (uint32_t)__popcll(in & live[k]);
        }
        if (lane == 0u) atomicAdd(&sh[j - c0], cnt);             // one LDS add per wave and candidate
    }
    __syncthreads();
    if (tid < c1 - c0 && sh[tid]) atomicAdd(&counts[c0 + tid], sh[tid]);
}

__global__ void __launch_bounds__(256) plane_winner_kernel(const PlaneCand *__restrict__ cand, const uint32_t *__restrict__ counts, uint32_t ns,
                                                           PlaneOut *__restrict__ out) {
    __shared__ unsigned long long sh[256];
    unsigned long long best = 0ull;                             // count in the high word, ~index in the low: max = first of the best
    for (uint32_t j = threadIdx.x; j < ns; j += 256u) {
        const uint32_t c = counts[j];
        if (c && cand[j].valid) best = max(best, ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - j));
    }
    sh[threadIdx.x] = best;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = max(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best = sh[0];
        PlaneOut o = {{0.0f, 0.0f, 0.0f, 0.0f}, 0u, 0u, 0u, 0u};
        if (best) {
            o.index = 0xFFFFFFFFu - (uint32_t)best;
            o.count = (uint32_t)(best >> 32);
            o.found = 1u;
            const PlaneCand pc = cand[o.index];
            o.coeff[0] = pc.a; o.coeff[1] = pc.b; o.coeff[2] = pc.c; o.coeff[3] = pc.d;
        }
        *out = o;
    }
}

// the winner's inliers: the scoring pass's decision, by the division alone
__global__ void __launch_bounds__(256) plane_flag_kernel(const float *__restrict__ xyz, uint32_t n, float thr, const PlaneOut *__restrict__ win,
                                                         const PlaneCand *__restrict__ cand, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 0u;
    if (win->found) {
        const PlaneCand pc = cand[win->index];
        const float as = fabsf(pc.a * xyz[3 * (size_t)i] + pc.b * xyz[3 * (size_t)i + 1] + pc.c * xyz[3 * (size_t)i + 2] + pc.d);
        f = plane_inlier_exact(as, pc.m, thr) ? 1u : 0u;
    }
    flag[i] = f;
}

tc_status plane_segment_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, const uint32_t *d_samples, size_t n_samples,
                               uint64_t state0, float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers, uint32_t *best_iteration) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n, ns = (uint32_t)n_samples;
    // the temporaries of one call, one block: winner | candidates | counts | flags | positions (n + 1), the last two with a list only
    ScopedBuf block;
    const size_t words = ns + (d_inlier_index ? n + (n + 1) : 0);
    if (tc_status s = ensure(ctx, block, sizeof(PlaneOut) + (size_t)ns * sizeof(PlaneCand) + words * sizeof(uint32_t))) return s;
    PlaneOut *win = (PlaneOut *)block.p;
    PlaneCand *cand = (PlaneCand *)(win + 1);
    uint32_t *counts = (uint32_t *)(cand + ns), *flag = counts + ns, *pos = flag + n;
    {
        ProfScope ps(ctx, "plane_model");
        hipLaunchKernelGGL(plane_model_kernel, dim3((ns + 255u) / 256u), dim3(256), 0, st, d_xyz, n32, d_samples, ns, state0, cand, counts);
    }
    {
        ProfScope ps(ctx, "plane_score");
        const dim3 grid((unsigned)((n + kPlanePointsPerBlock - 1) / kPlanePointsPerBlock), (ns + kPlaneCandChunk - 1) / kPlaneCandChunk);
        hipLaunchKernelGGL(plane_score_kernel, grid, dim3(kPlaneBlock), 0, st, d_xyz, n32, (const PlaneCand *)cand, ns, threshold, counts);
    }
    {
        ProfScope ps(ctx, "plane_winner");
        hipLaunchKernelGGL(plane_winner_kernel, dim3(1), dim3(256), 0, st, (const PlaneCand *)cand, (const uint32_t *)counts, ns, win);
    }
    if (d_inlier_index) {
        ProfScope ps(ctx, "plane_inliers");
        const dim3 grid((unsigned)((n + 255) / 256));
        hipLaunchKernelGGL(plane_flag_kernel, grid, dim3(256), 0, st, d_xyz, n32, threshold, (const PlaneOut *)win, (const PlaneCand *)cand, flag);
        if (tc_status s = compact_flagged(ctx, d_xyz, n32, flag, pos, ctx->tgt_index.blocksum, nullptr, d_inlier_index)) return s;
    }
    PlaneOut *h = &pinned_host(ctx)->plane_out;
    if (tc_status s = read_back(ctx, h, win, sizeof(PlaneOut))) return s;           // the call's one wait
    if (!h->found) return fail(ctx, TC_ALGORITHM, "Failed to find valid plane model");
    for (int k = 0; k < 4; ++k) coefficients[k] = h->coeff[k];
    *n_inliers = h->count;
    if (best_iteration) *best_iteration = h->index;
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_segmentation.h) -------------------------------------------
// checks in the reference's order (segmentation.rs:122-136), then the limits of this implementation
static tc_status plane_validate(tc_context *ctx, size_t n, float threshold, size_t iters, float *coefficients, size_t *n_inliers) {
    if (!ctx || !coefficients || !n_inliers) return TC_INVALID_DATA;
    *n_inliers = 0;
    if (n < 3) return fail(ctx, TC_INVALID_DATA, "Need at least 3 points for plane segmentation");
    if (threshold <= 0.0f) return fail(ctx, TC_INVALID_DATA, "Threshold must be positive");
    if (iters == 0) return fail(ctx, TC_INVALID_DATA, "Max iterations must be positive");
    if (iters > TC_SEGMENT_PLANE_MAX_ITERS) return fail(ctx, TC_UNSUPPORTED, "segment_plane: more than 2^20 iterations are not supported by the HIP backend");
    return check_point_count(ctx, n);
}

// gpu segmentation.rs:980, the seed XORed in
static uint64_t plane_state0(size_t n, size_t max_iters, uint64_t seed) {
    return (((uint64_t)n << 32) ^ (uint64_t)max_iters ^ 0x9E3779B97F4A7C15ull) ^ seed;
}

// the host twins: cloud (+ samples) through in_a, the device road, the inlier list back through out_a
static tc_status plane_host(tc_context *ctx, const float *xyz, size_t n, float threshold, const uint32_t *samples, size_t n_samples, uint64_t state0,
                            float *coefficients, uint32_t *inlier_index, size_t *n_inliers, uint32_t *best_iteration) {
    const size_t xyz_bytes = n * 3 * sizeof(float), smp_bytes = samples ? n_samples * 3 * sizeof(uint32_t) : 0;
    if (tc_status s = ensure(ctx, ctx->in_a, xyz_bytes + smp_bytes)) return s;          // room for both; stage_in copies the cloud
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, xyz_bytes)) return s;
    if (inlier_index) { if (tc_status s = ensure(ctx, ctx->out_a, n * sizeof(uint32_t))) return s; }
    float *d_xyz = (float *)ctx->in_a.p;
    uint32_t *d_samples = samples ? (uint32_t *)(d_xyz + 3 * n) : nullptr;
    if (samples) TC_HIP_TRY(ctx, hipMemcpyAsync(d_samples, samples, smp_bytes, hipMemcpyHostToDevice, ctx->stream));
    uint32_t *d_index = inlier_index ? (uint32_t *)ctx->out_a.p : nullptr;
    if (tc_status s = plane_segment_device(ctx, d_xyz, n, threshold, d_samples, n_samples, state0, coefficients, d_index, n_inliers, best_iteration)) return s;
    // the list's length is known only now: its copy is the host road's second wait
    return inlier_index && *n_inliers ? stage_out(ctx, inlier_index, d_index, *n_inliers * sizeof(uint32_t)) : TC_OK;
}

extern "C" {

tc_status tc_segment_plane_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, size_t max_iters, uint64_t seed,
                                  float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers, uint32_t *best_iteration) try {
    if (tc_status s = plane_validate(ctx, n, threshold, max_iters, coefficients, n_inliers)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return plane_segment_device(ctx, d_xyz, n, threshold, nullptr, max_iters, plane_state0(n, max_iters, seed), coefficients, d_inlier_index,
                                n_inliers, best_iteration);
} TC_CATCH_STATUS(ctx)

tc_status tc_segment_plane(tc_context *ctx, const float *xyz, size_t n, float threshold, size_t max_iters, uint64_t seed,
                           float *coefficients, uint32_t *inlier_index, size_t *n_inliers, uint32_t *best_iteration) try {
    if (tc_status s = plane_validate(ctx, n, threshold, max_iters, coefficients, n_inliers)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return plane_host(ctx, xyz, n, threshold, nullptr, max_iters, plane_state0(n, max_iters, seed), coefficients, inlier_index, n_inliers,
                      best_iteration);
} TC_CATCH_STATUS(ctx)

tc_status tc_segment_plane_samples_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, const uint32_t *d_samples,
                                          size_t n_samples, float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers,
                                          uint32_t *best_iteration) try {
    if (tc_status s = plane_validate(ctx, n, threshold, n_samples, coefficients, n_inliers)) return s;
    if (!d_samples) return fail(ctx, TC_INVALID_DATA, "segment_plane_samples: samples is NULL");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return plane_segment_device(ctx, d_xyz, n, threshold, d_samples, n_samples, 0ull, coefficients, d_inlier_index, n_inliers, best_iteration);
} TC_CATCH_STATUS(ctx)

tc_status tc_segment_plane_samples(tc_context *ctx, const float *xyz, size_t n, float threshold, const uint32_t *samples,
                                   size_t n_samples, float *coefficients, uint32_t *inlier_index, size_t *n_inliers,
                                   uint32_t *best_iteration) try {
    if (tc_status s = plane_validate(ctx, n, threshold, n_samples, coefficients, n_inliers)) return s;
    if (!samples) return fail(ctx, TC_INVALID_DATA, "segment_plane_samples: samples is NULL");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return plane_host(ctx, xyz, n, threshold, samples, n_samples, 0ull, coefficients, inlier_index, n_inliers, best_iteration);
} TC_CATCH_STATUS(ctx)

}  // extern "C"
