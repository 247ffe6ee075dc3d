// ground.hip -- ground segmentation of a LiDAR frame, Patchwork++ patches (patchwork_plus_plus / segment_ground,
// threecrate-algorithms/src/ground_segmentation.rs); the entry points of include/threecrate_hip_ground.h, which pins the arithmetic and the
// order of everything.  This unit is the whole of the companion library libthreecrate_hip_ground.so; the host layer of tc_internal.h
// (ensure, stage_in, read_back, sort_pairs, exclusive_scan_u32, compact_flagged, ProfScope) resolves from libthreecrate_hip.so.
//   ground_key        a thread per point: its patch in the high word of a 64-bit key (one past the last patch for a point out of range or not
//                     finite), its z as an order-preserving uint32 in the low word; value = the point's index; its flag word cleared
//   sort_pairs        on 32 + bits(patch count) bits: every patch one contiguous run, ascending in z (ties in input order: the sort is stable)
//   ground_starts     a thread per patch id: the lower bound of the id in the high words.  (group_by_key finds runs of WHOLE keys)
//   ground_list       a thread per patch: an empty or too small patch gets its record here; every other goes onto one of two work lists, by
//                     its count (integer atomicAdd: the order of a list plays no part in any result).  No host round trip sizes the lists:
//                     the fit launches cover the patch count and idle groups leave
//   ground_fit<wave>  THE HOT PATH.  A patch of at most 64 points has a wave, four patches to a block; a longer one a block of 256.  A patch
//                     of at most kGroundStage points is gathered through the sorted order into LDS once (float SoA) and every sweep reads
//                     it there; a longer one reads global memory again every sweep.  A sweep tests every point of the patch against the
//                     current plane and, in the same pass, sums the count and the nine raw moments of those that pass: the inliers of
//                     iteration t are the PCA input of iteration t + 1 and of the validation, so a patch costs 2 + iterations sweeps (the seed
//                     mean's, the cutoff's, one per plane) and one more over a ground patch to write its labels.  Sums: per lane in
//                     ascending position, butterfly over the wave, then the block's four waves in order through LDS.  Lane 0 solves the
//                     eigen-problem (sym3_eigen.h) and broadcasts the plane through LDS
//   ground_finish     a thread per point: the label byte and the complement flag
//   compact_flagged   twice: the ground indices, the other indices, in input order; the ground count is the first scan's total
// Atomics: integer only.  All f64; no FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS),
// and the pragma below holds even if a build drops the flag.
#include "tc_internal.h"
#include "sym3_eigen.h"
#include "../../include/threecrate_hip_ground.h"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace tc {

// Points of a patch a block keeps in LDS: 3 x 4 bytes each, 48 KiB, three blocks to a CU.  Not A/B-timed (STATE.md)
constexpr uint32_t kGroundStage = 4096;
// A patch of up to this many points is served by a wave, a longer one by a block.  Not A/B-timed (STATE.md)
constexpr uint32_t kGroundWavePatch = 64;
constexpr size_t kGroundMaxPatches = 65536;
constexpr int kMom = 10;                        // count, Sx, Sy, Sz, Sxx, Sxy, Sxz, Syy, Syz, Szz

__device__ __forceinline__ uint32_t ordered_bits(float z) {
    const uint32_t b = __float_as_uint(z);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the header's (1) for one point: its patch, or n_patches
__device__ __forceinline__ uint32_t ground_patch_of(const tc_ground_config &c, uint32_t n_patches, float x, float y, float z) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return n_patches;
    const float xx = x * x, yy = y * y;
    const float r = sqrtf(xx + yy);
    if (r > c.max_range) return n_patches;
    uint32_t base = 0;
    for (uint32_t zone = 0; zone < c.n_zones; ++zone) {
        const float r_inner = c.zone_radii[zone], r_outer = c.zone_radii[zone + 1];
        const uint32_t rings = c.num_rings[zone], sectors = c.num_sectors[zone];
        if (r >= r_inner && r < r_outer) {
            const float ring_width = (r_outer - r_inner) / (float)rings;
            const float u = (r - r_inner) / ring_width;
            const uint32_t ring = !(u >= 0.0f) ? 0u : (u < (float)rings ? min((uint32_t)u, rings - 1u) : rings - 1u);
            const float two_pi = 2.0f * 3.14159274101257324f;
            float theta = (float)atan2((double)y, (double)x);
            if (theta < 0.0f) theta += two_pi;
            const float sector_width = two_pi / (float)sectors;
            const float v = theta / sector_width;
            const uint32_t sector = !(v >= 0.0f) ? 0u : (v < (float)sectors ? min((uint32_t)v, sectors - 1u) : sectors - 1u);
            return base + ring * sectors + sector;
        }
        base += rings * sectors;
    }
    return n_patches;
}

__global__ void __launch_bounds__(256) ground_key_kernel(const float *__restrict__ xyz, uint32_t n, tc_ground_config cfg, uint32_t n_patches,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    const uint32_t p = ground_patch_of(cfg, n_patches, x, y, z);
    keys[i] = ((uint64_t)p << 32) | (uint64_t)ordered_bits(z);
    vals[i] = i;
    flag[i] = 0u;
}

// start[t], t = 0 .. n_patches: the first sorted position whose patch id is at least t (start[n_patches] = the points in range)
__global__ void __launch_bounds__(256) ground_starts_kernel(const uint64_t *__restrict__ keys_sorted, uint32_t n, uint32_t n_patches, uint32_t *__restrict__ start) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_patches) return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint32_t)(keys_sorted[mid] >> 32) < t) lo = mid + 1u; else hi = mid;
    }
    start[t] = lo;
}

__device__ __forceinline__ tc_ground_patch ground_record(uint32_t count, uint32_t status) {
    tc_ground_patch r;
    r.count = count; r.n_inliers = 0u; r.status = status;
    r.normal[0] = r.normal[1] = r.normal[2] = 0.0f;
    r.d = r.mean_z = r.flatness = 0.0f;
    return r;
}

// counters[0] = patches on the wave list, [1] = on the block list
__global__ void __launch_bounds__(256) ground_list_kernel(const uint32_t *__restrict__ start, uint32_t n_patches, uint32_t min_points, uint32_t *__restrict__ wave_list,
                                                         uint32_t *__restrict__ block_list, uint32_t *__restrict__ counters, tc_ground_patch *__restrict__ patches) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_patches) return;
    const uint32_t c = start[p + 1] - start[p];
    if (c == 0u || c < min_points) {
        if (patches) patches[p] = ground_record(c, c == 0u ? TC_GROUND_PATCH_EMPTY : TC_GROUND_PATCH_TOO_FEW_POINTS);
        return;
    }
    if (c <= kGroundWavePatch) wave_list[atomicAdd(&counters[0], 1u)] = p;          // (each list has room for every patch)
    else block_list[atomicAdd(&counters[1], 1u)] = p;
}

struct GroundFitArgs {
    const float *xyz;
    const uint32_t *order;      // the sorted values: point indices, patch by patch, ascending in z
    const uint32_t *start;      // n_patches + 1
    const uint32_t *list;       // the patches this launch serves ...
    const uint32_t *n_list;     // ... and how many they are
    uint32_t *flag;             // per point, cleared by the key pass
    tc_ground_patch *patches;   // or null
};

// The plane of a set from its moments about the pivot (the header's ARITHMETIC): out = nx, ny, nz, d' (in the pivot's frame), l0, l1, l2
__device__ inline void ground_plane_of(const double m[kMom], double out[7]) {
    const double cnt = m[0];
    const double mx = m[1] / cnt, my = m[2] / cnt, mz = m[3] / cnt;
    const double a[6] = {m[4] / cnt - mx * mx, m[5] / cnt - mx * my, m[6] / cnt - mx * mz, m[7] / cnt - my * my, m[8] / cnt - my * mz, m[9] / cnt - mz * mz};
    double w[3], v[9];
    sym3_eigen(a, w, v);
    double nx = v[0], ny = v[1], nz = v[2];
    if (nz < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
    out[0] = nx; out[1] = ny; out[2] = nz;
    out[3] = -((nx * mx + ny * my) + nz * mz);
    out[4] = w[0]; out[5] = w[1]; out[6] = w[2];
}

template <bool WAVE>
__global__ void __launch_bounds__(256) ground_fit_kernel(GroundFitArgs a, tc_ground_config cfg) {
    constexpr uint32_t T = WAVE ? 64u : 256u;                   // threads of a group
    constexpr uint32_t G = 256u / T;                            // groups of a block
    constexpr uint32_t STAGE = WAVE ? kGroundWavePatch : kGroundStage;
    __shared__ float sx[G][STAGE], sy[G][STAGE], sz[G][STAGE];
    __shared__ double red[4][kMom];                             // a block group's wave partials
    __shared__ double plane[G][8];
    const uint32_t g = threadIdx.x / T, l = threadIdx.x % T, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t item = blockIdx.x * G + g;
    if (item >= *a.n_list) return;                              // the whole group leaves (a block group: the whole block)
    auto group_sync = [&]() {
        if (WAVE) {                                             // one wave: its LDS operations are in order, nothing to wait for
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else {
            __syncthreads();
        }
    };
    const uint32_t p = a.list[item];
    const uint32_t s = a.start[p], c = a.start[p + 1] - s;
    const bool staged = c <= STAGE;
    const uint32_t i_pivot = a.order[s];
    const double px = (double)a.xyz[3 * (size_t)i_pivot], py = (double)a.xyz[3 * (size_t)i_pivot + 1], pz = (double)a.xyz[3 * (size_t)i_pivot + 2];
    if (staged) {
        for (uint32_t i = l; i < c; i += T) {
            const size_t j = a.order[s + i];
            sx[g][i] = a.xyz[3 * j]; sy[g][i] = a.xyz[3 * j + 1]; sz[g][i] = a.xyz[3 * j + 2];
        }
        group_sync();
    }
    // one sweep over the patch: the moments of the points that pass `pred(position, qx, qy, qz)`, the same in every thread of the group
    auto sweep = [&](auto pred, double m[kMom]) {
#pragma unroll
        for (int k = 0; k < kMom; ++k) m[k] = 0.0;
        for (uint32_t i = l; i < c; i += T) {
            float x, y, z;
            if (staged) { x = sx[g][i]; y = sy[g][i]; z = sz[g][i]; }
            else { const size_t j = a.order[s + i]; x = a.xyz[3 * j]; y = a.xyz[3 * j + 1]; z = a.xyz[3 * j + 2]; }
            const double qx = (double)x - px, qy = (double)y - py, qz = (double)z - pz;
            if (!pred(i, qx, qy, qz)) continue;
            m[0] += 1.0; m[1] += qx; m[2] += qy; m[3] += qz;
            m[4] += qx * qx; m[5] += qx * qy; m[6] += qx * qz; m[7] += qy * qy; m[8] += qy * qz; m[9] += qz * qz;
        }
#pragma unroll
        for (int k = 0; k < kMom; ++k) {
#pragma unroll
            for (int o = 32; o; o >>= 1) m[k] += __shfl_xor(m[k], o);
        }
        if (!WAVE) {
            if (lane == 0u) {
#pragma unroll
                for (int k = 0; k < kMom; ++k) red[wave][k] = m[k];
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kMom; ++k) m[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
            __syncthreads();                                    // the partials are free for the next sweep
        }
    };
    // lane 0 solves, everybody reads: pl = nx, ny, nz, d', l0, l1, l2
    auto solve = [&](const double m[kMom], double pl[7]) {
        if (l == 0u) {
            double out[7];
            ground_plane_of(m, out);
#pragma unroll
            for (int k = 0; k < 7; ++k) plane[g][k] = out[k];
        }
        group_sync();
#pragma unroll
        for (int k = 0; k < 7; ++k) pl[k] = plane[g][k];
        group_sync();                                           // read by all before the next solve writes
    };
    auto finish = [&](uint32_t status, uint32_t n_inliers, const double pl[7], double mean_z, double flatness) {
        if (l != 0u || !a.patches) return;
        tc_ground_patch r = ground_record(c, status);
        if (status >= TC_GROUND_PATCH_NOT_UPRIGHT) {
            r.n_inliers = n_inliers;
            r.normal[0] = (float)pl[0]; r.normal[1] = (float)pl[1]; r.normal[2] = (float)pl[2];
            r.d = (float)(pl[3] - ((pl[0] * px + pl[1] * py) + pl[2] * pz));
            r.mean_z = (float)mean_z;
            r.flatness = (float)flatness;
        }
        a.patches[p] = r;
    };
    const double none[7] = {0, 0, 0, 0, 0, 0, 0};

    // (2) the seeds: the mean of the lowest k (a prefix of the run), then everything up to the cutoff
    double cur[kMom], next[kMom], pl[7], last[7];
    const uint32_t k_seed = min(cfg.num_seed_points, c);
    sweep([&](uint32_t i, double, double, double) { return i < k_seed; }, cur);
    const double cutoff = cur[3] / (double)k_seed + (double)cfg.seed_selection_threshold;      // in the pivot's frame
    sweep([&](uint32_t, double, double, double qz) { return qz <= cutoff; }, cur);
    if (cur[0] < 3.0) { finish(TC_GROUND_PATCH_TOO_FEW_SEEDS, 0u, none, 0.0, 0.0); return; }
    if (cfg.num_iterations == 0u) { finish(TC_GROUND_PATCH_NO_ITERATION, 0u, none, 0.0, 0.0); return; }
    // (3) R-GPF
    const double dist_threshold = (double)cfg.dist_threshold;
    auto inlier = [&](uint32_t, double qx, double qy, double qz) { return fabs(((last[0] * qx + last[1] * qy) + last[2] * qz) + last[3]) <= dist_threshold; };
    for (uint32_t it = 0; it < cfg.num_iterations; ++it) {
        solve(cur, last);
        sweep(inlier, next);
        if (next[0] < 3.0) { finish(TC_GROUND_PATCH_TOO_FEW_INLIERS, 0u, none, 0.0, 0.0); return; }
        const bool stop = next[0] == cur[0];
#pragma unroll
        for (int k = 0; k < kMom; ++k) cur[k] = next[k];
        if (stop) break;
    }
    // (4) validation of `last` and its inliers `cur`
    solve(cur, pl);
    const double sum = (pl[4] + pl[5]) + pl[6];
    const double flatness = sum > 0.0 ? pl[4] / sum : 0.0;
    const double mean_z = pz + cur[3] / cur[0];
    uint32_t status = TC_GROUND_PATCH_GROUND;
    if (fabsf((float)last[2]) < cfg.uprightness_threshold) status = TC_GROUND_PATCH_NOT_UPRIGHT;
    else if (fabsf((float)mean_z + cfg.sensor_height) > cfg.elevation_threshold) status = TC_GROUND_PATCH_ELEVATION;
    else if (sum > 0.0 && (float)flatness > cfg.flatness_threshold) status = TC_GROUND_PATCH_NOT_FLAT;
    finish(status, (uint32_t)cur[0], last, mean_z, flatness);
    if (status != TC_GROUND_PATCH_GROUND) return;
    for (uint32_t i = l; i < c; i += T) {
        float x, y, z;
        if (staged) { x = sx[g][i]; y = sy[g][i]; z = sz[g][i]; }
        else { const size_t j = a.order[s + i]; x = a.xyz[3 * j]; y = a.xyz[3 * j + 1]; z = a.xyz[3 * j + 2]; }
        if (inlier(i, (double)x - px, (double)y - py, (double)z - pz)) a.flag[a.order[s + i]] = 1u;
    }
}

__global__ void __launch_bounds__(256) ground_finish_kernel(const uint32_t *__restrict__ flag, uint32_t n, uint8_t *__restrict__ labels, uint32_t *__restrict__ not_flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t f = flag[i];
    labels[i] = (uint8_t)f;
    not_flag[i] = 1u - f;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the header's checks (2) and (3); `what` = the message
static bool ground_config_ok(const tc_ground_config &c, const char *&what) {
    if (c.n_zones == 0) { what = "num_rings_per_zone must be non-empty"; return false; }
    const uint32_t nz = std::min<uint32_t>(c.n_zones, TC_GROUND_MAX_ZONES);
    for (uint32_t z = 0; z < nz; ++z)
        if (!(c.zone_radii[z] < c.zone_radii[z + 1])) { what = "zone_radii must be strictly increasing"; return false; }
    if (!(c.dist_threshold > 0.0f)) { what = "dist_threshold must be positive"; return false; }
    if (c.num_seed_points == 0) { what = "num_seed_points must be at least 1"; return false; }
    if (!(c.uprightness_threshold > 0.0f && c.uprightness_threshold <= 1.0f)) { what = "uprightness_threshold must be in (0, 1]"; return false; }
    if (c.n_zones > TC_GROUND_MAX_ZONES) { what = "ground: n_zones is above TC_GROUND_MAX_ZONES"; return false; }
    for (uint32_t z = 0; z < c.n_zones; ++z)
        if (c.num_rings[z] == 0 || c.num_sectors[z] == 0) { what = "ground: a zone has no ring or no sector"; return false; }
    return true;
}

static size_t ground_patch_count(const tc_ground_config &c) {
    size_t total = 0;
    for (uint32_t z = 0; z < c.n_zones; ++z) {
        const unsigned long long part = (unsigned long long)c.num_rings[z] * c.num_sectors[z];          // < 2^64
        total = part > SIZE_MAX - total ? SIZE_MAX : total + (size_t)part;
    }
    return total;
}

// a validated call with n >= 1; device pointers, labels never null
static tc_status ground_on_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_ground_config &cfg, size_t n_patches, uint8_t *d_labels,
                                  uint32_t *d_ground_index, uint32_t *d_nonground_index, tc_ground_patch *d_patches, size_t *n_ground) {
    hipStream_t st = ctx->stream;
    const uint32_t n32 = (uint32_t)n, P = (uint32_t)n_patches;
    // one block of scratch, carved: a call's set-up is one allocation
    ScopedBuf arena, sort_temp, blocksum;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    const size_t o_keys = carve(n * sizeof(uint64_t)), o_keys_sorted = carve(n * sizeof(uint64_t)), o_vals = carve(n * sizeof(uint32_t)),
                 o_order = carve(n * sizeof(uint32_t)), o_flag = carve(n * sizeof(uint32_t)), o_not = carve(n * sizeof(uint32_t)),
                 o_pos = carve((n + 1) * sizeof(uint32_t)), o_start = carve(((size_t)P + 1) * sizeof(uint32_t)), o_wave = carve((size_t)P * sizeof(uint32_t)),
                 o_block = carve((size_t)P * sizeof(uint32_t)), o_counters = carve(2 * sizeof(uint32_t));
    if (tc_status s = ensure(ctx, arena, off)) return s;
    char *base = (char *)arena.p;
    uint64_t *d_keys = (uint64_t *)(base + o_keys), *d_keys_sorted = (uint64_t *)(base + o_keys_sorted);
    uint32_t *d_vals = (uint32_t *)(base + o_vals), *d_order = (uint32_t *)(base + o_order), *d_flag = (uint32_t *)(base + o_flag), *d_not = (uint32_t *)(base + o_not),
             *d_pos = (uint32_t *)(base + o_pos), *d_start = (uint32_t *)(base + o_start), *d_wave = (uint32_t *)(base + o_wave), *d_block = (uint32_t *)(base + o_block),
             *d_counters = (uint32_t *)(base + o_counters);
    TC_HIP_TRY(ctx, hipMemsetAsync(d_counters, 0, 2 * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "ground_keys");
        hipLaunchKernelGGL(ground_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_xyz, n32, cfg, P, d_keys, d_vals, d_flag);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    {
        ProfScope ps(ctx, "ground_sort");
        if (tc_status s = sort_pairs(ctx, (const uint64_t *)d_keys, d_keys_sorted, (const uint32_t *)d_vals, d_order, n, 32u + bits_for_value(P), sort_temp)) return s;
    }
    {
        ProfScope ps(ctx, "ground_lists");
        hipLaunchKernelGGL(ground_starts_kernel, dim3(blocks_for((size_t)P + 1)), dim3(256), 0, st, (const uint64_t *)d_keys_sorted, n32, P, d_start);
        hipLaunchKernelGGL(ground_list_kernel, dim3(blocks_for(P)), dim3(256), 0, st, (const uint32_t *)d_start, P, cfg.min_points_per_patch, d_wave, d_block, d_counters,
                           d_patches);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    {
        ProfScope ps(ctx, "ground_fit");
        GroundFitArgs a{d_xyz, d_order, d_start, d_wave, d_counters, d_flag, d_patches};
        hipLaunchKernelGGL((ground_fit_kernel<true>), dim3((P + 3u) / 4u), dim3(256), 0, st, a, cfg);
        a.list = d_block; a.n_list = d_counters + 1;
        hipLaunchKernelGGL((ground_fit_kernel<false>), dim3(P), dim3(256), 0, st, a, cfg);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    {
        ProfScope ps(ctx, "ground_compact");
        hipLaunchKernelGGL(ground_finish_kernel, dim3(blocks_for(n)), dim3(256), 0, st, (const uint32_t *)d_flag, n32, d_labels, d_not);
        // the other indices first: the scan that stays in pos is the ground one, whose total is the count
        if (d_nonground_index)
            if (tc_status s = compact_flagged(ctx, nullptr, n32, d_not, d_pos, blocksum, nullptr, d_nonground_index)) return s;
        if (tc_status s = compact_flagged(ctx, nullptr, n32, d_flag, d_pos, blocksum, nullptr, d_ground_index)) return s;
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    GroundOut *h = &pinned_host(ctx)->ground_out;
    if (tc_status s = read_back(ctx, &h->n_ground, d_pos + n, sizeof(uint32_t))) return s;      // the wait: the ground count, behind everything else
    *n_ground = h->n_ground;
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_ground.h) --------------------------------------------------------------------------
// the header's checks (1) to (4), in its order
static tc_status ground_check(tc_context *ctx, const float *points, size_t n, const tc_ground_config *cfg, const uint8_t *out_labels, const size_t *n_ground,
                              size_t *n_patches) {
    if (!ctx) return TC_INVALID_DATA;
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "ground: config is NULL");
    if (!out_labels) return fail(ctx, TC_INVALID_DATA, "ground: out_labels is NULL");
    if (!n_ground) return fail(ctx, TC_INVALID_DATA, "ground: n_ground is NULL");
    if (!points && n != 0) return fail(ctx, TC_INVALID_DATA, "ground: points is NULL");
    const char *what = nullptr;
    if (!ground_config_ok(*cfg, what)) return fail(ctx, TC_INVALID_DATA, what);
    *n_patches = ground_patch_count(*cfg);
    if (*n_patches > kGroundMaxPatches) return fail(ctx, TC_UNSUPPORTED, "ground: more than 65536 patches");
    if (n >= kMaxPoints) return fail(ctx, TC_UNSUPPORTED, "ground: n is 2^32 - 16 or more");
    return TC_OK;
}

extern "C" {

void tc_ground_config_default(float sensor_height, tc_ground_config *cfg) try {
    if (!cfg) return;
    const float radii[5] = {0.0f, 2.7f, 12.3625f, 22.025f, 80.0f};
    const uint32_t rings[4] = {2, 4, 4, 4}, sectors[4] = {16, 32, 54, 32};
    *cfg = tc_ground_config{};
    cfg->sensor_height = sensor_height;
    cfg->n_zones = 4;
    for (int z = 0; z < 5; ++z) cfg->zone_radii[z] = radii[z];
    for (int z = 0; z < 4; ++z) { cfg->num_rings[z] = rings[z]; cfg->num_sectors[z] = sectors[z]; }
    cfg->max_range = 80.0f;
    cfg->min_points_per_patch = 10;
    cfg->num_seed_points = 20;
    cfg->seed_selection_threshold = 0.5f;
    cfg->dist_threshold = 0.125f;
    cfg->num_iterations = 3;
    cfg->uprightness_threshold = 0.707f;
    cfg->flatness_threshold = 0.05f;
    cfg->elevation_threshold = 1.0f;
} TC_CATCH_VOID

size_t tc_ground_patch_count(const tc_ground_config *cfg) try {
    const char *what = nullptr;
    if (!cfg || !ground_config_ok(*cfg, what)) return 0;
    return ground_patch_count(*cfg);
} TC_CATCH_VALUE(0)

tc_status tc_segment_ground_device(tc_context *ctx, const float *points, size_t n, const tc_ground_config *cfg, uint8_t *out_labels, uint32_t *out_ground_index,
                                   uint32_t *out_nonground_index, tc_ground_patch *out_patches, size_t *n_ground) try {
    size_t n_patches = 0;
    if (tc_status s = ground_check(ctx, points, n, cfg, out_labels, n_ground, &n_patches)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n == 0) {
        *n_ground = 0;
        if (!out_patches) return TC_OK;
        TC_HIP_TRY(ctx, hipMemsetAsync(out_patches, 0, n_patches * sizeof(tc_ground_patch), ctx->stream));       // count 0, TC_GROUND_PATCH_EMPTY
        return synced(ctx);
    }
    size_t count = 0;
    if (tc_status s = ground_on_device(ctx, points, n, *cfg, n_patches, out_labels, out_ground_index, out_nonground_index, out_patches, &count)) return s;
    *n_ground = count;
    return synced(ctx);                                         // the call's scratch is released on return: nothing may still read it
} TC_CATCH_STATUS(ctx)

tc_status tc_segment_ground(tc_context *ctx, const float *points, size_t n, const tc_ground_config *cfg, uint8_t *out_labels, uint32_t *out_ground_index,
                            uint32_t *out_nonground_index, tc_ground_patch *out_patches, size_t *n_ground) try {
    size_t n_patches = 0;
    if (tc_status s = ground_check(ctx, points, n, cfg, out_labels, n_ground, &n_patches)) return s;
    if (n == 0) {
        *n_ground = 0;
        for (size_t p = 0; out_patches && p < n_patches; ++p) out_patches[p] = tc_ground_patch{};               // count 0, TC_GROUND_PATCH_EMPTY
        return TC_OK;
    }
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, points, n * 3 * sizeof(float))) return s;
    // the outputs, carved from one block: labels, ground indices, other indices, records
    ScopedBuf out;
    const size_t idx_bytes = (n * sizeof(uint32_t) + 255) / 256 * 256, lab_bytes = (n + 255) / 256 * 256;
    const size_t o_ground = lab_bytes, o_non = o_ground + (out_ground_index ? idx_bytes : 0), o_patches = o_non + (out_nonground_index ? idx_bytes : 0);
    if (tc_status s = ensure(ctx, out, o_patches + (out_patches ? n_patches * sizeof(tc_ground_patch) : 0))) return s;
    char *base = (char *)out.p;
    uint32_t *d_ground = out_ground_index ? (uint32_t *)(base + o_ground) : nullptr, *d_non = out_nonground_index ? (uint32_t *)(base + o_non) : nullptr;
    tc_ground_patch *d_patches = out_patches ? (tc_ground_patch *)(base + o_patches) : nullptr;
    size_t count = 0;
    if (tc_status s = ground_on_device(ctx, (const float *)ctx->in_a.p, n, *cfg, n_patches, (uint8_t *)base, d_ground, d_non, d_patches, &count)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(out_labels, base, n, hipMemcpyDeviceToHost, ctx->stream));
    if (d_ground && count) TC_HIP_TRY(ctx, hipMemcpyAsync(out_ground_index, d_ground, count * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (d_non && n - count) TC_HIP_TRY(ctx, hipMemcpyAsync(out_nonground_index, d_non, (n - count) * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (d_patches) TC_HIP_TRY(ctx, hipMemcpyAsync(out_patches, d_patches, n_patches * sizeof(tc_ground_patch), hipMemcpyDeviceToHost, ctx->stream));
    if (tc_status s = synced(ctx)) return s;                     // the caller's buffers are free
    *n_ground = count;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

}  // extern "C"
