// global.hip -- the two device steps of global registration (threecrate-algorithms/src/global_registration.rs): descriptor matching
// (find_feature_correspondences, :85-110) and RANSAC over the correspondences (:252-299 with estimate_transform_svd :112-145 and
// count_inliers :147-163); the entry points of include/threecrate_hip_global.h, which pins the arithmetic.  This unit is the whole of the
// companion library libthreecrate_hip_global.so; the host layer of tc_internal.h resolves from libthreecrate_hip.so.
//   match           a lane owns one source descriptor (33 registers), the block stages a tile of target descriptors in LDS and every
//                   lane reads the same target word (a broadcast); the incumbent (distance, index) stays in registers across the
//                   tiles, which come in ascending order: the lowest-index rule needs no second pass
//   ransac_gather   the m pairs once into a packed array of six floats; a pair with an index out of range becomes six NaNs
//   ransac_model    a thread per candidate: its triple (from the caller's list, or the LCG jumped ahead to its own three draws),
//                   the f64 three-pair solve (a one-sided Jacobi SVD of its own), 12 stored floats + a valid flag
//   ransac_score    the hot path: pair tiles x candidate tiles, as plane_score.  A lane keeps four pairs in registers, the block walks
//                   its candidates (wave-uniform records, scalar loads); per candidate and wave the inlier ballots are counted and
//                   added to an LDS counter by one lane, then one integer atomicAdd per block and candidate.  Integer sums
//   ransac_fold     one block after every chunk of kRansacChunk candidates: the chunk into the device-resident state (the best so
//                   far, the first candidate that reached the early-exit count).  Later launches leave at once when the exit is set
#include "tc_internal.h"
#include "../../include/threecrate_hip_global.h"

#include <algorithm>
#include <cmath>

namespace tc {

constexpr int kMatchSrcPerBlock = 128;                              // sources (= threads) of a matching block
constexpr int kMatchTgtTile = 128;                                  // target descriptors staged in LDS at a time
constexpr int kMatchRow = 36;                                       // floats between two rows of the tile: 33, padded to 16-byte rows
constexpr int kRansacBlock = 256;                                   // threads of a scoring block
constexpr int kRansacPerLane = 4;                                   // pairs a lane keeps in registers
constexpr int kRansacPairsPerBlock = kRansacBlock * kRansacPerLane; // 1024: the pair tile
constexpr int kRansacCandTile = 128;                                // candidates a scoring block walks
constexpr int kRansacChunk = 4096;                                  // candidates between two folds (a multiple of kRansacCandTile)
static_assert(kRansacCandTile <= kRansacBlock && kRansacChunk % kRansacCandTile == 0, "one thread flushes one counter; whole tiles per chunk");
static_assert(kMatchRow >= TC_FPFH_DIM && kMatchRow % 4 == 0, "");

// ---- matching --------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kMatchSrcPerBlock) match_kernel(const float *__restrict__ src, uint32_t ns, const float *__restrict__ tgt,
                                                                  uint32_t nt, uint32_t *__restrict__ out_index, float *__restrict__ out_dist) {
    __shared__ __attribute__((aligned(16))) float tile[kMatchTgtTile * kMatchRow];
    const size_t i = (size_t)blockIdx.x * kMatchSrcPerBlock + threadIdx.x;      // 64-bit: ns and nt go up to 2^32 - 17, a 32-bit counter would wrap
    float s[TC_FPFH_DIM];
#pragma unroll
    for (int j = 0; j < TC_FPFH_DIM; ++j) s[j] = i < ns ? src[i * TC_FPFH_DIM + j] : 0.0f;
    float best = 0.0f;
    uint32_t best_index = 0u;
    for (size_t t0 = 0; t0 < nt; t0 += kMatchTgtTile) {
        const uint32_t cnt = (uint32_t)min((size_t)kMatchTgtTile, (size_t)nt - t0);
        __syncthreads();                                        // the previous tile has been read
        for (uint32_t e = threadIdx.x; e < cnt * TC_FPFH_DIM; e += kMatchSrcPerBlock) {
            const uint32_t r = e / TC_FPFH_DIM;
            tile[r * kMatchRow + (e - r * TC_FPFH_DIM)] = tgt[t0 * TC_FPFH_DIM + e];
        }
        __syncthreads();
        for (uint32_t r = 0; r < cnt; ++r) {
            const float *g = &tile[r * kMatchRow];
            float acc = 0.0f;                                   // :87-89: sub, mul, add, in order (-ffp-contract=off)
#pragma unroll
            for (int j = 0; j < TC_FPFH_DIM; ++j) {
                const float t = s[j] - g[j];
                acc = acc + t * t;
            }
            if (t0 + r == 0u || acc < best) { best = acc; best_index = (uint32_t)(t0 + r); }     // target 0 is the first incumbent, NaN or not
        }
    }
    if (i < ns) {
        out_index[i] = best_index;
        if (out_dist) out_dist[i] = best;
    }
}

static tc_status match_device(tc_context *ctx, const float *d_src, size_t ns, const float *d_tgt, size_t nt, uint32_t *d_index, float *d_dist) {
    ProfScope ps(ctx, "match_features");
    const dim3 grid((unsigned)((ns + kMatchSrcPerBlock - 1) / kMatchSrcPerBlock));
    hipLaunchKernelGGL(match_kernel, grid, dim3(kMatchSrcPerBlock), 0, ctx->stream, d_src, (uint32_t)ns, d_tgt, (uint32_t)nt, d_index, d_dist);
    TC_HIP_TRY(ctx, hipGetLastError());                         // a refused launch is this call's error (the _device road does not wait)
    return TC_OK;
}

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------
// A candidate as the scoring pass reads it (64 bytes, scalar loads).  A candidate without a model is valid == 0 with twelve NaNs:
// every d2 is NaN under it, so it scores 0, and the fold skips it.
struct RansacCand {
    float T[12];            // the stored R (row-major) and t
    uint32_t valid, pad[3];
};
static_assert(sizeof(RansacCand) == 64, "");

// (multiplier, increment) of `steps` LCG steps at once, by repeated squaring (plane.hip has its own copy)
__device__ __forceinline__ void ransac_lcg_jump(uint64_t steps, uint64_t &mult, uint64_t &inc) {
    uint64_t cm = 6364136223846793005ull, ci = 1442695040888963407ull;
    mult = 1; inc = 0;
    for (; steps; steps >>= 1) {
        if (steps & 1) { mult *= cm; inc = inc * cm + ci; }
        ci = (cm + 1) * ci;
        cm *= cm;
    }
}
__device__ __forceinline__ uint32_t ransac_lcg_draw(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 32);
}

__global__ void __launch_bounds__(256) ransac_gather_kernel(const float *__restrict__ src, uint32_t ns, const float *__restrict__ tgt, uint32_t nt,
                                                            const uint32_t *__restrict__ corr_src, const uint32_t *__restrict__ corr_tgt, uint32_t m,
                                                            float *__restrict__ pairs) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const uint32_t si = corr_src[p], ti = corr_tgt[p];
    const bool ok = si < ns && ti < nt;
    float *o = pairs + 6 * p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        o[c] = ok ? src[3 * (size_t)si + c] : NAN;
        o[3 + c] = ok ? tgt[3 * (size_t)ti + c] : NAN;
    }
}

// The rigid transform of three pairs, in f64: centroids, H = sum ds dt^T, H = U S V^T by a one-sided Jacobi (column rotations of
// G = H, accumulated in V: at the end the columns of G are sigma_i u_i), R = V diag(1, 1, det(V U^T)) U^T, t = c_t - R c_s.  H of
// three centred pairs has rank <= 2, so the third pair of singular vectors is u1 x u2, v1 x v2 and the determinant's sign is taken
// care of by the cross products.  false: sigma_2 <= 1e-9 sigma_1.
__device__ bool ransac_solve3(const double s[3][3], const double t[3][3], double R[9], double tr[3]) {
    double cs[3], ct[3], G[3][3], V[3][3];
    for (int a = 0; a < 3; ++a) {
        cs[a] = (s[0][a] + s[1][a] + s[2][a]) / 3.0;
        ct[a] = (t[0][a] + t[1][a] + t[2][a]) / 3.0;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) {
            G[a][b] = (s[0][a] - cs[a]) * (t[0][b] - ct[b]) + (s[1][a] - cs[a]) * (t[1][b] - ct[b]) + (s[2][a] - cs[a]) * (t[2][b] - ct[b]);
            V[a][b] = a == b ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            const double alpha = G[0][p] * G[0][p] + G[1][p] * G[1][p] + G[2][p] * G[2][p];
            const double beta = G[0][q] * G[0][q] + G[1][q] * G[1][q] + G[2][q] * G[2][q];
            const double gamma = G[0][p] * G[0][q] + G[1][p] * G[1][q] + G[2][p] * G[2][q];
            if (gamma == 0.0 || !(fabs(gamma) > 1e-15 * (sqrt(alpha) * sqrt(beta)))) continue;
            rotated = true;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            const double tq = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
            const double c = 1.0 / sqrt(1.0 + tq * tq), sn = c * tq;
            for (int r = 0; r < 3; ++r) {
                const double gp = G[r][p], gq = G[r][q], vp = V[r][p], vq = V[r][q];
                G[r][p] = c * gp - sn * gq; G[r][q] = sn * gp + c * gq;
                V[r][p] = c * vp - sn * vq; V[r][q] = sn * vp + c * vq;
            }
        }
        if (!rotated) break;
    }
    double nrm[3];
    for (int c = 0; c < 3; ++c) nrm[c] = sqrt(G[0][c] * G[0][c] + G[1][c] * G[1][c] + G[2][c] * G[2][c]);
    int i1 = 0;
    if (nrm[1] > nrm[i1]) i1 = 1;
    if (nrm[2] > nrm[i1]) i1 = 2;
    int i2 = i1 == 0 ? 1 : 0;
    for (int c = 0; c < 3; ++c) if (c != i1 && nrm[c] > nrm[i2]) i2 = c;
    if (!(nrm[i2] > 1e-9 * nrm[i1])) return false;             // collinear / coincident / a NaN that slipped through
    double u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
    for (int r = 0; r < 3; ++r) { u1[r] = G[r][i1] / nrm[i1]; u2[r] = G[r][i2] / nrm[i2]; v1[r] = V[r][i1]; v2[r] = V[r][i2]; }
    u3[0] = u1[1] * u2[2] - u1[2] * u2[1]; u3[1] = u1[2] * u2[0] - u1[0] * u2[2]; u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
    v3[0] = v1[1] * v2[2] - v1[2] * v2[1]; v3[1] = v1[2] * v2[0] - v1[0] * v2[2]; v3[2] = v1[0] * v2[1] - v1[1] * v2[0];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = v1[a] * u1[b] + v2[a] * u2[b] + v3[a] * u3[b];
    for (int a = 0; a < 3; ++a) tr[a] = ct[a] - (R[3 * a] * cs[0] + R[3 * a + 1] * cs[1] + R[3 * a + 2] * cs[2]);
    return true;
}

__global__ void __launch_bounds__(256) ransac_model_kernel(const float *__restrict__ pairs, uint32_t m, const uint32_t *__restrict__ samples,
                                                           uint32_t n_cand, uint64_t state0, RansacCand *__restrict__ cand,
                                                           float *__restrict__ cand_transform) {
    const uint32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= n_cand) return;
    uint32_t idx[3];
    bool ok;
    if (samples) {
        for (int k = 0; k < 3; ++k) idx[k] = samples[3 * (size_t)it + k];
        ok = idx[0] < m && idx[1] < m && idx[2] < m && idx[0] != idx[1] && idx[0] != idx[2] && idx[1] != idx[2];
    } else {                                                    // :261-272, distinct by construction (m >= 3)
        uint64_t mult, inc;
        ransac_lcg_jump(3ull * it, mult, inc);
        uint64_t state = state0 * mult + inc;
        idx[0] = ransac_lcg_draw(state) % m;
        idx[1] = ransac_lcg_draw(state) % (m - 1u);
        if (idx[1] >= idx[0]) ++idx[1];
        idx[2] = ransac_lcg_draw(state) % (m - 2u);
        if (idx[2] >= min(idx[0], idx[1])) ++idx[2];
        if (idx[2] >= max(idx[0], idx[1])) ++idx[2];
        ok = true;
    }
    RansacCand rc;
    for (int k = 0; k < 12; ++k) rc.T[k] = NAN;
    rc.valid = 0u; rc.pad[0] = rc.pad[1] = rc.pad[2] = 0u;
    if (ok) {
        double s[3][3], t[3][3], R[9], tr[3];
        bool finite = true;
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) {
                const float a = pairs[6 * (size_t)idx[k] + c], b = pairs[6 * (size_t)idx[k] + 3 + c];
                finite = finite && isfinite(a) && isfinite(b);   // (a pair with an index out of range is six NaNs)
                s[k][c] = (double)a; t[k][c] = (double)b;
            }
        if (finite && ransac_solve3(s, t, R, tr)) {
            for (int k = 0; k < 9; ++k) rc.T[k] = (float)R[k];
            for (int k = 0; k < 3; ++k) rc.T[9 + k] = (float)tr[k];
            rc.valid = 1u;
        }
    }
    cand[it] = rc;
    if (cand_transform)
        for (int k = 0; k < 12; ++k) cand_transform[12 * (size_t)it + k] = rc.T[k];
}

__global__ void __launch_bounds__(kRansacBlock) ransac_score_kernel(const float *__restrict__ pairs, uint32_t m, const RansacCand *__restrict__ cand,
                                                                    uint32_t c_begin, uint32_t c_end, float thr2, const RansacOut *__restrict__ state,
                                                                    uint32_t *__restrict__ counts) {
    __shared__ uint32_t sh[kRansacCandTile];
    if (state->exit) return;                                    // an earlier chunk ended the loop (uniform over the grid)
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const size_t base = (size_t)blockIdx.x * kRansacPairsPerBlock;
    float x[kRansacPerLane], y[kRansacPerLane], z[kRansacPerLane], X[kRansacPerLane], Y[kRansacPerLane], Z[kRansacPerLane];
#pragma unroll
    for (int k = 0; k < kRansacPerLane; ++k) {                  // a lane without a pair holds NaNs: never an inlier
        const size_t p = base + (size_t)k * kRansacBlock + tid;
        const bool in_range = p < m;
        x[k] = in_range ? pairs[6 * p] : NAN; y[k] = in_range ? pairs[6 * p + 1] : NAN; z[k] = in_range ? pairs[6 * p + 2] : NAN;
        X[k] = in_range ? pairs[6 * p + 3] : NAN; Y[k] = in_range ? pairs[6 * p + 4] : NAN; Z[k] = in_range ? pairs[6 * p + 5] : NAN;
    }
    if (tid < kRansacCandTile) sh[tid] = 0u;
    __syncthreads();
    const uint32_t c0 = c_begin + blockIdx.y * kRansacCandTile, c1 = min(c0 + (uint32_t)kRansacCandTile, c_end);
    for (uint32_t j = c0; j < c1; ++j) {
        const RansacCand rc = cand[j];
        uint32_t cnt = 0u;
#pragma unroll
        for (int k = 0; k < kRansacPerLane; ++k) {
            const float dx = (((rc.T[0] * x[k] + rc.T[1] * y[k]) + rc.T[2] * z[k]) + rc.T[9]) - X[k];
            const float dy = (((rc.T[3] * x[k] + rc.T[4] * y[k]) + rc.T[5] * z[k]) + rc.T[10]) - Y[k];
            const float dz = (((rc.T[6] * x[k] + rc.T[7] * y[k]) + rc.T[8] * z[k]) + rc.T[11]) - Z[k];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            cnt += (uint32_t)__popcll(__ballot(d2 <= thr2));
        }
        if (lane == 0u && cnt) atomicAdd(&sh[j - c0], cnt);      // one LDS add per wave and candidate
    }
    __syncthreads();
    if (c0 < c1 && tid < c1 - c0 && sh[tid]) atomicAdd(&counts[c0 + tid], sh[tid]);
}

// candidates [c_begin, c_end) into the state.  The closed form of the loop :291-298: the first candidate that reaches `exit_count`
// wins and ends the loop; otherwise the greatest count wins, the lowest index among equals (an earlier chunk's best stays on a tie)
__global__ void __launch_bounds__(256) ransac_fold_kernel(const RansacCand *__restrict__ cand, const uint32_t *__restrict__ counts, uint32_t c_begin,
                                                          uint32_t c_end, unsigned long long exit_count, RansacOut *__restrict__ state) {
    __shared__ unsigned long long sh_best[256];
    __shared__ uint32_t sh_first[256];
    if (state->exit) return;
    unsigned long long best = 0ull;                             // count in the high word, ~index in the low: max = first of the best
    uint32_t first = 0xFFFFFFFFu;
    for (uint32_t j = c_begin + threadIdx.x; j < c_end; j += 256u) {
        const uint32_t c = counts[j];
        if (c && cand[j].valid) {
            best = max(best, ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - j));
            if ((unsigned long long)c >= exit_count) first = min(first, j);
        }
    }
    sh_best[threadIdx.x] = best; sh_first[threadIdx.x] = first;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh_best[threadIdx.x] = max(sh_best[threadIdx.x], sh_best[threadIdx.x + s]);
            sh_first[threadIdx.x] = min(sh_first[threadIdx.x], sh_first[threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        best = sh_best[0]; first = sh_first[0];
        uint32_t win = 0xFFFFFFFFu;
        if (first != 0xFFFFFFFFu) win = first;
        else if (best && (uint32_t)(best >> 32) > (state->found ? state->count : 0u)) win = 0xFFFFFFFFu - (uint32_t)best;
        if (win != 0xFFFFFFFFu) {
            const RansacCand rc = cand[win];
            for (int k = 0; k < 12; ++k) state->transform[k] = rc.T[k];
            state->count = counts[win]; state->index = win; state->found = 1u;
            state->exit = first != 0xFFFFFFFFu ? 1u : 0u;
        }
    }
}

// :255 -- max(3, ceil(inlier_ratio * m as f32) as usize): the conversion saturates, NaN -> 0
static unsigned long long ransac_exit_count(float inlier_ratio, size_t m) {
    const float e = std::ceil(inlier_ratio * (float)m);
    unsigned long long E = 0ull;
    if (e >= 18446744073709551616.0f) E = ~0ull;
    else if (e > 0.0f) E = (unsigned long long)e;
    return std::max(E, 3ull);
}

// a validated call; device pointers, d_samples null = the seeded generator from state0, d_cand_* optional; transform / result on the host
static tc_status ransac_device(tc_context *ctx, const float *d_src, size_t ns, const float *d_tgt, size_t nt, const uint32_t *d_corr_src,
                               const uint32_t *d_corr_tgt, size_t m, float threshold, float inlier_ratio, const uint32_t *d_samples, size_t n_cand,
                               uint64_t state0, float *transform, tc_ransac_result *result, float *d_cand_transform, uint32_t *d_cand_count) {
    hipStream_t st = ctx->stream;
    const uint32_t m32 = (uint32_t)m, nc = (uint32_t)n_cand;
    // the temporaries of one call, one block: state | candidates | counts | pairs
    ScopedBuf block;
    if (tc_status s = ensure(ctx, block, sizeof(RansacOut) + (size_t)nc * (sizeof(RansacCand) + sizeof(uint32_t)) + m * 6 * sizeof(float))) return s;
    RansacOut *state = (RansacOut *)block.p;
    RansacCand *cand = (RansacCand *)(state + 1);
    uint32_t *counts = (uint32_t *)(cand + nc);
    float *pairs = (float *)(counts + nc);
    TC_HIP_TRY(ctx, hipMemsetAsync(state, 0, sizeof(RansacOut), st));
    TC_HIP_TRY(ctx, hipMemsetAsync(counts, 0, (size_t)nc * sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "ransac_gather");
        hipLaunchKernelGGL(ransac_gather_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_src, (uint32_t)ns, d_tgt, (uint32_t)nt, d_corr_src,
                           d_corr_tgt, m32, pairs);
    }
    {
        ProfScope ps(ctx, "ransac_models");
        hipLaunchKernelGGL(ransac_model_kernel, dim3((nc + 255u) / 256u), dim3(256), 0, st, (const float *)pairs, m32, d_samples, nc, state0, cand,
                           d_cand_transform);
    }
    const float thr2 = threshold * threshold;                   // :155
    const unsigned long long exit_count = ransac_exit_count(inlier_ratio, m);
    const unsigned pair_tiles = (unsigned)((m + kRansacPairsPerBlock - 1) / kRansacPairsPerBlock);
    for (uint32_t c0 = 0; c0 < nc; c0 += kRansacChunk) {        // every chunk is enqueued; the ones behind the exit return at once
        const uint32_t c1 = std::min(c0 + (uint32_t)kRansacChunk, nc);
        {
            ProfScope ps(ctx, "ransac_score");
            const dim3 grid(pair_tiles, (c1 - c0 + kRansacCandTile - 1) / kRansacCandTile);
            hipLaunchKernelGGL(ransac_score_kernel, grid, dim3(kRansacBlock), 0, st, (const float *)pairs, m32, (const RansacCand *)cand, c0, c1, thr2,
                               (const RansacOut *)state, counts);
        }
        {
            ProfScope ps(ctx, "ransac_fold");
            hipLaunchKernelGGL(ransac_fold_kernel, dim3(1), dim3(256), 0, st, (const RansacCand *)cand, (const uint32_t *)counts, c0, c1, exit_count, state);
        }
    }
    if (d_cand_count) TC_HIP_TRY(ctx, hipMemcpyAsync(d_cand_count, counts, (size_t)nc * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    RansacOut *h = &pinned_host(ctx)->ransac_out;
    if (tc_status s = read_back(ctx, h, state, sizeof(RansacOut))) return s;            // the call's one wait
    for (int k = 0; k < 12; ++k) transform[k] = h->found ? h->transform[k] : ((k == 0 || k == 4 || k == 8) ? 1.0f : 0.0f);
    result->inlier_count = h->found ? h->count : 0u;
    result->iterations_run = h->exit ? (uint64_t)h->index + 1u : (uint64_t)nc;
    result->best_iteration = h->found ? h->index : 0u;
    result->early_exit = h->exit ? 1 : 0;
    result->inlier_ratio = (float)result->inlier_count / (float)m;                      // :302-306
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_global.h) -------------------------------------------------
static tc_status match_validate(tc_context *ctx, const float *src, size_t ns, const float *tgt, size_t nt, size_t dim, uint32_t *index, bool *nothing) {
    *nothing = false;
    if (!ctx) return TC_INVALID_DATA;
    if (dim != TC_FPFH_DIM) return fail(ctx, TC_UNSUPPORTED, "match_features: only descriptors of TC_FPFH_DIM = 33 floats are supported by the HIP backend");
    if (ns == 0) { *nothing = true; return TC_OK; }
    if (!src || !tgt || !index) return fail(ctx, TC_INVALID_DATA, "match_features: a descriptor or output array is NULL");
    if (nt == 0) return fail(ctx, TC_INVALID_DATA, "match_features: no target descriptors");
    return check_point_count(ctx, ns, nt);
}

// the reference's message (:235-238) first, then the parameter checks in plane segmentation's words, then the limits
static tc_status ransac_validate(tc_context *ctx, const float *src, size_t ns, const float *tgt, size_t nt, const uint32_t *corr_src,
                                 const uint32_t *corr_tgt, size_t m, float threshold, size_t iters, bool need_samples, const uint32_t *samples,
                                 float *transform, tc_ransac_result *result) {
    if (!ctx || !transform || !result) return TC_INVALID_DATA;
    if (m < 3) return fail(ctx, TC_INVALID_DATA, "Too few feature correspondences for RANSAC (need >= 3)");
    if (threshold <= 0.0f) return fail(ctx, TC_INVALID_DATA, "Threshold must be positive");
    if (iters == 0) return fail(ctx, TC_INVALID_DATA, "Max iterations must be positive");
    if (!src || !tgt || !corr_src || !corr_tgt) return fail(ctx, TC_INVALID_DATA, "ransac_correspondences: a cloud or correspondence array is NULL");
    if (need_samples && !samples) return fail(ctx, TC_INVALID_DATA, "ransac_correspondences_samples: samples is NULL");
    if (tc_status s = check_point_count(ctx, ns, nt)) return s;
    if (tc_status s = check_point_count(ctx, m)) return s;
    if (iters > TC_RANSAC_MAX_ITERS) return fail(ctx, TC_UNSUPPORTED, "ransac_correspondences: more than 2^20 iterations are not supported by the HIP backend");
    return TC_OK;
}

static uint64_t ransac_state0(size_t m, size_t max_iters, uint64_t seed) {
    return (((uint64_t)m << 32) ^ (uint64_t)max_iters ^ 0x9E3779B97F4A7C15ull) ^ seed;
}

static size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// the host twins: clouds, correspondences (+ samples) through in_a, the device road, the candidates back through out_a
static tc_status ransac_host(tc_context *ctx, const float *src, size_t ns, const float *tgt, size_t nt, const uint32_t *corr_src, const uint32_t *corr_tgt,
                             size_t m, float threshold, float inlier_ratio, const uint32_t *samples, size_t n_cand, uint64_t state0, float *transform,
                             tc_ransac_result *result, float *cand_transform, uint32_t *cand_count) {
    const size_t src_b = pad16(ns * 3 * sizeof(float)), tgt_b = pad16(nt * 3 * sizeof(float)), corr_b = pad16(m * sizeof(uint32_t));
    const size_t smp_b = samples ? n_cand * 3 * sizeof(uint32_t) : 0;
    if (tc_status s = ensure(ctx, ctx->in_a, src_b + tgt_b + 2 * corr_b + smp_b)) return s;
    char *base = (char *)ctx->in_a.p;
    float *d_src = (float *)base, *d_tgt = (float *)(base + src_b);
    uint32_t *d_cs = (uint32_t *)(base + src_b + tgt_b), *d_ct = (uint32_t *)(base + src_b + tgt_b + corr_b);
    uint32_t *d_samples = samples ? (uint32_t *)(base + src_b + tgt_b + 2 * corr_b) : nullptr;
    hipStream_t st = ctx->stream;
    if (ns) TC_HIP_TRY(ctx, hipMemcpyAsync(d_src, src, ns * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    if (nt) TC_HIP_TRY(ctx, hipMemcpyAsync(d_tgt, tgt, nt * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_cs, corr_src, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_ct, corr_tgt, m * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (samples) TC_HIP_TRY(ctx, hipMemcpyAsync(d_samples, samples, smp_b, hipMemcpyHostToDevice, st));
    const size_t ct_b = cand_transform ? pad16(n_cand * 12 * sizeof(float)) : 0, cc_b = cand_count ? n_cand * sizeof(uint32_t) : 0;
    if (ct_b + cc_b) { if (tc_status s = ensure(ctx, ctx->out_a, ct_b + cc_b)) return s; }
    float *d_ct_out = cand_transform ? (float *)ctx->out_a.p : nullptr;
    uint32_t *d_cc_out = cand_count ? (uint32_t *)((char *)ctx->out_a.p + ct_b) : nullptr;
    float T[12];
    tc_ransac_result res;
    if (tc_status s = ransac_device(ctx, d_src, ns, d_tgt, nt, d_cs, d_ct, m, threshold, inlier_ratio, d_samples, n_cand, state0, T, &res, d_ct_out, d_cc_out))
        return s;
    if (cand_transform) { if (tc_status s = stage_out(ctx, cand_transform, d_ct_out, n_cand * 12 * sizeof(float))) return s; }
    if (cand_count) { if (tc_status s = stage_out(ctx, cand_count, d_cc_out, cc_b)) return s; }
    for (int k = 0; k < 12; ++k) transform[k] = T[k];
    *result = res;
    return TC_OK;
}

extern "C" {

tc_status tc_match_features_device(tc_context *ctx, const float *d_src_desc, size_t ns, const float *d_tgt_desc, size_t nt, size_t dim,
                                   uint32_t *d_match_index, float *d_match_dist) try {
    bool nothing;
    if (tc_status s = match_validate(ctx, d_src_desc, ns, d_tgt_desc, nt, dim, d_match_index, &nothing)) return s;
    if (nothing) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return match_device(ctx, d_src_desc, ns, d_tgt_desc, nt, d_match_index, d_match_dist);
} TC_CATCH_STATUS(ctx)

tc_status tc_match_features(tc_context *ctx, const float *src_desc, size_t ns, const float *tgt_desc, size_t nt, size_t dim,
                            uint32_t *match_index, float *match_dist) try {
    bool nothing;
    if (tc_status s = match_validate(ctx, src_desc, ns, tgt_desc, nt, dim, match_index, &nothing)) return s;
    if (nothing) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, src_desc, ns * TC_FPFH_DIM * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_b, tgt_desc, nt * TC_FPFH_DIM * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, ctx->out_a, ns * (sizeof(uint32_t) + sizeof(float)))) return s;        // indices | distances
    uint32_t *d_index = (uint32_t *)ctx->out_a.p;
    float *d_dist = match_dist ? (float *)(d_index + ns) : nullptr;
    if (tc_status s = match_device(ctx, (const float *)ctx->in_a.p, ns, (const float *)ctx->in_b.p, nt, d_index, d_dist)) return s;
    if (match_dist) TC_HIP_TRY(ctx, hipMemcpyAsync(match_dist, d_dist, ns * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (tc_status s = stage_out(ctx, match_index, d_index, ns * sizeof(uint32_t))) return s;
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
} TC_CATCH_STATUS(ctx)

tc_status tc_ransac_correspondences_device(tc_context *ctx, const float *d_src_xyz, size_t ns, const float *d_tgt_xyz, size_t nt,
                                           const uint32_t *d_corr_src, const uint32_t *d_corr_tgt, size_t m, float threshold,
                                           float inlier_ratio, size_t max_iters, uint64_t seed, float *transform, tc_ransac_result *result,
                                           float *d_cand_transform, uint32_t *d_cand_count) try {
    if (tc_status s = ransac_validate(ctx, d_src_xyz, ns, d_tgt_xyz, nt, d_corr_src, d_corr_tgt, m, threshold, max_iters, false, nullptr, transform, result))
        return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ransac_device(ctx, d_src_xyz, ns, d_tgt_xyz, nt, d_corr_src, d_corr_tgt, m, threshold, inlier_ratio, nullptr, max_iters,
                         ransac_state0(m, max_iters, seed), transform, result, d_cand_transform, d_cand_count);
} TC_CATCH_STATUS(ctx)

tc_status tc_ransac_correspondences(tc_context *ctx, const float *src_xyz, size_t ns, const float *tgt_xyz, size_t nt,
                                    const uint32_t *corr_src, const uint32_t *corr_tgt, size_t m, float threshold, float inlier_ratio,
                                    size_t max_iters, uint64_t seed, float *transform, tc_ransac_result *result, float *cand_transform,
                                    uint32_t *cand_count) try {
    if (tc_status s = ransac_validate(ctx, src_xyz, ns, tgt_xyz, nt, corr_src, corr_tgt, m, threshold, max_iters, false, nullptr, transform, result))
        return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ransac_host(ctx, src_xyz, ns, tgt_xyz, nt, corr_src, corr_tgt, m, threshold, inlier_ratio, nullptr, max_iters,
                       ransac_state0(m, max_iters, seed), transform, result, cand_transform, cand_count);
} TC_CATCH_STATUS(ctx)

tc_status tc_ransac_correspondences_samples_device(tc_context *ctx, const float *d_src_xyz, size_t ns, const float *d_tgt_xyz, size_t nt,
                                                   const uint32_t *d_corr_src, const uint32_t *d_corr_tgt, size_t m, float threshold,
                                                   float inlier_ratio, const uint32_t *d_samples, size_t n_samples, float *transform,
                                                   tc_ransac_result *result, float *d_cand_transform, uint32_t *d_cand_count) try {
    if (tc_status s = ransac_validate(ctx, d_src_xyz, ns, d_tgt_xyz, nt, d_corr_src, d_corr_tgt, m, threshold, n_samples, true, d_samples, transform, result))
        return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ransac_device(ctx, d_src_xyz, ns, d_tgt_xyz, nt, d_corr_src, d_corr_tgt, m, threshold, inlier_ratio, d_samples, n_samples, 0ull, transform,
                         result, d_cand_transform, d_cand_count);
} TC_CATCH_STATUS(ctx)

tc_status tc_ransac_correspondences_samples(tc_context *ctx, const float *src_xyz, size_t ns, const float *tgt_xyz, size_t nt,
                                            const uint32_t *corr_src, const uint32_t *corr_tgt, size_t m, float threshold,
                                            float inlier_ratio, const uint32_t *samples, size_t n_samples, float *transform,
                                            tc_ransac_result *result, float *cand_transform, uint32_t *cand_count) try {
    if (tc_status s = ransac_validate(ctx, src_xyz, ns, tgt_xyz, nt, corr_src, corr_tgt, m, threshold, n_samples, true, samples, transform, result))
        return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ransac_host(ctx, src_xyz, ns, tgt_xyz, nt, corr_src, corr_tgt, m, threshold, inlier_ratio, samples, n_samples, 0ull, transform, result,
                       cand_transform, cand_count);
} TC_CATCH_STATUS(ctx)

}  // extern "C"
