// tsdf.hip -- TSDF depth fusion and surface extraction on a dense device volume (threecrate-gpu/src/tsdf.rs, tsdf_integration.wgsl,
// surface_extraction.wgsl); the entry points of include/threecrate_hip_tsdf.h, which pins the arithmetic.
//   tsdf_integrate   a wave owns kTsdfRun voxels along x of one (y, z) row.  Projection and the depth gather come first (the image is
//                    small and stays in cache); a lane touches its voxel -- ONE 8-byte load, one 8-byte store -- only when it has a
//                    depth to fuse, so a wave without such a lane neither reads nor writes state.  Every voxel is projected from its
//                    own integer coordinates: marching along an axis would change the rounding.  Only when the caller asks for the
//                    count (an instantiation of its own) are the updated voxels counted: ballot + popcount per wave, one integer
//                    atomic per block.
//   tsdf_count       a wave owns kTsdfRun cubes along x of one row of cubes, a block kTsdfBlock / kTsdfRun consecutive runs: the
//                    blocks are contiguous in the order of the output.  Each lane counts the points of its cube; one total per block
//   exclusive_scan_u32 (grid.hip)   over the block totals
//   tsdf_fill        recomputes every cube's edges, ranks the cube inside its block and writes its points.  Nothing per cube is
//                    ever in memory.
//   tsdf_reset / tsdf_pack / tsdf_unpack   the initial state; the state from / into the arrays of the upload / download calls
#include "tc_internal.h"
#include "../../include/threecrate_hip_tsdf.h"

#include <algorithm>
#include <cmath>
#include <vector>

struct tc_tsdf_volume {
    tc_context *ctx = nullptr;
    tc_tsdf_volume_config cfg{};
    size_t nvox = 0;
    tc::DevBuf state;               // nvox x { f32 tsdf; u32 weight << 24 | r << 16 | g << 8 | b }, owned
    tc::DevBuf counter;             // one u32: the updated voxels of the integration in flight, owned
};

namespace tc {

constexpr int kTsdfRunsPerBlock = kTsdfBlock / kTsdfRun;
static_assert(kTsdfRun == 64 && kTsdfBlock % kTsdfRun == 0, "a run is one wave");

struct TsdfGeom {
    float    vs, tau;
    float    ox, oy, oz;
    uint32_t rx, ry, rz;
    uint32_t max_w;
    uint32_t nseg;          // runs per row: of voxels (integration) or of cubes (extraction)
    uint32_t nruns;         // runs in all
};
struct TsdfCam {
    float    fx, fy, cx, cy;
    float    wf, hf;        // f32(width), f32(height)
    uint32_t w;
    float    m[12];
};

constexpr uint32_t kTsdfInitialBits = 0x3F800000u;      // tsdf = 1.0f (weight 0, colour 0 in the other word)

__global__ void __launch_bounds__(256) tsdf_reset_kernel(uint2 *__restrict__ state, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) state[i] = make_uint2(kTsdfInitialBits, 0u);
}

__global__ void __launch_bounds__(256) tsdf_pack_kernel(uint2 *__restrict__ state, size_t n, const float *__restrict__ tsdf,
                                                       const uint8_t *__restrict__ weight, const uint8_t *__restrict__ rgb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w = (uint32_t)weight[i] << 24;
    if (rgb) w |= (uint32_t)rgb[3 * i] << 16 | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2];
    state[i] = make_uint2(__float_as_uint(tsdf[i]), w);
}

__global__ void __launch_bounds__(256) tsdf_unpack_kernel(const uint2 *__restrict__ state, size_t n, float *__restrict__ tsdf,
                                                         uint8_t *__restrict__ weight, uint8_t *__restrict__ rgb) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint2 s = state[i];
    if (tsdf) tsdf[i] = __uint_as_float(s.x);
    if (weight) weight[i] = (uint8_t)(s.y >> 24);
    if (rgb) { rgb[3 * i] = (uint8_t)(s.y >> 16); rgb[3 * i + 1] = (uint8_t)(s.y >> 8); rgb[3 * i + 2] = (uint8_t)s.y; }
}

// the run of this wave: its row (z ry + y, or the row of cubes) and first x; false past the last run
__device__ __forceinline__ bool tsdf_run(const TsdfGeom &g, uint32_t rows_y, uint32_t &x0, uint32_t &y, uint32_t &z) {
    const uint32_t run = __builtin_amdgcn_readfirstlane(blockIdx.x * kTsdfRunsPerBlock + (threadIdx.x >> 6));
    if (run >= g.nruns) return false;
    const uint32_t row = run / g.nseg;
    x0 = (run - row * g.nseg) * kTsdfRun;
    z = row / rows_y;
    y = row - z * rows_y;
    return true;
}

// COUNT: the caller wants n_updated.  Without it there is no LDS word, no barrier and no atomic
template <bool COUNT>
__global__ void __launch_bounds__(kTsdfBlock) tsdf_integrate_kernel(uint2 *__restrict__ state, const float *__restrict__ depth,
                                                                   const uint8_t *__restrict__ rgb, TsdfGeom g, TsdfCam c,
                                                                   uint32_t *__restrict__ n_updated) {
    const uint32_t lane = threadIdx.x & 63;
    uint32_t x0 = 0, y = 0, z = 0;
    bool ok = false;
    size_t vi = 0, pix = 0;
    float cz = 0.0f, d = 0.0f;
    if (tsdf_run(g, g.ry, x0, y, z)) {
        const uint32_t x = x0 + lane;
        if (x < g.rx) {
            vi = ((size_t)z * g.ry + y) * g.rx + x;
            const float wx = (float)x * g.vs + g.ox, wy = (float)y * g.vs + g.oy, wz = (float)z * g.vs + g.oz;
            const float cx = ((c.m[0] * wx + c.m[1] * wy) + c.m[2] * wz) + c.m[3];
            const float cy = ((c.m[4] * wx + c.m[5] * wy) + c.m[6] * wz) + c.m[7];
            cz = ((c.m[8] * wx + c.m[9] * wy) + c.m[10] * wz) + c.m[11];
            if (cz > 0.0f) {
                const float a = ((cx / cz) * c.fx + c.cx) + 0.5f, b = ((cy / cz) * c.fy + c.cy) + 0.5f;
                if (a >= 0.0f && a < c.wf && b >= 0.0f && b < c.hf) {        // (a NaN fails)
                    pix = (size_t)(uint32_t)b * c.w + (uint32_t)a;
                    d = depth[pix];
                    ok = d > 0.0f && d < INFINITY;
                }
            }
        }
    }
    if (ok) {
        const uint2 s = state[vi];
        const float t = fminf(fmaxf(d - cz, -g.tau), g.tau);
        const uint32_t w1 = min((s.y >> 24) + 1u, g.max_w);
        const float alpha = 1.0f / (float)w1, keep = 1.0f - alpha;
        const float tsdf = keep * __uint_as_float(s.x) + alpha * t;
        uint32_t colour = s.y & 0xFFFFFFu;
        if (rgb) {
            const uint32_t pr = rgb[3 * pix], pg = rgb[3 * pix + 1], pb = rgb[3 * pix + 2];
            if (pr | pg | pb) {
                const uint32_t r = (uint32_t)fminf(fmaxf(keep * (float)(colour >> 16) + alpha * (float)pr, 0.0f), 255.0f);
                const uint32_t gr = (uint32_t)fminf(fmaxf(keep * (float)((colour >> 8) & 0xFFu) + alpha * (float)pg, 0.0f), 255.0f);
                const uint32_t bl = (uint32_t)fminf(fmaxf(keep * (float)(colour & 0xFFu) + alpha * (float)pb, 0.0f), 255.0f);
                colour = r << 16 | gr << 8 | bl;
            }
        }
        state[vi] = make_uint2(__float_as_uint(tsdf), w1 << 24 | colour);
    }
    if constexpr (COUNT) {
        __shared__ uint32_t wcount[kTsdfRunsPerBlock];
        const unsigned long long updated = __ballot(ok);
        if (lane == 0) wcount[threadIdx.x >> 6] = (uint32_t)__popcll(updated);
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t total = 0;
#pragma unroll
            for (int w = 0; w < kTsdfRunsPerBlock; ++w) total += wcount[w];
            if (total) atomicAdd(n_updated, total);
        }
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------------------
// corner c = x + 2 y + 4 z of a cube; edge e = 4 axis + j runs from corner a to corner a + (1 << axis), where a takes the two bits of
// j on the other two axes in their order: the shader's order (include/threecrate_hip_tsdf.h)
__device__ __forceinline__ constexpr int tsdf_edge_from(int e) {
    return (e >> 2) == 0 ? (e & 3) << 1 : (e >> 2) == 1 ? ((e & 1) | (e & 2) << 1) : (e & 3);
}

// the corner values of the cube at voxel vi and the mask of its emitting edges; 0 when the base voxel was never observed
__device__ __forceinline__ uint32_t tsdf_cube(const uint2 *__restrict__ state, const TsdfGeom &g, size_t vi, float iso, uint32_t observed_only,
                                              float v[8], uint32_t &colour) {
    const uint2 base = state[vi];
    if ((base.y >> 24) == 0) return 0;
    colour = base.y & 0xFFFFFFu;
    const size_t sy = g.rx, sz = (size_t)g.rx * g.ry;
    uint32_t seen = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint2 s = c == 0 ? base : state[vi + (c & 1) + ((c >> 1) & 1) * sy + (size_t)(c >> 2) * sz];
        const bool has = (s.y >> 24) != 0;
        v[c] = has ? __uint_as_float(s.x) - iso : g.tau;
        seen |= (uint32_t)has << c;
    }
    uint32_t mask = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        const int a = tsdf_edge_from(e), b = a + (1 << (e >> 2));
        const bool both = ((seen >> a) & (seen >> b) & 1u) != 0;
        if (v[a] * v[b] <= 0.0f && (both || !observed_only)) mask |= 1u << e;
    }
    return mask;
}

__global__ void __launch_bounds__(kTsdfBlock) tsdf_count_kernel(const uint2 *__restrict__ state, TsdfGeom g, float iso, uint32_t observed_only,
                                                               uint32_t *__restrict__ block_total) {
    __shared__ uint32_t wsum[kTsdfRunsPerBlock];
    uint32_t x0 = 0, y = 0, z = 0, n = 0;
    if (tsdf_run(g, g.ry - 1, x0, y, z)) {
        const uint32_t x = x0 + (threadIdx.x & 63);
        if (x < g.rx - 1) {
            float v[8];
            uint32_t colour;
            n = (uint32_t)__popc(tsdf_cube(state, g, ((size_t)z * g.ry + y) * g.rx + x, iso, observed_only, v, colour));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int w = 0; w < kTsdfRunsPerBlock; ++w) total += wsum[w];
        block_total[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(kTsdfBlock) tsdf_fill_kernel(const uint2 *__restrict__ state, TsdfGeom g, float iso, uint32_t observed_only,
                                                              const uint32_t *__restrict__ block_start, float *__restrict__ xyz,
                                                              uint8_t *__restrict__ rgb) {
    __shared__ uint32_t wsum[kTsdfRunsPerBlock];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x0 = 0, y = 0, z = 0, mask = 0, colour = 0, x = 0;
    float v[8];
    if (tsdf_run(g, g.ry - 1, x0, y, z)) {
        x = x0 + lane;
        if (x < g.rx - 1) mask = tsdf_cube(state, g, ((size_t)z * g.ry + y) * g.rx + x, iso, observed_only, v, colour);
    }
    const uint32_t n = (uint32_t)__popc(mask);
    uint32_t inc = n;                                           // the cube's rank inside its block: wave prefix + the waves in front
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o);
        if (lane >= (unsigned)o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    if (!mask) return;
    size_t o = (size_t)block_start[blockIdx.x] + (inc - n);
    for (uint32_t w = 0; w < wave; ++w) o += wsum[w];
    const uint32_t base[3] = {x, y, z};
#pragma unroll
    for (int e = 0; e < 12; ++e) {
        if (!(mask & (1u << e))) continue;
        const int axis = e >> 2, a = tsdf_edge_from(e), b = a + (1 << axis);
        const float va = v[a], vb = v[b];
        float p[3];
        // pa; along the other two axes pb = pa, and both rules return pa there: 0.5 (pa + pa) and pa + s 0 with a finite s
        p[0] = g.ox + (float)(base[0] + (a & 1)) * g.vs;
        p[1] = g.oy + (float)(base[1] + ((a >> 1) & 1)) * g.vs;
        p[2] = g.oz + (float)(base[2] + (a >> 2)) * g.vs;
        const float org = axis == 0 ? g.ox : axis == 1 ? g.oy : g.oz;
        const float pa = p[axis], pb = org + (float)(base[axis] + 1u) * g.vs;
        if (fabsf(va - vb) < 0.00001f) p[axis] = 0.5f * (pa + pb);
        else p[axis] = pa + fminf(fmaxf(va / (va - vb), 0.0f), 1.0f) * (pb - pa);
        if (xyz) { xyz[3 * o] = p[0]; xyz[3 * o + 1] = p[1]; xyz[3 * o + 2] = p[2]; }
        if (rgb) { rgb[3 * o] = (uint8_t)(colour >> 16); rgb[3 * o + 1] = (uint8_t)(colour >> 8); rgb[3 * o + 2] = (uint8_t)colour; }
        ++o;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
static TsdfGeom tsdf_geom(const tc_tsdf_volume *vol, bool cubes) {
    const tc_tsdf_volume_config &c = vol->cfg;
    TsdfGeom g{};
    g.vs = c.voxel_size; g.tau = c.truncation_distance;
    g.ox = c.origin[0]; g.oy = c.origin[1]; g.oz = c.origin[2];
    g.rx = c.resolution[0]; g.ry = c.resolution[1]; g.rz = c.resolution[2];
    g.max_w = c.max_weight;
    const uint32_t d = cubes ? 1u : 0u;                         // a row of rx voxels has rx - 1 cubes; there are ry - 1 rows of them per slice
    g.nseg = (g.rx - d + kTsdfRun - 1) / kTsdfRun;
    g.nruns = g.nseg * (g.ry - d) * (g.rz - d);                 // <= voxels <= 2^28
    return g;
}
static unsigned tsdf_blocks(const TsdfGeom &g) { return (unsigned)((g.nruns + kTsdfRunsPerBlock - 1) / kTsdfRunsPerBlock); }
static tc_status tsdf_reset(tc_tsdf_volume *vol) {
    tc_context *ctx = vol->ctx;
    ProfScope ps(ctx, "tsdf_reset");
    hipLaunchKernelGGL(tsdf_reset_kernel, dim3(blocks_for(vol->nvox)), dim3(256), 0, ctx->stream, (uint2 *)vol->state.p, vol->nvox);
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

static tc_status tsdf_integrate_device(tc_tsdf_volume *vol, const float *d_depth, const uint8_t *d_rgb, const tc_camera_intrinsics *in,
                                       const float *m, size_t *n_updated) {
    tc_context *ctx = vol->ctx;
    const TsdfGeom g = tsdf_geom(vol, false);
    TsdfCam c{};
    c.fx = in->fx; c.fy = in->fy; c.cx = in->cx; c.cy = in->cy;
    c.wf = (float)in->width; c.hf = (float)in->height; c.w = in->width;
    for (int k = 0; k < 12; ++k) c.m[k] = m[k];
    if (n_updated) TC_HIP_TRY(ctx, hipMemsetAsync(vol->counter.p, 0, sizeof(uint32_t), ctx->stream));
    {
        ProfScope ps(ctx, "tsdf_integrate");
        if (n_updated)
            hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3(tsdf_blocks(g)), dim3(kTsdfBlock), 0, ctx->stream, (uint2 *)vol->state.p, d_depth, d_rgb, g,
                               c, (uint32_t *)vol->counter.p);
        else
            hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3(tsdf_blocks(g)), dim3(kTsdfBlock), 0, ctx->stream, (uint2 *)vol->state.p, d_depth, d_rgb, g,
                               c, (uint32_t *)nullptr);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (!n_updated) return TC_OK;
    TsdfOut *h = &pinned_host(ctx)->tsdf_out;
    if (tc_status s = read_back(ctx, &h->n_updated, vol->counter.p, sizeof(uint32_t))) return s;
    *n_updated = h->n_updated;
    return TC_OK;
}

// count, scan, [fill]: the caller's arrays, each optional, are device arrays, or -- on_host -- host arrays that are filled through a
// device block of exactly the result's size, allocated once the count is known; the stream is drained on return (the scratch is released)
static tc_status tsdf_extract(tc_tsdf_volume *vol, float iso, uint32_t flags, float *xyz, uint8_t *rgb, size_t capacity, size_t *n_points, bool on_host) {
    tc_context *ctx = vol->ctx;
    const tc_tsdf_volume_config &cfg = vol->cfg;
    *n_points = 0;
    if (cfg.resolution[0] < 2 || cfg.resolution[1] < 2 || cfg.resolution[2] < 2) return TC_OK;     // no cube
    const TsdfGeom g = tsdf_geom(vol, true);
    const unsigned nb = tsdf_blocks(g);
    const uint32_t observed_only = flags & TC_TSDF_OBSERVED_EDGES;
    ScopedBuf words, blocksum;                                  // block totals (nb) | their exclusive prefix (nb + 1)
    if (tc_status s = ensure(ctx, words, ((size_t)2 * nb + 1) * sizeof(uint32_t))) return s;
    uint32_t *total = (uint32_t *)words.p, *start = total + nb;
    {
        ProfScope ps(ctx, "tsdf_count");
        hipLaunchKernelGGL(tsdf_count_kernel, dim3(nb), dim3(kTsdfBlock), 0, ctx->stream, (const uint2 *)vol->state.p, g, iso, observed_only, total);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tc_status s = exclusive_scan_u32(ctx, total, nb, start, blocksum)) return s;
    TsdfOut *h = &pinned_host(ctx)->tsdf_out;
    if (tc_status s = read_back(ctx, &h->n_points, start + nb, sizeof(uint32_t))) return s;
    const size_t n = h->n_points;
    *n_points = n;
    if (n == 0 || (!xyz && !rgb)) return TC_OK;
    if (capacity < n) return fail(ctx, TC_INVALID_DATA, "tsdf_extract_surface: capacity is smaller than the number of points");
    ScopedBuf staged;                                           // on_host: xyz (12 n) | rgb (3 n)
    float *d_xyz = xyz;
    uint8_t *d_rgb = rgb;
    if (on_host) {
        if (tc_status s = ensure(ctx, staged, n * 15)) return s;
        d_xyz = xyz ? (float *)staged.p : nullptr;
        d_rgb = rgb ? (uint8_t *)staged.p + n * 12 : nullptr;
    }
    {
        ProfScope ps(ctx, "tsdf_fill");
        hipLaunchKernelGGL(tsdf_fill_kernel, dim3(nb), dim3(kTsdfBlock), 0, ctx->stream, (const uint2 *)vol->state.p, g, iso, observed_only,
                           (const uint32_t *)start, d_xyz, d_rgb);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (on_host && xyz) TC_HIP_TRY(ctx, hipMemcpyAsync(xyz, d_xyz, n * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (on_host && rgb) TC_HIP_TRY(ctx, hipMemcpyAsync(rgb, d_rgb, n * 3, hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_tsdf.h) ---------------------------------------------------------------------------------
static tc_status tsdf_check_config(tc_context *ctx, const tc_tsdf_volume_config *c, size_t *nvox) {
    if (!(std::isfinite(c->voxel_size) && c->voxel_size > 0.0f)) return fail(ctx, TC_INVALID_DATA, "tsdf_volume: voxel_size must be positive and finite");
    if (!(std::isfinite(c->truncation_distance) && c->truncation_distance > 0.0f))
        return fail(ctx, TC_INVALID_DATA, "tsdf_volume: truncation_distance must be positive and finite");
    if (!c->resolution[0] || !c->resolution[1] || !c->resolution[2]) return fail(ctx, TC_INVALID_DATA, "tsdf_volume: every resolution must be at least 1");
    if (!(std::isfinite(c->origin[0]) && std::isfinite(c->origin[1]) && std::isfinite(c->origin[2])))
        return fail(ctx, TC_INVALID_DATA, "tsdf_volume: origin must be finite");
    // every voxel position f32(i) voxel_size + origin is finite: the extraction's interpolation rests on it (pa + s 0 = pa)
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite((float)c->resolution[k] * c->voxel_size + std::fabs(c->origin[k])))
            return fail(ctx, TC_INVALID_DATA, "tsdf_volume: resolution x voxel_size + |origin| must be finite");
    if (c->max_weight < 1 || c->max_weight > 255) return fail(ctx, TC_INVALID_DATA, "tsdf_volume: max_weight must be in 1..255");
    // (each factor is below 2^32: the product of two fits 64 bits, and is compared before the third comes in)
    const uint64_t xy = (uint64_t)c->resolution[0] * c->resolution[1];
    if (xy > kTsdfMaxVoxels || xy * c->resolution[2] > kTsdfMaxVoxels) return fail(ctx, TC_UNSUPPORTED, "tsdf_volume: more than 2^28 voxels");
    *nvox = (size_t)(xy * c->resolution[2]);
    return TC_OK;
}

static tc_status tsdf_check_frame(tc_tsdf_volume *vol, const float *depth, const tc_camera_intrinsics *in, const float *m) {
    if (!vol) return TC_INVALID_DATA;
    tc_context *ctx = vol->ctx;
    if (!depth || !in || !m) return fail(ctx, TC_INVALID_DATA, "tsdf_integrate: depth, intrinsics or world_to_camera is NULL");
    if (!(std::isfinite(in->fx) && std::isfinite(in->fy) && std::isfinite(in->cx) && std::isfinite(in->cy)))
        return fail(ctx, TC_INVALID_DATA, "tsdf_integrate: the intrinsics must be finite");
    if (!in->width || !in->height) return fail(ctx, TC_INVALID_DATA, "tsdf_integrate: width and height must be at least 1");
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(m[k])) return fail(ctx, TC_INVALID_DATA, "tsdf_integrate: world_to_camera must be finite");
    if ((uint64_t)in->width * in->height >= (1ull << 31)) return fail(ctx, TC_UNSUPPORTED, "tsdf_integrate: an image of 2^31 pixels or more");
    return TC_OK;
}

static tc_status tsdf_check_extract(tc_tsdf_volume *vol, float iso, uint32_t flags, size_t *n_points) {
    if (!vol || !n_points) return TC_INVALID_DATA;
    *n_points = 0;
    if (flags & ~TC_TSDF_OBSERVED_EDGES) return fail(vol->ctx, TC_INVALID_DATA, "tsdf_extract_surface: unknown flag");
    if (!std::isfinite(iso)) return fail(vol->ctx, TC_INVALID_DATA, "tsdf_extract_surface: iso_value must be finite");
    return TC_OK;
}

extern "C" {

tc_status tc_tsdf_volume_create(tc_context *ctx, const tc_tsdf_volume_config *cfg, tc_tsdf_volume **out) try {
    if (!out) return TC_INVALID_DATA;
    *out = nullptr;
    if (!cfg) return ctx ? fail(ctx, TC_INVALID_DATA, "tsdf_volume: config is NULL") : TC_INVALID_DATA;
    size_t nvox = 0;
    if (tc_status s = tsdf_check_config(ctx, cfg, &nvox)) return s;      // (before any device work: also without a context)
    if (!ctx) return TC_INVALID_DATA;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    tc_tsdf_volume *vol = new tc_tsdf_volume();
    vol->ctx = ctx; vol->cfg = *cfg; vol->nvox = nvox;
    // the state is large and lives long: a block of exactly its size from the device, not a padded one from the pool (destroy frees it)
    tc_status s = TC_OK;
    if (hipMalloc(&vol->state.p, nvox * sizeof(uint2)) != hipSuccess) {
        (void)hipGetLastError();
        vol->state.p = nullptr;
        s = fail(ctx, TC_GPU, "tsdf_volume: out of device memory");
    } else vol->state.cap = nvox * sizeof(uint2);
    if (s == TC_OK) s = ensure(ctx, vol->counter, 256);
    if (s == TC_OK) s = tsdf_reset(vol);
    if (s != TC_OK) { free_buf(vol->state); recycle(ctx, vol->counter); delete vol; return s; }
    *out = vol;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

void tc_tsdf_volume_destroy(tc_tsdf_volume *vol) try {
    if (!vol) return;
    (void)hipSetDevice(vol->ctx->device);
    (void)hipStreamSynchronize(vol->ctx->stream);
    // a volume lives long and is large: its state goes back to the device, not into the pool that serves a handle per frame
    free_buf(vol->state);
    recycle(vol->ctx, vol->counter);
    delete vol;
} TC_CATCH_VOID

tc_status tc_tsdf_volume_reset(tc_tsdf_volume *vol) try {
    if (!vol) return TC_INVALID_DATA;
    TC_HIP_TRY(vol->ctx, hipSetDevice(vol->ctx->device));
    if (tc_status s = tsdf_reset(vol)) return s;
    return synced(vol->ctx);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_integrate_device(tc_tsdf_volume *vol, const float *d_depth, const uint8_t *d_rgb, const tc_camera_intrinsics *intrinsics,
                                   const float world_to_camera[12], size_t *n_updated) try {
    if (tc_status s = tsdf_check_frame(vol, d_depth, intrinsics, world_to_camera)) return s;
    TC_HIP_TRY(vol->ctx, hipSetDevice(vol->ctx->device));
    return tsdf_integrate_device(vol, d_depth, d_rgb, intrinsics, world_to_camera, n_updated);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_integrate(tc_tsdf_volume *vol, const float *depth, const uint8_t *rgb, const tc_camera_intrinsics *intrinsics,
                            const float world_to_camera[12], size_t *n_updated) try {
    if (tc_status s = tsdf_check_frame(vol, depth, intrinsics, world_to_camera)) return s;
    tc_context *ctx = vol->ctx;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t npix = (size_t)intrinsics->width * intrinsics->height;
    if (tc_status s = stage_in(ctx, ctx->in_a, depth, npix * sizeof(float))) return s;
    if (rgb) if (tc_status s = stage_in(ctx, ctx->in_b, rgb, npix * 3)) return s;
    if (tc_status s = tsdf_integrate_device(vol, (const float *)ctx->in_a.p, rgb ? (const uint8_t *)ctx->in_b.p : nullptr, intrinsics, world_to_camera,
                                            n_updated)) return s;
    return synced(ctx);                                         // the caller's buffers are free, the volume is updated
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_volume_download_device(tc_tsdf_volume *vol, float *d_tsdf, uint8_t *d_weight, uint8_t *d_rgb) try {
    if (!vol) return TC_INVALID_DATA;
    tc_context *ctx = vol->ctx;
    if (!d_tsdf && !d_weight && !d_rgb) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "tsdf_unpack");
        hipLaunchKernelGGL(tsdf_unpack_kernel, dim3(blocks_for(vol->nvox)), dim3(256), 0, ctx->stream, (const uint2 *)vol->state.p, vol->nvox, d_tsdf,
                           d_weight, d_rgb);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_volume_download(tc_tsdf_volume *vol, float *tsdf, uint8_t *weight, uint8_t *rgb) try {
    if (!vol) return TC_INVALID_DATA;
    tc_context *ctx = vol->ctx;
    if (!tsdf && !weight && !rgb) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t n = vol->nvox;
    ScopedBuf arrays;                                           // tsdf (4 n) | weight (n) | rgb (3 n)
    if (tc_status s = ensure(ctx, arrays, 8 * n)) return s;
    float *d_tsdf = (float *)arrays.p;
    uint8_t *d_weight = (uint8_t *)arrays.p + 4 * n, *d_rgb = d_weight + n;
    {
        ProfScope ps(ctx, "tsdf_unpack");
        hipLaunchKernelGGL(tsdf_unpack_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, (const uint2 *)vol->state.p, n, tsdf ? d_tsdf : nullptr,
                           weight ? d_weight : nullptr, rgb ? d_rgb : nullptr);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (tsdf) TC_HIP_TRY(ctx, hipMemcpyAsync(tsdf, d_tsdf, 4 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (weight) TC_HIP_TRY(ctx, hipMemcpyAsync(weight, d_weight, n, hipMemcpyDeviceToHost, ctx->stream));
    if (rgb) TC_HIP_TRY(ctx, hipMemcpyAsync(rgb, d_rgb, 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_volume_upload_device(tc_tsdf_volume *vol, const float *d_tsdf, const uint8_t *d_weight, const uint8_t *d_rgb) try {
    if (!vol) return TC_INVALID_DATA;
    tc_context *ctx = vol->ctx;
    if (!d_tsdf || !d_weight) return fail(ctx, TC_INVALID_DATA, "tsdf_volume_upload: tsdf or weight is NULL");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    {
        ProfScope ps(ctx, "tsdf_pack");
        hipLaunchKernelGGL(tsdf_pack_kernel, dim3(blocks_for(vol->nvox)), dim3(256), 0, ctx->stream, (uint2 *)vol->state.p, vol->nvox, d_tsdf, d_weight,
                           d_rgb);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_volume_upload(tc_tsdf_volume *vol, const float *tsdf, const uint8_t *weight, const uint8_t *rgb) try {
    if (!vol) return TC_INVALID_DATA;
    tc_context *ctx = vol->ctx;
    if (!tsdf || !weight) return fail(ctx, TC_INVALID_DATA, "tsdf_volume_upload: tsdf or weight is NULL");
    const size_t n = vol->nvox;
    for (size_t i = 0; i < n; ++i)
        if (weight[i] > vol->cfg.max_weight) return fail(ctx, TC_INVALID_DATA, "tsdf_volume_upload: a weight is above max_weight");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedBuf arrays;                                           // tsdf (4 n) | weight (n) | rgb (3 n)
    if (tc_status s = ensure(ctx, arrays, 8 * n)) return s;
    float *d_tsdf = (float *)arrays.p;
    uint8_t *d_weight = (uint8_t *)arrays.p + 4 * n, *d_rgb = d_weight + n;
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_tsdf, tsdf, 4 * n, hipMemcpyHostToDevice, ctx->stream));
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_weight, weight, n, hipMemcpyHostToDevice, ctx->stream));
    if (rgb) TC_HIP_TRY(ctx, hipMemcpyAsync(d_rgb, rgb, 3 * n, hipMemcpyHostToDevice, ctx->stream));
    {
        ProfScope ps(ctx, "tsdf_pack");
        hipLaunchKernelGGL(tsdf_pack_kernel, dim3(blocks_for(n)), dim3(256), 0, ctx->stream, (uint2 *)vol->state.p, n, (const float *)d_tsdf,
                           (const uint8_t *)d_weight, rgb ? (const uint8_t *)d_rgb : nullptr);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    return synced(ctx);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_extract_surface_device(tc_tsdf_volume *vol, float iso_value, uint32_t flags, float *d_xyz, uint8_t *d_rgb, size_t capacity,
                                         size_t *n_points) try {
    if (tc_status s = tsdf_check_extract(vol, iso_value, flags, n_points)) return s;
    TC_HIP_TRY(vol->ctx, hipSetDevice(vol->ctx->device));
    return tsdf_extract(vol, iso_value, flags, d_xyz, d_rgb, capacity, n_points, false);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

tc_status tc_tsdf_extract_surface(tc_tsdf_volume *vol, float iso_value, uint32_t flags, float *xyz, uint8_t *rgb, size_t capacity,
                                  size_t *n_points) try {
    if (tc_status s = tsdf_check_extract(vol, iso_value, flags, n_points)) return s;
    tc_context *ctx = vol->ctx;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return tsdf_extract(vol, iso_value, flags, xyz, rgb, capacity, n_points, true);
} TC_CATCH_STATUS(vol ? vol->ctx : nullptr)

}  // extern "C"
