// color.hip -- colour a point cloud from registered camera images (colorize_point_cloud / colorize_from_images,
// threecrate-algorithms/src/colorization.rs:203-331); the entry points of include/threecrate_hip_color.h, which pins the arithmetic.
// This unit is the whole of the companion library libthreecrate_hip_color.so; the host layer of tc_internal.h (ensure, stage_in,
// read_back, synced, ProfScope) resolves from libthreecrate_hip.so.
//   One road per call:
//   color_table     the caller's source table (host memory) travels as kernel arguments, kColorTableChunk sources a launch, and is
//                   written to the device: no copy that would have to outlive the caller's array, no host wait
//   colorize        a lane per point; the sources in order (their records are wave-uniform reads), the first that colours the point
//                   ends its loop.  Byte loads for the texels, three byte stores for the colour.  COUNT: the block's coloured points
//                   (ballot popcounts per wave, summed over the block) go with ONE atomic into slice blockIdx % kColorSlices
//   -- with a count: one read-back of the slices, added up on the host --
//   The device scratch (table | slices | the host road's outputs) is the context's out_a; the host road stages the cloud in in_a, the
//   images in in_b and the depth images in in_c.
// No FMA contraction: the unit is compiled with the library's -ffp-contract=off (csrc/Makefile, CXXFLAGS), and the pragma below holds
// even if a build drops the flag.
#include "tc_internal.h"
#include "../../include/threecrate_hip_color.h"

#include <cmath>

#pragma clang fp contract(off)

namespace tc {

constexpr int kColorTableChunk = 32;                            // sources per table launch: 32 x 88 bytes of kernel arguments
constexpr size_t kColorTableBytes = TC_COLOR_MAX_SOURCES * sizeof(tc_color_source);
constexpr size_t kColorHeadBytes = kColorTableBytes + sizeof(ColorOut);     // table | slices; the host road's outputs follow
static_assert(sizeof(tc_color_source) == 88 && kColorHeadBytes % 16 == 0, "");

struct ColorTableChunk { tc_color_source s[kColorTableChunk]; };

__global__ void __launch_bounds__(64) color_table_kernel(ColorTableChunk chunk, tc_color_source *__restrict__ table, uint32_t count) {
    if (threadIdx.x < count) table[threadIdx.x] = chunk.s[threadIdx.x];
}

__device__ __forceinline__ bool color_finite(float x) { return fabsf(x) < INFINITY; }      // false for a NaN

// COUNT: the caller wants colored_count.  Without it there is no barrier and no atomic
template <bool COUNT>
__global__ void __launch_bounds__(256) colorize_kernel(const float *__restrict__ xyz, uint32_t n, const tc_color_source *__restrict__ table,
                                                      uint32_t n_sources, tc_colorize_config cfg, uint8_t *__restrict__ rgb,
                                                      int32_t *__restrict__ source_index, uint32_t *__restrict__ slices) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    int32_t index = -1;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        uint8_t o0 = cfg.default_color[0], o1 = cfg.default_color[1], o2 = cfg.default_color[2];
        const uint32_t n_try = (color_finite(x) && color_finite(y) && color_finite(z)) ? n_sources : 0u;       // (1)
        for (uint32_t s = 0; s < n_try; ++s) {
            const tc_color_source &S = table[s];
            const float *m = S.world_to_camera;
            const float c_x = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];                                        // (2)
            const float c_y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
            const float c_z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
            if (!(c_z >= cfg.min_depth)) continue;                                                              // (3)
            const float u = (S.intrinsics.fx * c_x) / c_z + S.intrinsics.cx;                                    // (4)
            const float v = (S.intrinsics.fy * c_y) / c_z + S.intrinsics.cy;
            if (!color_finite(u) || !color_finite(v)) continue;                                                 // (5)
            const uint32_t w = S.intrinsics.width;
            const float fw = (float)w, fh = (float)S.intrinsics.height;                                         // exact: at most 65 536
            const float xn = roundf(u), yn = roundf(v);                                                         // (6)
            const bool inside_n = xn >= 0.0f && xn < fw && yn >= 0.0f && yn < fh;
            if (S.depth) {                                                                                      // (7)
                if (!inside_n) continue;
                const float d = S.depth[(size_t)(uint32_t)yn * w + (uint32_t)xn];
                if (!(color_finite(d) && d > 0.0f && fabsf(c_z - d) <= cfg.depth_tolerance)) continue;
            }
            uint8_t p0, p1, p2;
            const float xf = floorf(u), yf = floorf(v);                                                         // (8)
            if (cfg.interpolation == TC_COLOR_BILINEAR && xf >= 0.0f && yf >= 0.0f && xf + 1.0f < fw && yf + 1.0f < fh) {
                const float tx = u - xf, ty = v - yf;
                const uint8_t *r0 = S.rgb + 3 * ((size_t)(uint32_t)yf * w + (uint32_t)xf), *r1 = r0 + 3 * (size_t)w;
                uint8_t out[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float c00 = (float)r0[c], c10 = (float)r0[3 + c], c01 = (float)r1[c], c11 = (float)r1[3 + c];
                    const float top = c00 + (c10 - c00) * tx;
                    const float bot = c01 + (c11 - c01) * tx;
                    const float val = top + (bot - top) * ty;
                    out[c] = (uint8_t)(uint32_t)roundf(val);                                                    // val lies in [0, 255]
                }
                p0 = out[0]; p1 = out[1]; p2 = out[2];
            } else {
                if (!inside_n) continue;
                const uint8_t *r = S.rgb + 3 * ((size_t)(uint32_t)yn * w + (uint32_t)xn);
                p0 = r[0]; p1 = r[1]; p2 = r[2];
            }
            if (p0 == cfg.default_color[0] && p1 == cfg.default_color[1] && p2 == cfg.default_color[2]) continue;       // (9)
            o0 = p0; o1 = p1; o2 = p2; index = (int32_t)s;                                                      // (10)
            break;
        }
        if (rgb) { rgb[3 * (size_t)i] = o0; rgb[3 * (size_t)i + 1] = o1; rgb[3 * (size_t)i + 2] = o2; }
        if (source_index) source_index[i] = index;
    }
    if constexpr (COUNT) {
        const int total = __syncthreads_count(index >= 0 ? 1 : 0);
        if (threadIdx.x == 0 && total) atomicAdd(&slices[blockIdx.x % (uint32_t)kColorSlices], (uint32_t)total);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// validated arguments; the table's pointers, d_xyz, d_rgb and d_index are device pointers
static tc_status colorize_on_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                                    const tc_colorize_config *cfg, uint8_t *d_rgb, int32_t *d_index, size_t *colored_count) {
    hipStream_t st = ctx->stream;
    if (tc_status s = ensure(ctx, ctx->out_a, kColorHeadBytes)) return s;
    tc_color_source *table = (tc_color_source *)ctx->out_a.p;
    uint32_t *slices = (uint32_t *)((char *)ctx->out_a.p + kColorTableBytes);
    for (size_t base = 0; base < n_sources; base += kColorTableChunk) {
        ColorTableChunk chunk;
        const size_t count = n_sources - base < (size_t)kColorTableChunk ? n_sources - base : (size_t)kColorTableChunk;
        for (size_t k = 0; k < (size_t)kColorTableChunk; ++k) chunk.s[k] = sources[base + (k < count ? k : 0)];
        hipLaunchKernelGGL(color_table_kernel, dim3(1), dim3(64), 0, st, chunk, table + base, (uint32_t)count);
    }
    if (colored_count) TC_HIP_TRY(ctx, hipMemsetAsync(slices, 0, sizeof(ColorOut), st));
    {
        // a row per instantiation: every call launches exactly one of the two
        ProfScope ps(ctx, colored_count ? "colorize_counted" : "colorize");
        const dim3 grid((unsigned)((n + 255) / 256)), block(256);
        if (colored_count)
            hipLaunchKernelGGL(colorize_kernel<true>, grid, block, 0, st, d_xyz, (uint32_t)n, (const tc_color_source *)table, (uint32_t)n_sources, *cfg,
                               d_rgb, d_index, slices);
        else
            hipLaunchKernelGGL(colorize_kernel<false>, grid, block, 0, st, d_xyz, (uint32_t)n, (const tc_color_source *)table, (uint32_t)n_sources, *cfg,
                               d_rgb, d_index, slices);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (!colored_count) return TC_OK;
    ColorOut *h = &pinned_host(ctx)->color_out;
    if (tc_status s = read_back(ctx, h, slices, sizeof(ColorOut))) return s;
    size_t total = 0;
    for (uint32_t c : h->slice) total += c;
    *colored_count = total;
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_color.h) --------------------------------------------------------------------------
// the header's checks, in its order; *nothing: a valid call with no point
static tc_status color_check(tc_context *ctx, const float *xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                             const tc_colorize_config *cfg, uint8_t *rgb, int32_t *source_index, size_t *colored_count, bool *nothing) {
    *nothing = false;
    if (!ctx) return TC_INVALID_DATA;
    if (!xyz && n > 0) return fail(ctx, TC_INVALID_DATA, "colorize: xyz is NULL");
    if (!sources) return fail(ctx, TC_INVALID_DATA, "colorize: sources is NULL");
    if (!cfg) return fail(ctx, TC_INVALID_DATA, "colorize: config is NULL");
    for (size_t s = 0; s < n_sources; ++s)
        if (!sources[s].rgb) return fail(ctx, TC_INVALID_DATA, "colorize: source " + std::to_string(s) + ": rgb is NULL");
    if (!rgb && !source_index && !colored_count) return fail(ctx, TC_INVALID_DATA, "colorize: rgb, source_index and colored_count are all NULL");
    if (n_sources == 0) return fail(ctx, TC_INVALID_DATA, "colorize_from_images: sources slice must not be empty");     // colorization.rs:266-270
    if (n_sources > TC_COLOR_MAX_SOURCES) return fail(ctx, TC_UNSUPPORTED, "colorize: more than TC_COLOR_MAX_SOURCES (64) sources");
    if (cfg->interpolation > TC_COLOR_BILINEAR) return fail(ctx, TC_INVALID_DATA, "colorize: interpolation is neither nearest (0) nor bilinear (1)");
    if (!std::isfinite(cfg->min_depth) || !std::isfinite(cfg->depth_tolerance) || cfg->depth_tolerance < 0.0f)
        return fail(ctx, TC_INVALID_DATA, "colorize: min_depth and depth_tolerance must be finite, the tolerance not negative");
    for (size_t s = 0; s < n_sources; ++s) {
        const tc_camera_intrinsics &k = sources[s].intrinsics;
        bool finite = std::isfinite(k.fx) && std::isfinite(k.fy) && std::isfinite(k.cx) && std::isfinite(k.cy);
        for (float v : sources[s].world_to_camera) finite = finite && std::isfinite(v);
        if (!finite) return fail(ctx, TC_INVALID_DATA, "colorize: source " + std::to_string(s) + ": an intrinsic or matrix entry is not finite");
        if (k.width == 0 || k.height == 0) return fail(ctx, TC_INVALID_DATA, "colorize: source " + std::to_string(s) + ": width or height is zero");
        if (k.width > 65536u || k.height > 65536u)
            return fail(ctx, TC_UNSUPPORTED, "colorize: source " + std::to_string(s) + ": width or height is above 65536");
    }
    if (tc_status s = check_point_count(ctx, n)) return s;
    if (n == 0) {
        if (colored_count) *colored_count = 0;
        *nothing = true;
    }
    return TC_OK;
}

extern "C" {

void tc_colorize_config_default(tc_colorize_config *cfg) try {
    if (!cfg) return;
    cfg->default_color[0] = cfg->default_color[1] = cfg->default_color[2] = 128;
    cfg->interpolation = TC_COLOR_BILINEAR;
    cfg->min_depth = 1e-4f;
    cfg->depth_tolerance = 0.05f;
} TC_CATCH_VOID

tc_status tc_colorize_device(tc_context *ctx, const float *xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                             const tc_colorize_config *cfg, uint8_t *rgb, int32_t *source_index, size_t *colored_count) try {
    bool nothing;
    if (tc_status s = color_check(ctx, xyz, n, sources, n_sources, cfg, rgb, source_index, colored_count, &nothing)) return s;
    if (nothing) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return colorize_on_device(ctx, xyz, n, sources, n_sources, cfg, rgb, source_index, colored_count);
} TC_CATCH_STATUS(ctx)

tc_status tc_colorize(tc_context *ctx, const float *xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                      const tc_colorize_config *cfg, uint8_t *rgb, int32_t *source_index, size_t *colored_count) try {
    bool nothing;
    if (tc_status s = color_check(ctx, xyz, n, sources, n_sources, cfg, rgb, source_index, colored_count, &nothing)) return s;
    if (nothing) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the images one behind the other in in_b, the depth images in in_c, each at a 16-byte boundary
    auto pad16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    size_t b_images = 0, b_depths = 0;
    for (size_t s = 0; s < n_sources; ++s) {
        const size_t npix = (size_t)sources[s].intrinsics.width * sources[s].intrinsics.height;
        b_images += pad16(npix * 3);
        if (sources[s].depth) b_depths += pad16(npix * sizeof(float));
    }
    const size_t b_rgb = rgb ? pad16(n * 3) : 0, b_index = source_index ? n * sizeof(int32_t) : 0;
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, ctx->in_b, b_images)) return s;
    if (b_depths) if (tc_status s = ensure(ctx, ctx->in_c, b_depths)) return s;
    if (tc_status s = ensure(ctx, ctx->out_a, kColorHeadBytes + b_rgb + b_index)) return s;
    tc_color_source staged[TC_COLOR_MAX_SOURCES];
    size_t o_image = 0, o_depth = 0;
    for (size_t s = 0; s < n_sources; ++s) {
        const size_t npix = (size_t)sources[s].intrinsics.width * sources[s].intrinsics.height;
        staged[s] = sources[s];
        staged[s].rgb = (const uint8_t *)ctx->in_b.p + o_image;
        TC_HIP_TRY(ctx, hipMemcpyAsync((void *)staged[s].rgb, sources[s].rgb, npix * 3, hipMemcpyHostToDevice, st));
        o_image += pad16(npix * 3);
        if (sources[s].depth) {
            staged[s].depth = (const float *)((const char *)ctx->in_c.p + o_depth);
            TC_HIP_TRY(ctx, hipMemcpyAsync((void *)staged[s].depth, sources[s].depth, npix * sizeof(float), hipMemcpyHostToDevice, st));
            o_depth += pad16(npix * sizeof(float));
        }
    }
    uint8_t *d_rgb = rgb ? (uint8_t *)ctx->out_a.p + kColorHeadBytes : nullptr;
    int32_t *d_index = source_index ? (int32_t *)((char *)ctx->out_a.p + kColorHeadBytes + b_rgb) : nullptr;
    if (tc_status s = colorize_on_device(ctx, (const float *)ctx->in_a.p, n, staged, n_sources, cfg, d_rgb, d_index, colored_count)) return s;
    if (rgb) TC_HIP_TRY(ctx, hipMemcpyAsync(rgb, d_rgb, n * 3, hipMemcpyDeviceToHost, st));
    if (source_index) return stage_out(ctx, source_index, d_index, b_index);
    return synced(ctx);                                         // the caller's buffers are free
} TC_CATCH_STATUS(ctx)

}  // extern "C"
