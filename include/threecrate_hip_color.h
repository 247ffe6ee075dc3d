/* threecrate_hip_color.h -- companion surface: colour a point cloud from registered camera images (colorize_point_cloud,
 * colorize_from_images, threecrate-algorithms/src/colorization.rs:203-331; the wheel's colorize_point_cloud).  Every point is
 * projected into the cameras in the caller's order and takes the colour of the first one that sees it.
 *
 * The symbols live in a library of their own, libthreecrate_hip_color.so, which is linked against libthreecrate_hip.so (it sits
 * in the same directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by
 * tc_context_create serves both.  tc_abi_version() is unchanged.  A consumer links both libraries.  The TSDF header is included
 * for tc_camera_intrinsics and the 3 x 4 world_to_camera convention alone: no TSDF function is called.
 *
 * ---- the contract, in the order of operations; every result is bit for bit ----
 * All arithmetic is f32, one rounding per operation (no contraction), IEEE division; roundf is half away from zero.
 * For point p = (x, y, z) and the sources s = 0, 1, ... in order:
 *    1. a coordinate of p that is not finite: the default colour and index -1; the point ends here
 *    2. c_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3]
 *    3. skip the source unless c_z >= min_depth (a NaN fails)
 *    4. u = (fx c_x) / c_z + cx, v = (fy c_y) / c_z + cy
 *    5. skip unless u and v are finite
 *    6. xn = roundf(u), yn = roundf(v); inside_n = 0 <= xn < f32(width) and 0 <= yn < f32(height)
 *    7. with depth != NULL: skip unless inside_n; d = depth[yn width + xn]; skip unless d is finite, d > 0 and
 *       |c_z - d| <= depth_tolerance
 *    8. sample.  Bilinear mode: xf = floorf(u), yf = floorf(v); if xf >= 0, yf >= 0, xf + 1 < f32(width) and
 *       yf + 1 < f32(height): tx = u - xf, ty = v - yf and per channel, with c00, c10, c01, c11 = f32(byte) of the pixels
 *       (xf, yf), (xf + 1, yf), (xf, yf + 1), (xf + 1, yf + 1):
 *           top = c00 + (c10 - c00) tx;  bot = c01 + (c11 - c01) tx;  val = top + (bot - top) ty;  out = (uint8)roundf(val)
 *       Otherwise, and in nearest mode: skip unless inside_n; out = pixel (xn, yn)
 *    9. out equal to default_color in all three channels: skip the source.  This is the reference's rule (hit = color !=
 *       default_color, and colorize_from_images falls through to the next image): A PIXEL OF THE DEFAULT COLOUR COLOURS NOTHING
 *   10. otherwise write out and index s; the point ends here
 *   11. no source left: the default colour and index -1
 * colored_count is the number of points with index >= 0.
 * Deviations from colorization.rs:
 *   - a NaN u or v, or a point that is not finite, samples pixel (0, 0) in the reference (Rust's `as i32` maps NaN to 0) and in
 *     bilinear mode writes (0, 0, 0).  Here such points are skipped (1, 5).
 *   - x0 + 1 overflows in the reference for u >= 2^31; here the comparison is made in floats (8).
 *   - Isometry3 * point (the quaternion form) becomes the 3 x 4 product of (2): the caller supplies the twelve floats, as for TSDF.
 *   - the depth test (7) is an addition.  With depth == NULL the result is the reference's. */
#ifndef THREECRATE_HIP_COLOR_H
#define THREECRATE_HIP_COLOR_H

#include "threecrate_hip.h"
#include "threecrate_hip_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_COLOR_NEAREST  0u
#define TC_COLOR_BILINEAR 1u
#define TC_COLOR_MAX_SOURCES 64

typedef struct tc_color_source {        /* one (RgbImageView, CameraIntrinsics, Isometry3) of colorize_from_images, + a depth image */
    const uint8_t *rgb;                 /* height x width x 3, row-major, tightly packed */
    const float   *depth;               /* height x width f32 metres, or NULL: no occlusion test */
    tc_camera_intrinsics intrinsics;    /* fx fy cx cy width height */
    float world_to_camera[12];          /* 3 x 4 row-major, the TSDF header's convention */
} tc_color_source;

typedef struct tc_colorize_config {     /* ColorizationConfig, colorization.rs:143-153, + the tolerance of the depth test */
    uint8_t default_color[3];
    uint8_t interpolation;              /* TC_COLOR_NEAREST | TC_COLOR_BILINEAR */
    float   min_depth;
    float   depth_tolerance;            /* read only by sources with depth != NULL */
} tc_colorize_config;

/* {128, 128, 128}, bilinear, 1e-4f, 0.05f (ColorizationConfig::default, :155-163).  NULL is allowed. */
void tc_colorize_config_default(tc_colorize_config *cfg);

/* Colour n points (xyz: n x 3 floats) from n_sources cameras.
 *   rgb            n x 3 uint8, or NULL
 *   source_index   n int32: the source that coloured the point, -1 for none; or NULL
 *   colored_count  points with index >= 0; or NULL
 * Checks, in this order:
 *   1. a NULL context; a NULL xyz with n > 0; NULL sources or cfg; a source whose rgb is NULL; rgb, source_index and
 *      colored_count all NULL: TC_INVALID_DATA
 *   2. n_sources == 0: TC_INVALID_DATA ("sources slice must not be empty", :266-270)
 *   3. n_sources > TC_COLOR_MAX_SOURCES: TC_UNSUPPORTED
 *   4. interpolation > 1: TC_INVALID_DATA
 *   5. min_depth or depth_tolerance not finite, or a negative tolerance: TC_INVALID_DATA
 *   6. per source, in index order: an intrinsic or matrix entry that is not finite, a zero width or height: TC_INVALID_DATA with a
 *      message; a width or height above 65 536: TC_UNSUPPORTED
 *   7. n >= 2^32 - 16: TC_UNSUPPORTED
 * n == 0 is then TC_OK with a count of 0.  A call that fails writes nothing.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for xyz, every
 * sources[s].rgb and .depth, rgb and source_index (sources, cfg and colored_count are host pointers in both) and, with
 * colored_count == NULL, only enqueues on the context's stream. */
tc_status tc_colorize(tc_context *ctx, const float *xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                      const tc_colorize_config *cfg, uint8_t *rgb, int32_t *source_index, size_t *colored_count);
tc_status tc_colorize_device(tc_context *ctx, const float *xyz, size_t n, const tc_color_source *sources, size_t n_sources,
                             const tc_colorize_config *cfg, uint8_t *rgb, int32_t *source_index, size_t *colored_count);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_COLOR_H */
