/* threecrate_hip_tsdf.h -- extension surface of libthreecrate_hip.so: TSDF depth fusion and surface extraction.
 *
 * The symbols live in the same shared library as those of threecrate_hip.h and use its status and context types;
 * tc_abi_version() is unchanged.  They are declared apart so that the main header and the other extension headers keep the sets
 * of names they have. */
#ifndef THREECRATE_HIP_TSDF_H
#define THREECRATE_HIP_TSDF_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the volume ----
 * TsdfVolume / TsdfVolumeGpu (threecrate-gpu/src/tsdf.rs:24-37, :549-803), the kernels tsdf_integration.wgsl and
 * surface_extraction.wgsl.  A handle owns a dense volume in device memory that integrate updates in place and extract_surface
 * reads in place: the reference recompiles its shader on every call, keeps 32 bytes per voxel and carries the whole volume through
 * the host for every extraction.
 *
 * Voxel (x, y, z) has the index (z ry + y) rx + x.  Initial state: tsdf = 1.0, weight = 0, colour (0, 0, 0).
 * Device state: 8 bytes per voxel, { float tsdf; uint32_t weight << 24 | r << 16 | g << 8 | b }.  The reference's weights are whole
 * numbers (0, + 1, min with the cap) and its colours 0..255, so nothing is lost against its 32-byte record.
 *
 *   voxel_size, truncation_distance   > 0 and finite
 *   resolution                        each >= 1; a product above 2^28 is TC_UNSUPPORTED (12 points per cube must fit a 32-bit scan)
 *   origin                            finite: the position of voxel (0, 0, 0); f32(resolution_k) voxel_size + |origin_k| is finite too
 *                                     (every voxel has a finite position)
 *   max_weight                        1..255 (the reference hard-codes 100.0)
 * All arithmetic is f32, one rounding per operation (no contraction), IEEE division. */
typedef struct tc_tsdf_volume tc_tsdf_volume;

typedef struct tc_tsdf_volume_config {      /* TsdfVolume, tsdf.rs:24-29, + the cap of the weight */
    float    voxel_size;
    float    truncation_distance;
    uint32_t resolution[3];
    float    origin[3];
    uint32_t max_weight;
} tc_tsdf_volume_config;

typedef struct tc_camera_intrinsics {       /* CameraIntrinsics, tsdf.rs:41-50, without depth_scale (its shader never reads it) */
    float    fx;
    float    fy;
    float    cx;
    float    cy;
    uint32_t width;
    uint32_t height;
} tc_camera_intrinsics;

/* extract_surface flags */
#define TC_TSDF_OBSERVED_EDGES 1u           /* an edge emits only when both of its ends have weight > 0 */

/* NULL context, config or out: TC_INVALID_DATA.  A size that is not finite or <= 0, a zero resolution, an origin that is not finite, a
 * far corner that is not finite, max_weight outside 1..255: TC_INVALID_DATA with a message.  The volume starts in the initial state. */
tc_status tc_tsdf_volume_create(tc_context *ctx, const tc_tsdf_volume_config *cfg, tc_tsdf_volume **out);
void tc_tsdf_volume_destroy(tc_tsdf_volume *vol);
/* back to the initial state */
tc_status tc_tsdf_volume_reset(tc_tsdf_volume *vol);

/* ---- integrate ----
 *   depth            height x width f32, row-major, metres
 *   rgb              height x width x 3 uint8, or NULL
 *   world_to_camera  3 x 4, row-major: the matrix the kernel multiplies by (inverting a camera pose is the caller's job, so that
 *                    every implementation sees the same twelve floats)
 *   n_updated        voxels that were updated, or NULL
 * For every voxel (x, y, z):
 *    1. w_k = f32(i_k) voxel_size + origin_k
 *    2. c_i = ((m[i][0] w_x + m[i][1] w_y) + m[i][2] w_z) + m[i][3]
 *    3. skip unless c_z > 0
 *    4. a = ((c_x / c_z) fx + cx) + 0.5, b likewise with c_y, fy, cy
 *    5. skip unless 0 <= a < f32(width) and 0 <= b < f32(height) (a NaN fails)
 *    6. u = (uint32)a, v = (uint32)b, d = depth[v width + u]
 *    7. skip unless d > 0 and d is finite
 *    8. t = min(max(d - c_z, -truncation), truncation)
 *    9. w' = min(w + 1, max_weight)
 *   10. alpha = 1.0f / f32(w')
 *   11. tsdf' = (1.0f - alpha) tsdf + alpha t
 *   12. colour, only with rgb and a pixel whose r, g, b are not all zero, per channel:
 *       c' = (uint32)min(max((1.0f - alpha) f32(c) + alpha f32(pixel), 0.0f), 255.0f)
 * Deviations from tsdf_integration.wgsl and its host code:
 *   - the shader converts a negative or NaN pixel coordinate with u32(), which clamps to 0 or is indeterminate: every voxel left of
 *     or above the frustum is fused with pixel column or row 0.  Here such voxels are skipped (5).
 *   - the shader does not test c_z; here voxels at or behind the camera plane are skipped (3).
 *   - the shader lets a NaN depth through; here it is skipped, as is an infinite one (7).
 *   - the host code writes the rows of the inverse pose into a column-major mat4x4, i.e. uploads it transposed: right only for the
 *     identity, the one pose the reference tests.  Here the product is the intended W2C p.
 *   - depth_scale of CameraIntrinsics is never read by the shader: it is not part of the struct.
 *   - TsdfVolumeGpu::integrate hands raw RGB bytes to a shader that expects one packed word per pixel; tsdf_integrate packs them.
 *     The meaning here is tsdf_integrate's: the pixel's own r, g, b.
 * NULL volume: TC_INVALID_DATA.  NULL depth, intrinsics or matrix, an intrinsic or matrix entry that is not finite, a zero width
 * or height: TC_INVALID_DATA with a message; width x height of 2^31 or more: TC_UNSUPPORTED.
 * The host variant returns with the caller's buffers free.  The _device variant takes device pointers for depth and rgb
 * (intrinsics, matrix and n_updated are host pointers in both) and, with n_updated == NULL, only enqueues on the context's stream. */
tc_status tc_tsdf_integrate(tc_tsdf_volume *vol, const float *depth, const uint8_t *rgb, const tc_camera_intrinsics *intrinsics,
                            const float world_to_camera[12], size_t *n_updated);
tc_status tc_tsdf_integrate_device(tc_tsdf_volume *vol, const float *d_depth, const uint8_t *d_rgb, const tc_camera_intrinsics *intrinsics,
                                   const float world_to_camera[12], size_t *n_updated);

/* ---- the state as arrays ----
 * tsdf: one f32 per voxel; weight: one uint8; rgb: three uint8; all in voxel index order.
 * download: any of the three may be NULL.  upload: tsdf and weight are required, rgb NULL means zeros; the host variant answers a
 * weight above max_weight with TC_INVALID_DATA and leaves the volume as it was, the _device variant trusts the caller (a larger
 * weight is stored as it is and the next integrate caps it).  The _device variants take device pointers and are complete when
 * they return. */
tc_status tc_tsdf_volume_download(tc_tsdf_volume *vol, float *tsdf, uint8_t *weight, uint8_t *rgb);
tc_status tc_tsdf_volume_download_device(tc_tsdf_volume *vol, float *d_tsdf, uint8_t *d_weight, uint8_t *d_rgb);
tc_status tc_tsdf_volume_upload(tc_tsdf_volume *vol, const float *tsdf, const uint8_t *weight, const uint8_t *rgb);
tc_status tc_tsdf_volume_upload_device(tc_tsdf_volume *vol, const float *d_tsdf, const uint8_t *d_weight, const uint8_t *d_rgb);

/* ---- extract_surface ----
 * surface_extraction.wgsl: a cube has its base voxel at x < rx - 1, y < ry - 1, z < rz - 1; a cube whose base voxel has weight 0
 * emits nothing.  Corner value: tsdf - iso_value with weight > 0, else + truncation (not truncation - iso_value).  The 12 edges in
 * the shader's order, corners written xyz: 000-100 010-110 001-101 011-111 (along x), 000-010 100-110 001-011 101-111 (along y),
 * 000-001 100-101 010-011 110-111 (along z).  An edge with corner values va, vb emits one point when the f32 product va vb <= 0:
 *   pa_k = origin_k + f32(i_k) voxel_size;  |va - vb| < 1e-5: 0.5 (pa + pb);  else pa + min(max(va / (va - vb), 0), 1) (pb - pa)
 * with the base voxel's colour.  flags: TC_TSDF_OBSERVED_EDGES -- an edge additionally needs weight > 0 at both ends (without it
 * an unobserved voxel beside an observed one behind the surface reads as + truncation and leaves a sheet of points along the
 * frustum's boundary); any other bit is TC_INVALID_DATA.
 * The output is the shader's multiset -- an interior edge is emitted by up to four cubes -- in a fixed order: cubes by ascending
 * index of their base voxel, edges in the order above.  There is no cap (the reference drops what exceeds min(voxels, 10^6) points).
 *   xyz, rgb    n x 3 f32, n x 3 uint8; either may be NULL
 *   capacity    points each non-NULL array has room for
 *   n_points    always written.  xyz == NULL and rgb == NULL is the count call: TC_OK.  Otherwise capacity < n returns
 *               TC_INVALID_DATA ("capacity is smaller than the number of points") without writing an array.
 * NULL volume or n_points: TC_INVALID_DATA; an iso_value that is not finite: TC_INVALID_DATA.
 * The _device variant takes device pointers for xyz and rgb; n_points is a host pointer; it is complete when it returns. */
tc_status tc_tsdf_extract_surface(tc_tsdf_volume *vol, float iso_value, uint32_t flags, float *xyz, uint8_t *rgb, size_t capacity,
                                  size_t *n_points);
tc_status tc_tsdf_extract_surface_device(tc_tsdf_volume *vol, float iso_value, uint32_t flags, float *d_xyz, uint8_t *d_rgb, size_t capacity,
                                         size_t *n_points);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_TSDF_H */
