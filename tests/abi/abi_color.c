/* abi_color.c -- a COMPILED consumer of include/threecrate_hip_color.h (test infrastructure), the companion of abi_voxelmap.c for the
 * surface of libthreecrate_hip_color.so: prints sizeof of its structs, offsetof and size of every field and the values of its constants,
 * one `name value` pair per line; tests/test_abi_color.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the
 * #[repr(C)] structs of bindings/rust (ffi_color.rs).  It takes the address of every export, so it links only against a library that
 * has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_color.c -Lthreecrate_amd -lthreecrate_hip_color -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_color.h"

#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf("offsetof." #T "." #f " %zu\nfieldsize." #T "." #f " %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
#define VAL(c) printf("const." #c " %lld\n", (long long)(c))
#ifdef __cplusplus
#define ALIGN(T) printf("alignof." #T " %zu\n", (size_t)alignof(T))
#else
#define ALIGN(T) printf("alignof." #T " %zu\n", (size_t)_Alignof(T))
#endif

int main(void) {
    /* the prototypes as a caller spells them: a mismatch with the header is a compile error */
    void (*defaults)(tc_colorize_config *) = tc_colorize_config_default;
    tc_status (*colorize[2])(tc_context *, const float *, size_t, const tc_color_source *, size_t, const tc_colorize_config *, uint8_t *, int32_t *,
                             size_t *) = {tc_colorize, tc_colorize_device};
    printf("count.exports %d\n", (defaults != 0) + (colorize[0] != 0) + (colorize[1] != 0));

    SZ(tc_color_source); ALIGN(tc_color_source);
    OFF(tc_color_source, rgb); OFF(tc_color_source, depth); OFF(tc_color_source, intrinsics); OFF(tc_color_source, world_to_camera);
    SZ(tc_colorize_config); ALIGN(tc_colorize_config);
    OFF(tc_colorize_config, default_color); OFF(tc_colorize_config, interpolation); OFF(tc_colorize_config, min_depth);
    OFF(tc_colorize_config, depth_tolerance);
    SZ(tc_camera_intrinsics);
    VAL(TC_COLOR_NEAREST);
    VAL(TC_COLOR_BILINEAR);
    VAL(TC_COLOR_MAX_SOURCES);
    VAL(TC_INVALID_DATA);
    /* the defaults */
    tc_colorize_config cfg = {{0, 0, 0}, 0, 0.0f, 0.0f};
    defaults(&cfg);
    defaults(NULL);
    printf("default.color %d\ndefault.interpolation %d\n", cfg.default_color[0] * 65536 + cfg.default_color[1] * 256 + cfg.default_color[2],
           (int)cfg.interpolation);
    printf("default.min_depth_ok %d\ndefault.depth_tolerance_ok %d\n", (int)(cfg.min_depth == 1e-4f), (int)(cfg.depth_tolerance == 0.05f));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float xyz[3] = {0.0f, 0.0f, 1.0f};
    uint8_t image[3] = {1, 2, 3}, rgb[3] = {7, 7, 7};
    int32_t index = 7;
    size_t count = 7;
    tc_color_source src = {image, NULL, {1.0f, 1.0f, 0.0f, 0.0f, 1, 1}, {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
    printf("call.colorize_null %d\n", (int)colorize[0](NULL, xyz, 1, &src, 1, &cfg, rgb, &index, &count));
    printf("call.colorize_device_null %d\n", (int)colorize[1](NULL, xyz, 1, &src, 1, &cfg, rgb, &index, &count));
    printf("call.null_wrote %d\n", (int)(rgb[0] != 7 || index != 7 || count != 7));
    return 0;
}
