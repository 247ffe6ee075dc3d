/* abi_ground.c -- a COMPILED consumer of include/threecrate_hip_ground.h (test infrastructure), the companion of abi_alpha.c for the
 * surface of libthreecrate_hip_ground.so: prints sizeof of its structs, offsetof and size of every field, one `name value` pair per line;
 * tests/test_abi_ground.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)] structs of bindings/rust
 * (ffi_ground.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_ground.c -Lthreecrate_amd -lthreecrate_hip_ground -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_ground.h"

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
    void (*defaults)(float, tc_ground_config *) = tc_ground_config_default;
    size_t (*count)(const tc_ground_config *) = tc_ground_patch_count;
    tc_status (*segment[2])(tc_context *, const float *, size_t, const tc_ground_config *, uint8_t *, uint32_t *, uint32_t *, tc_ground_patch *,
                            size_t *) = {tc_segment_ground, tc_segment_ground_device};
    printf("count.exports %d\n", (defaults != 0) + (count != 0) + (segment[0] != 0) + (segment[1] != 0));

    SZ(tc_ground_config); ALIGN(tc_ground_config);
    OFF(tc_ground_config, sensor_height); OFF(tc_ground_config, n_zones); OFF(tc_ground_config, zone_radii); OFF(tc_ground_config, num_rings);
    OFF(tc_ground_config, num_sectors); OFF(tc_ground_config, max_range); OFF(tc_ground_config, min_points_per_patch);
    OFF(tc_ground_config, num_seed_points); OFF(tc_ground_config, seed_selection_threshold); OFF(tc_ground_config, dist_threshold);
    OFF(tc_ground_config, num_iterations); OFF(tc_ground_config, uprightness_threshold); OFF(tc_ground_config, flatness_threshold);
    OFF(tc_ground_config, elevation_threshold);
    SZ(tc_ground_patch); ALIGN(tc_ground_patch);
    OFF(tc_ground_patch, count); OFF(tc_ground_patch, n_inliers); OFF(tc_ground_patch, status); OFF(tc_ground_patch, normal); OFF(tc_ground_patch, d);
    OFF(tc_ground_patch, mean_z); OFF(tc_ground_patch, flatness);
    VAL(TC_INVALID_DATA); VAL(TC_GROUND_MAX_ZONES);
    VAL(TC_GROUND_PATCH_EMPTY); VAL(TC_GROUND_PATCH_TOO_FEW_POINTS); VAL(TC_GROUND_PATCH_TOO_FEW_SEEDS); VAL(TC_GROUND_PATCH_TOO_FEW_INLIERS);
    VAL(TC_GROUND_PATCH_NO_ITERATION); VAL(TC_GROUND_PATCH_NOT_UPRIGHT); VAL(TC_GROUND_PATCH_ELEVATION); VAL(TC_GROUND_PATCH_NOT_FLAT);
    VAL(TC_GROUND_PATCH_GROUND);
    /* the defaults */
    tc_ground_config cfg;
    defaults(1.5f, &cfg);
    defaults(1.5f, NULL);
    printf("default.n_zones %u\ndefault.height_ok %d\ndefault.patches %zu\ndefault.null_patches %zu\n", (unsigned)cfg.n_zones, (int)(cfg.sensor_height == 1.5f),
           count(&cfg), count(NULL));
    printf("default.radii_ok %d\n", (int)(cfg.zone_radii[0] == 0.0f && cfg.zone_radii[1] == 2.7f && cfg.zone_radii[2] == 12.3625f && cfg.zone_radii[3] == 22.025f &&
                                          cfg.zone_radii[4] == 80.0f && cfg.max_range == 80.0f));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float points[6] = {5, 1, -1.5f, 5, 2, -1.5f};
    uint8_t labels[2] = {7, 7};
    size_t n_ground = 7;
    printf("call.segment_null %d\n", (int)segment[0](NULL, points, 2, &cfg, labels, NULL, NULL, NULL, &n_ground));
    printf("call.segment_device_null %d\n", (int)segment[1](NULL, points, 2, &cfg, labels, NULL, NULL, NULL, &n_ground));
    printf("call.null_wrote %d\n", (int)(labels[0] != 7 || labels[1] != 7 || n_ground != 7));
    return 0;
}
