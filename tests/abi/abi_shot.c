/* abi_shot.c -- a COMPILED consumer of include/threecrate_hip_shot.h (test infrastructure), the companion of abi_ground.c for the
 * surface of libthreecrate_hip_shot.so: prints sizeof of its struct, offsetof and size of every field, one `name value` pair per line;
 * tests/test_abi_shot.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)] struct of bindings/rust
 * (ffi_shot.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_shot.c -Lthreecrate_amd -lthreecrate_hip_shot -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_shot.h"

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
    void (*defaults)(tc_shot_config *) = tc_shot_config_default;
    size_t (*dim)(int) = tc_shot_dim;
    tc_status (*extract[2])(tc_context *, const float *, size_t, const tc_shot_config *, float *, float *, uint32_t *) = {
        tc_extract_shot_features_with_normals, tc_extract_shot_features_with_normals_device};
    printf("count.exports %d\n", (defaults != 0) + (dim != 0) + (extract[0] != 0) + (extract[1] != 0));

    SZ(tc_shot_config); ALIGN(tc_shot_config);
    OFF(tc_shot_config, search_radius); OFF(tc_shot_config, k_neighbors); OFF(tc_shot_config, variant);
    VAL(TC_INVALID_DATA); VAL(TC_SHOT_DIM); VAL(TC_USC_DIM); VAL(TC_SHOT_VARIANT_SHOT); VAL(TC_SHOT_VARIANT_USC);
    VAL(TC_SHOT_ROAD_BALL); VAL(TC_SHOT_ROAD_FALLBACK); VAL(TC_SHOT_ROAD_INERT); VAL(TC_SHOT_ROAD_MASK); VAL(TC_SHOT_X_TIE); VAL(TC_SHOT_ZERO_COV);
    VAL(TC_SHOT_EMPTY);
    /* the defaults and the row lengths */
    tc_shot_config cfg;
    defaults(&cfg);
    defaults(NULL);
    printf("default.radius_ok %d\ndefault.k %zu\ndefault.variant %d\n", (int)(cfg.search_radius == 0.2f), cfg.k_neighbors, cfg.variant);
    printf("dim.shot %zu\ndim.usc %zu\ndim.other %zu\ndim.negative %zu\n", dim(0), dim(1), dim(2), dim(-1));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float points[12] = {0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 1};
    float out[4] = {7, 7, 7, 7};
    uint32_t flags[2] = {7, 7};
    printf("call.extract_null %d\n", (int)extract[0](NULL, points, 2, &cfg, out, NULL, flags));
    printf("call.extract_device_null %d\n", (int)extract[1](NULL, points, 2, &cfg, out, NULL, flags));
    printf("call.null_wrote %d\n", (int)(out[0] != 7 || out[3] != 7 || flags[0] != 7 || flags[1] != 7));
    return 0;
}
