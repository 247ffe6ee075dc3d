/* abi_alpha.c -- a COMPILED consumer of include/threecrate_hip_alpha.h (test infrastructure), the companion of abi_qem.c for the
 * surface of libthreecrate_hip_alpha.so: prints sizeof of its structs, offsetof and size of every field, one `name value` pair per line;
 * tests/test_abi_alpha.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)] structs of bindings/rust
 * (ffi_alpha.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_alpha.c -Lthreecrate_amd -lthreecrate_hip_alpha -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_alpha.h"

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
    void (*defaults)(float, tc_alpha_config *) = tc_alpha_config_default;
    tc_status (*shape[2])(tc_context *, const float *, size_t, const tc_alpha_config *, uint32_t *, size_t, tc_alpha_stats *) = {tc_alpha_shape,
                                                                                                                                 tc_alpha_shape_device};
    printf("count.exports %d\n", (defaults != 0) + (shape[0] != 0) + (shape[1] != 0));

    SZ(tc_alpha_config); ALIGN(tc_alpha_config);
    OFF(tc_alpha_config, alpha); OFF(tc_alpha_config, mode); OFF(tc_alpha_config, min_triangle_area); OFF(tc_alpha_config, max_triangles);
    SZ(tc_alpha_stats); ALIGN(tc_alpha_stats);
    OFF(tc_alpha_stats, candidates); OFF(tc_alpha_stats, boundary_candidates); OFF(tc_alpha_stats, faces); OFF(tc_alpha_stats, capped);
    VAL(TC_INVALID_DATA); VAL(TC_ALPHA_BOUNDARY_ONLY); VAL(TC_ALPHA_FULL);
    /* the defaults */
    tc_alpha_config cfg = {9.0f, 9, 9.0f, 9};
    defaults(0.25f, &cfg);
    defaults(0.25f, NULL);
    printf("default.mode %u\ndefault.alpha_ok %d\ndefault.area_ok %d\ndefault.max_triangles %u\n", (unsigned)cfg.mode, (int)(cfg.alpha == 0.25f),
           (int)(cfg.min_triangle_area == 1e-8f), (unsigned)cfg.max_triangles);
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float points[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
    uint32_t out_faces[3] = {7, 7, 7};
    tc_alpha_stats stats = {7, 7, 7, 7};
    printf("call.shape_null %d\n", (int)shape[0](NULL, points, 3, &cfg, out_faces, 1, &stats));
    printf("call.shape_device_null %d\n", (int)shape[1](NULL, points, 3, &cfg, out_faces, 1, &stats));
    printf("call.null_wrote %d\n", (int)(out_faces[0] != 7 || out_faces[2] != 7 || stats.candidates != 7 || stats.boundary_candidates != 7 || stats.faces != 7 ||
                                        stats.capped != 7));
    return 0;
}
