/* abi_qem.c -- a COMPILED consumer of include/threecrate_hip_qem.h (test infrastructure), the companion of abi_simplify.c for the
 * surface of libthreecrate_hip_qem.so: prints sizeof of its struct, offsetof and size of every field, one `name value` pair per line;
 * tests/test_abi_qem.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)] struct of bindings/rust
 * (ffi_qem.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_qem.c -Lthreecrate_amd -lthreecrate_hip_qem -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_qem.h"

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
    void (*defaults)(float, tc_qem_config *) = tc_qem_config_default;
    tc_status (*simplify[2])(tc_context *, const float *, size_t, const uint32_t *, size_t, const tc_qem_config *, float *, size_t, uint32_t *, size_t,
                             uint32_t *, size_t *, size_t *, uint32_t *) = {tc_simplify_quadric, tc_simplify_quadric_device};
    printf("count.exports %d\n", (defaults != 0) + (simplify[0] != 0) + (simplify[1] != 0));

    SZ(tc_qem_config); ALIGN(tc_qem_config);
    OFF(tc_qem_config, reduction_ratio); OFF(tc_qem_config, preserve_boundary); OFF(tc_qem_config, max_edge_length);
    VAL(TC_INVALID_DATA);
    /* the defaults */
    tc_qem_config cfg = {9.0f, 9, 9.0f};
    defaults(0.25f, &cfg);
    defaults(0.25f, NULL);
    printf("default.preserve_boundary %u\ndefault.ratio_ok %d\ndefault.no_limit %d\n", (unsigned)cfg.preserve_boundary, (int)(cfg.reduction_ratio == 0.25f),
           (int)(cfg.max_edge_length == 0.0f));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float vertices[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, out[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
    uint32_t faces[3] = {0, 1, 2}, out_faces[3] = {7, 7, 7}, map[3] = {7, 7, 7}, rounds = 7;
    size_t nv = 7, nf = 7;
    printf("call.simplify_null %d\n", (int)simplify[0](NULL, vertices, 3, faces, 1, &cfg, out, 3, out_faces, 1, map, &nv, &nf, &rounds));
    printf("call.simplify_device_null %d\n", (int)simplify[1](NULL, vertices, 3, faces, 1, &cfg, out, 3, out_faces, 1, map, &nv, &nf, &rounds));
    printf("call.null_wrote %d\n", (int)(out[0] != 7 || out[8] != 7 || out_faces[0] != 7 || map[0] != 7 || nv != 7 || nf != 7 || rounds != 7));
    return 0;
}
