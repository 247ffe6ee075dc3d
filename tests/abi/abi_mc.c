/* abi_mc.c -- a COMPILED consumer of include/threecrate_hip_mc.h (test infrastructure), the companion of abi_simplify.c for the surface
 * of libthreecrate_hip_mc.so: prints sizeof of its structs, offsetof and size of every field and the values of its constants, one
 * `name value` pair per line; tests/test_abi_mc.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)]
 * structs of bindings/rust (ffi_mc.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_mc.c -Lthreecrate_amd -lthreecrate_hip_mc -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_mc.h"

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
    void (*defaults)(tc_mc_config *) = tc_mc_config_default;
    tc_status (*mc[2])(tc_context *, const tc_mc_grid *, const float *, const uint8_t *, const tc_mc_config *, float *, float *, uint32_t *, size_t, size_t,
                       size_t *, size_t *) = {tc_marching_cubes, tc_marching_cubes_device};
    printf("count.exports %d\n", (defaults != 0) + (mc[0] != 0) + (mc[1] != 0));

    SZ(tc_mc_grid); ALIGN(tc_mc_grid);
    OFF(tc_mc_grid, dims); OFF(tc_mc_grid, voxel_size); OFF(tc_mc_grid, origin); OFF(tc_mc_grid, layout);
    SZ(tc_mc_config); ALIGN(tc_mc_config);
    OFF(tc_mc_config, iso_level); OFF(tc_mc_config, flags);
    VAL(TC_MC_Z_FASTEST); VAL(TC_MC_X_FASTEST); VAL(TC_MC_NORMALS); VAL(TC_MC_WELD);
    VAL(TC_INVALID_DATA);
    /* the defaults */
    tc_mc_config cfg = {9.0f, 9};
    defaults(&cfg);
    defaults(NULL);
    printf("default.iso_is_zero %d\ndefault.flags %u\n", (int)(cfg.iso_level == 0.0f), (unsigned)cfg.flags);
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    tc_mc_grid grid = {{2, 2, 2}, {1.0f, 1.0f, 1.0f}, {0.0f, 0.0f, 0.0f}, TC_MC_Z_FASTEST};
    float values[8] = {-1, 1, 1, 1, 1, 1, 1, 1}, v[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7}, n[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
    uint32_t f[3] = {7, 7, 7};
    size_t nv = 7, nf = 7;
    printf("call.mc_null %d\n", (int)mc[0](NULL, &grid, values, NULL, &cfg, v, n, f, 3, 1, &nv, &nf));
    printf("call.mc_device_null %d\n", (int)mc[1](NULL, &grid, values, NULL, &cfg, v, n, f, 3, 1, &nv, &nf));
    printf("call.null_wrote %d\n", (int)(v[0] != 7 || v[8] != 7 || n[0] != 7 || f[0] != 7 || nv != 7 || nf != 7));
    return 0;
}
