/* abi_poisson.c -- a COMPILED consumer of include/threecrate_hip_poisson.h (test infrastructure), the companion of abi_shot.c for the
 * surface of libthreecrate_hip_poisson.so: prints sizeof of its structs, offsetof and size of every field, one `name value` pair per line;
 * tests/test_abi_poisson.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the #[repr(C)] structs of bindings/rust
 * (ffi_poisson.rs).  It takes the address of every export, so it links only against a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_poisson.c -Lthreecrate_amd -lthreecrate_hip_poisson -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_poisson.h"

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
    void (*defaults)(tc_poisson_config *) = tc_poisson_config_default;
    tc_status (*field[2])(tc_context *, const float *, const float *, size_t, const tc_poisson_config *, tc_mc_grid *, float *, float *, tc_poisson_stats *) = {
        tc_poisson_field, tc_poisson_field_device};
    tc_status (*recon[2])(tc_context *, const float *, const float *, size_t, const tc_poisson_config *, float *, uint32_t *, size_t, size_t, size_t *,
                          size_t *, tc_poisson_stats *) = {tc_poisson_reconstruct, tc_poisson_reconstruct_device};
    printf("count.exports %d\n", (defaults != 0) + (field[0] != 0) + (field[1] != 0) + (recon[0] != 0) + (recon[1] != 0));

    SZ(tc_poisson_config); ALIGN(tc_poisson_config);
    OFF(tc_poisson_config, depth); OFF(tc_poisson_config, scale); OFF(tc_poisson_config, point_weight); OFF(tc_poisson_config, max_iterations);
    OFF(tc_poisson_config, tolerance); OFF(tc_poisson_config, min_density);
    SZ(tc_poisson_stats); ALIGN(tc_poisson_stats);
    OFF(tc_poisson_stats, iterations); OFF(tc_poisson_stats, rel_residual); OFF(tc_poisson_stats, iso_value); OFF(tc_poisson_stats, occupied_nodes);
    VAL(TC_INVALID_DATA); VAL(TC_POISSON_MIN_POINTS); VAL(TC_POISSON_MIN_DEPTH); VAL(TC_POISSON_MAX_DEPTH);
    /* the defaults */
    tc_poisson_config cfg;
    defaults(&cfg);
    defaults(NULL);
    printf("default.depth %u\ndefault.max_iterations %u\ndefault.floats_ok %d\n", cfg.depth, cfg.max_iterations,
           (int)(cfg.scale == 1.1f && cfg.point_weight == 0.0f && cfg.tolerance == 1e-5f && cfg.min_density == 0.0f));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float points[36] = {0}, normals[36] = {0}, chi[4] = {7, 7, 7, 7};
    tc_mc_grid grid = {{7, 7, 7}, {7, 7, 7}, {7, 7, 7}, 7};
    tc_poisson_stats stats = {7, 7, 7, 7};
    size_t nv = 7, nf = 7;
    for (int k = 0; k < 2; ++k) {
        printf("call.field_null_%d %d\n", k, (int)field[k](NULL, points, normals, 12, &cfg, &grid, chi, NULL, &stats));
        printf("call.reconstruct_null_%d %d\n", k, (int)recon[k](NULL, points, normals, 12, &cfg, NULL, NULL, 0, 0, &nv, &nf, &stats));
    }
    printf("call.null_wrote %d\n", (int)(chi[0] != 7 || chi[3] != 7 || grid.dims[0] != 7 || grid.layout != 7 || stats.iterations != 7 || nv != 7 || nf != 7));
    return 0;
}
