/* abi_global.c -- a COMPILED consumer of include/threecrate_hip_global.h (test infrastructure), the companion of abi_conformance.c and
 * abi_tsdf.c for the surface of libthreecrate_hip_global.so: prints sizeof of its struct, offsetof and size of every field and the value
 * of its constant, one `name value` pair per line; tests/test_abi_global.py compares them with the ctypes mirror (threecrate_amd/_lib.py)
 * and with the #[repr(C)] struct of bindings/rust (ffi_global.rs).  It takes the address of every export, so it links only against a
 * library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_global.c -Lthreecrate_amd -lthreecrate_hip_global -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_global.h"

#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf("offsetof." #T "." #f " %zu\nfieldsize." #T "." #f " %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
#define VAL(c) printf("const." #c " %lld\n", (long long)(c))

int main(void) {
    /* the prototypes as a caller spells them: a mismatch with the header is a compile error */
    tc_status (*match[2])(tc_context *, const float *, size_t, const float *, size_t, size_t, uint32_t *, float *) = {tc_match_features,
                                                                                                                      tc_match_features_device};
    tc_status (*seeded[2])(tc_context *, const float *, size_t, const float *, size_t, const uint32_t *, const uint32_t *, size_t, float, float, size_t,
                           uint64_t, float *, tc_ransac_result *, float *, uint32_t *) = {tc_ransac_correspondences, tc_ransac_correspondences_device};
    tc_status (*samples[2])(tc_context *, const float *, size_t, const float *, size_t, const uint32_t *, const uint32_t *, size_t, float, float,
                            const uint32_t *, size_t, float *, tc_ransac_result *, float *, uint32_t *) = {tc_ransac_correspondences_samples,
                                                                                                          tc_ransac_correspondences_samples_device};
    int exports = 0;
    for (int k = 0; k < 2; ++k) exports += (match[k] != 0) + (seeded[k] != 0) + (samples[k] != 0);
    printf("count.exports %d\n", exports);

    SZ(tc_ransac_result);
    OFF(tc_ransac_result, inlier_count); OFF(tc_ransac_result, iterations_run); OFF(tc_ransac_result, best_iteration);
    OFF(tc_ransac_result, early_exit); OFF(tc_ransac_result, inlier_ratio);
    VAL(TC_RANSAC_MAX_ITERS);
    VAL(TC_FPFH_DIM);
    VAL(TC_INVALID_DATA);
    /* the error paths that need no device: a NULL context is TC_INVALID_DATA everywhere and nothing is written */
    float t[12] = {7.0f};
    tc_ransac_result r = {7u, 7u, 7u, 7, 7.0f};
    uint32_t idx = 7u;
    printf("call.match_null %d\n", (int)match[0](NULL, t, 1, t, 1, TC_FPFH_DIM, &idx, NULL));
    printf("call.ransac_null %d\n", (int)seeded[0](NULL, t, 4, t, 4, &idx, &idx, 4, 0.1f, 0.25f, 10, 0u, t, &r, NULL, NULL));
    printf("call.samples_null %d\n", (int)samples[1](NULL, t, 4, t, 4, &idx, &idx, 4, 0.1f, 0.25f, &idx, 10, t, &r, NULL, NULL));
    printf("call.null_wrote %d\n", (int)(idx != 7u || t[0] != 7.0f || r.inlier_count != 7u || r.early_exit != 7));
    return 0;
}
