/* abi_mesh.c -- a COMPILED consumer of include/threecrate_hip_mesh.h (test infrastructure), the companion of abi_color.c for the
 * surface of libthreecrate_hip_mesh.so: prints sizeof of its struct, offsetof and size of every field and the values of its constants,
 * one `name value` pair per line; tests/test_abi_mesh.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the
 * #[repr(C)] struct of bindings/rust (ffi_mesh.rs).  It takes the address of every export, so it links only against a library that
 * has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_mesh.c -Lthreecrate_amd -lthreecrate_hip_mesh -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_mesh.h"

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
    void (*defaults)(uint32_t, tc_mesh_smooth_config *) = tc_mesh_smooth_config_default;
    tc_status (*smooth[2])(tc_context *, const float *, size_t, const uint32_t *, size_t, const tc_mesh_smooth_config *, float *) = {
        tc_mesh_smooth, tc_mesh_smooth_device};
    tc_status (*adjacency[2])(tc_context *, size_t, const uint32_t *, size_t, uint32_t *, uint32_t *, size_t, size_t *) = {
        tc_mesh_vertex_adjacency, tc_mesh_vertex_adjacency_device};
    printf("count.exports %d\n", (defaults != 0) + (smooth[0] != 0) + (smooth[1] != 0) + (adjacency[0] != 0) + (adjacency[1] != 0));

    SZ(tc_mesh_smooth_config); ALIGN(tc_mesh_smooth_config);
    OFF(tc_mesh_smooth_config, method); OFF(tc_mesh_smooth_config, iterations); OFF(tc_mesh_smooth_config, lambda);
    OFF(tc_mesh_smooth_config, mu); OFF(tc_mesh_smooth_config, alpha); OFF(tc_mesh_smooth_config, beta);
    VAL(TC_MESH_LAPLACIAN);
    VAL(TC_MESH_TAUBIN);
    VAL(TC_MESH_HC);
    VAL(TC_INVALID_DATA);
    /* the defaults */
    tc_mesh_smooth_config cfg = {9, 9, 9.0f, 9.0f, 9.0f, 9.0f};
    defaults(TC_MESH_HC, &cfg);
    defaults(TC_MESH_HC, NULL);
    printf("default.method %u\ndefault.iterations %u\n", (unsigned)cfg.method, (unsigned)cfg.iterations);
    printf("default.lambda_ok %d\ndefault.mu_ok %d\ndefault.alpha_ok %d\ndefault.beta_ok %d\n", (int)(cfg.lambda == 0.5f), (int)(cfg.mu == -0.53f),
           (int)(cfg.alpha == 0.0f), (int)(cfg.beta == 0.5f));
    /* the error path that needs no device: a NULL context is TC_INVALID_DATA and nothing is written */
    float vertices[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, out[9] = {7, 7, 7, 7, 7, 7, 7, 7, 7};
    uint32_t faces[3] = {0, 1, 2}, offsets[4] = {7, 7, 7, 7}, neighbors[6] = {7, 7, 7, 7, 7, 7};
    size_t entries = 7;
    printf("call.smooth_null %d\n", (int)smooth[0](NULL, vertices, 3, faces, 1, &cfg, out));
    printf("call.smooth_device_null %d\n", (int)smooth[1](NULL, vertices, 3, faces, 1, &cfg, out));
    printf("call.adjacency_null %d\n", (int)adjacency[0](NULL, 3, faces, 1, offsets, neighbors, 6, &entries));
    printf("call.adjacency_device_null %d\n", (int)adjacency[1](NULL, 3, faces, 1, offsets, neighbors, 6, &entries));
    printf("call.null_wrote %d\n", (int)(out[0] != 7 || out[8] != 7 || offsets[0] != 7 || neighbors[0] != 7 || entries != 7));
    return 0;
}
