/* abi_tsdf.c -- a COMPILED consumer of include/threecrate_hip_tsdf.h (test infrastructure), the companion of abi_conformance.c for
 * the TSDF surface: prints sizeof of its two structs, offsetof and size of every field and the value of its flag constant, one
 * `name value` pair per line; tests/test_abi_tsdf.py compares them with the ctypes mirror (threecrate_amd/_lib.py) and with the
 * #[repr(C)] structs of bindings/rust (ffi_tsdf.rs).  It takes the address of every export, so it links only against a library that has
 * them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_tsdf.c -Lthreecrate_amd -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_tsdf.h"

#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf("offsetof." #T "." #f " %zu\nfieldsize." #T "." #f " %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
#define VAL(c) printf("const." #c " %lld\n", (long long)(c))

int main(void) {
    /* the prototypes as a caller spells them: a mismatch with the header is a compile error */
    tc_status (*create)(tc_context *, const tc_tsdf_volume_config *, tc_tsdf_volume **) = tc_tsdf_volume_create;
    void (*destroy)(tc_tsdf_volume *) = tc_tsdf_volume_destroy;
    tc_status (*reset)(tc_tsdf_volume *) = tc_tsdf_volume_reset;
    tc_status (*integrate[2])(tc_tsdf_volume *, const float *, const uint8_t *, const tc_camera_intrinsics *, const float *, size_t *) = {
        tc_tsdf_integrate, tc_tsdf_integrate_device};
    tc_status (*download[2])(tc_tsdf_volume *, float *, uint8_t *, uint8_t *) = {tc_tsdf_volume_download, tc_tsdf_volume_download_device};
    tc_status (*upload[2])(tc_tsdf_volume *, const float *, const uint8_t *, const uint8_t *) = {tc_tsdf_volume_upload, tc_tsdf_volume_upload_device};
    tc_status (*extract[2])(tc_tsdf_volume *, float, uint32_t, float *, uint8_t *, size_t, size_t *) = {tc_tsdf_extract_surface,
                                                                                                       tc_tsdf_extract_surface_device};
    int exports = (create != 0) + (destroy != 0) + (reset != 0);
    for (int k = 0; k < 2; ++k) exports += (integrate[k] != 0) + (download[k] != 0) + (upload[k] != 0) + (extract[k] != 0);
    printf("count.exports %d\n", exports);

    SZ(tc_tsdf_volume_config);
    OFF(tc_tsdf_volume_config, voxel_size); OFF(tc_tsdf_volume_config, truncation_distance); OFF(tc_tsdf_volume_config, resolution);
    OFF(tc_tsdf_volume_config, origin); OFF(tc_tsdf_volume_config, max_weight);
    SZ(tc_camera_intrinsics);
    OFF(tc_camera_intrinsics, fx); OFF(tc_camera_intrinsics, fy); OFF(tc_camera_intrinsics, cx); OFF(tc_camera_intrinsics, cy);
    OFF(tc_camera_intrinsics, width); OFF(tc_camera_intrinsics, height);
    VAL(TC_TSDF_OBSERVED_EDGES);
    VAL(TC_INVALID_DATA);
    /* the error paths that need no device: a NULL handle is TC_INVALID_DATA everywhere, destroy(NULL) is a no-op */
    destroy(NULL);
    size_t n = 7;
    printf("call.reset_null %d\n", (int)reset(NULL));
    printf("call.extract_null %d\n", (int)extract[0](NULL, 0.0f, 0u, NULL, NULL, 0, &n));
    printf("call.extract_null_n %zu\n", n);
    return 0;
}
