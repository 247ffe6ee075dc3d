/* abi_voxelmap.c -- a COMPILED consumer of include/threecrate_hip_voxelmap.h (test infrastructure), the companion of abi_global.c for
 * the surface of libthreecrate_hip_voxelmap.so: prints sizeof of its struct, offsetof and size of every field and the values of its
 * constants, one `name value` pair per line; tests/test_abi_voxelmap.py compares them with the ctypes mirror (threecrate_amd/_lib.py)
 * and with the #[repr(C)] struct of bindings/rust (ffi_voxelmap.rs).  It takes the address of every export, so it links only against
 * a library that has them all.
 * Build: gcc -std=c11 -Wall -Wextra -Werror -Iinclude tests/abi/abi_voxelmap.c -Lthreecrate_amd -lthreecrate_hip_voxelmap -lthreecrate_hip
 */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "threecrate_hip_voxelmap.h"

#define SZ(T) printf("sizeof." #T " %zu\n", sizeof(T))
#define OFF(T, f) printf("offsetof." #T "." #f " %zu\nfieldsize." #T "." #f " %zu\n", offsetof(T, f), sizeof(((T *)0)->f))
#define VAL(c) printf("const." #c " %lld\n", (long long)(c))

int main(void) {
    /* the prototypes as a caller spells them: a mismatch with the header is a compile error */
    tc_status (*create)(tc_context *, const tc_voxel_map_config *, tc_voxel_map **) = tc_voxel_map_create;
    void (*destroy)(tc_voxel_map *) = tc_voxel_map_destroy;
    tc_status (*reset)(tc_voxel_map *) = tc_voxel_map_reset;
    size_t (*size)(tc_voxel_map *) = tc_voxel_map_size;
    uint64_t (*points)(tc_voxel_map *) = tc_voxel_map_points;
    tc_status (*insert[2])(tc_voxel_map *, const float *, size_t) = {tc_voxel_map_insert, tc_voxel_map_insert_device};
    tc_status (*extract[2])(tc_voxel_map *, int32_t *, uint32_t *, double *, float *, size_t, size_t *) = {tc_voxel_map_extract,
                                                                                                         tc_voxel_map_extract_device};
    int exports = (create != 0) + (destroy != 0) + (reset != 0) + (size != 0) + (points != 0);
    for (int k = 0; k < 2; ++k) exports += (insert[k] != 0) + (extract[k] != 0);
    printf("count.exports %d\n", exports);

    SZ(tc_voxel_map_config);
    OFF(tc_voxel_map_config, voxel_size); OFF(tc_voxel_map_config, initial_capacity);
    VAL(TC_VOXEL_MAP_KEY_LIMIT);
    VAL(TC_VOXEL_MAP_MIN_CAPACITY);
    VAL(TC_VOXEL_MAP_DEFAULT_CAPACITY);
    VAL(TC_VOXEL_MAP_MAX_CAPACITY);
    VAL(TC_INVALID_DATA);
    /* the error paths that need no device: a NULL context or handle is TC_INVALID_DATA everywhere and nothing is written */
    float xyz[3] = {7.0f, 7.0f, 7.0f};
    int32_t keys[3] = {7, 7, 7};
    size_t n = 7;
    tc_voxel_map_config cfg = {1.0f, 0};
    tc_voxel_map *map = (tc_voxel_map *)&cfg;
    printf("call.create_null %d\n", (int)create(NULL, &cfg, &map));
    printf("call.create_wrote_null %d\n", (int)(map == NULL));
    printf("call.reset_null %d\n", (int)reset(NULL));
    printf("call.insert_null %d\n", (int)insert[0](NULL, xyz, 1));
    printf("call.insert_device_null %d\n", (int)insert[1](NULL, xyz, 1));
    printf("call.extract_null %d\n", (int)extract[0](NULL, keys, NULL, NULL, NULL, 1, &n));
    printf("call.extract_device_null %d\n", (int)extract[1](NULL, keys, NULL, NULL, NULL, 1, &n));
    printf("call.size_null %d\n", (int)(size(NULL) + points(NULL)));
    destroy(NULL);
    printf("call.null_wrote %d\n", (int)(xyz[0] != 7.0f || keys[0] != 7 || n != 7));
    return 0;
}
