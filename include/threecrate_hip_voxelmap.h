/* threecrate_hip_voxelmap.h -- companion surface: a voxel map that lives on the device across chunks of a point stream
 * (StreamingVoxelFilter, threecrate-algorithms/src/streaming.rs:191-285; the wheel's RealtimeVoxelFilter,
 * threecrate-python/src/lib.rs:2380-2497).  Chunks are inserted as they arrive; every voxel keeps f64 sums and a count; the
 * result is one centroid per voxel.
 *
 * The symbols live in a library of their own, libthreecrate_hip_voxelmap.so, which is linked against libthreecrate_hip.so (it
 * sits in the same directory and finds it through $ORIGIN) and uses its status and context types: a tc_context made by
 * tc_context_create serves both.  tc_abi_version() is unchanged.  A consumer links both libraries.
 *
 * A tc_voxel_map is bound to the tc_context that created it and to that context's stream; the context must outlive it and
 * serves one call at a time, the map's calls included.
 *
 * ---- the contract, in the order of operations; every result is bit for bit ----
 * Keys (voxel_key, streaming.rs:231-239).  inv = 1.0f / voxel_size, once, in f32.  Per axis p = x * inv in f32 (a product, not
 *   a division; no FMA is involved), k = (int32) floor(p).  A NaN product (a NaN coordinate; 0 x inf when inv overflowed) gives
 *   k = 0 on that axis, which is what Rust's `as i32` yields.
 * Key range.  A key is valid when every axis lies in [-TC_VOXEL_MAP_KEY_LIMIT, TC_VOXEL_MAP_KEY_LIMIT) = [-2^20, 2^20): 21 bits
 *   per axis of a packed 64-bit key.  If ANY point of a chunk falls outside (+-inf and saturated products included), the insert
 *   returns TC_UNSUPPORTED, its message names the limit, and the map is exactly what it was: validity is decided for the whole
 *   chunk before the table is touched.  (The reference has no such limit: its keys are any i32.)
 * Sums (process_chunk, :254-261).  For every voxel and axis the f64 sum is the sequential fold s = s + (double)x over the
 *   voxel's points in stream order: chunks in call order, inside a chunk ascending index, starting from the sum the voxel
 *   already holds.  The state after a stream therefore does not depend on how the stream was cut into chunks.  A NaN coordinate
 *   poisons its axis' sum, as in the reference (the sign and payload of such a NaN are unspecified).  count is a u32: the
 *   behaviour beyond 2^32 - 1 points in one voxel is unspecified.
 * Centroid (finalize, :270-275).  (float)(sum / (double)count): a true f64 division.
 * Extraction order.  Ascending (kx, ky, kz) as signed integers.  (The reference's order is its HashMap's, unspecified.)  It does
 *   not depend on the table's capacity or history.
 *
 * ---- the table ----
 * Open addressing with linear probing over a power-of-two number of slots; the load factor is at most 1/2 after every insert.
 * Before a chunk with R distinct voxels goes in, the slots are doubled while 2 * (V + R) > slots (V = voxels held), and every
 * occupied slot is re-inserted once into the new table.  Beyond TC_VOXEL_MAP_MAX_CAPACITY slots the insert returns
 * TC_UNSUPPORTED and the map is unchanged.  tc_voxel_map_config::initial_capacity is in slots, rounded up to a power of two;
 * 0 means TC_VOXEL_MAP_DEFAULT_CAPACITY; anything below TC_VOXEL_MAP_MIN_CAPACITY is raised to it.
 * The scratch of an insert and of an extraction lives in the handle and only grows.
 * The number of NEW voxels of an insert is counted on the device and comes back to the host with the next call's read-back
 * (the next insert's, or the one tc_voxel_map_size / tc_voxel_map_extract make when a count is outstanding): an insert waits
 * for the device once, for the chunk's run count and range flag, apart from calls that grow the scratch (one more wait per
 * buffer that grows) or the table (one more wait, after the rehash): a caller must not assume that every _device insert
 * overlaps with its own work. */
#ifndef THREECRATE_HIP_VOXELMAP_H
#define THREECRATE_HIP_VOXELMAP_H

#include "threecrate_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TC_VOXEL_MAP_KEY_LIMIT        1048576                /* 2^20: keys lie in [-2^20, 2^20) per axis */
#define TC_VOXEL_MAP_MIN_CAPACITY     ((size_t)1 << 8)       /* slots: the floor of initial_capacity */
#define TC_VOXEL_MAP_DEFAULT_CAPACITY ((size_t)1 << 16)      /* slots: initial_capacity == 0 */
#define TC_VOXEL_MAP_MAX_CAPACITY     ((size_t)1 << 28)      /* slots: the table never grows beyond this */

typedef struct tc_voxel_map tc_voxel_map;

typedef struct tc_voxel_map_config {        /* StreamingVoxelFilterConfig, streaming.rs:196-201, + the table's first size */
    float  voxel_size;
    size_t initial_capacity;
} tc_voxel_map_config;

/* Checks, in this order: a NULL out is TC_INVALID_DATA; *out = NULL; a NULL config is TC_INVALID_DATA; voxel_size must be > 0
 * (a NaN fails this), else TC_INVALID_DATA "voxel_size must be positive" (:251-253); initial_capacity above
 * TC_VOXEL_MAP_MAX_CAPACITY is TC_UNSUPPORTED; a NULL context is TC_INVALID_DATA. */
tc_status tc_voxel_map_create(tc_context *ctx, const tc_voxel_map_config *config, tc_voxel_map **out);
/* NULL is allowed.  Waits for the context's stream. */
void tc_voxel_map_destroy(tc_voxel_map *map);
/* Empties the map (no voxels, no points) and keeps the table at its current size and the scratch.  NULL is TC_INVALID_DATA. */
tc_status tc_voxel_map_reset(tc_voxel_map *map);
/* The number of voxels held (voxel_count, :241-244); 0 for NULL (or when the outstanding count could not be read). */
size_t tc_voxel_map_size(tc_voxel_map *map);
/* The number of points inserted since creation or the last reset; 0 for NULL. */
uint64_t tc_voxel_map_points(tc_voxel_map *map);

/* Insert n points (xyz: n x 3 floats) as the next chunk of the stream.
 * Checks, in this order: a NULL map is TC_INVALID_DATA; n == 0 is TC_OK and does nothing; a NULL xyz is TC_INVALID_DATA;
 * n >= 2^32 - 16 is TC_UNSUPPORTED; a point outside the key range is TC_UNSUPPORTED; a table that would have to grow beyond
 * TC_VOXEL_MAP_MAX_CAPACITY is TC_UNSUPPORTED.  A call that fails leaves the map and both counters as they were.
 * The _device variant takes a device pointer and returns once the insert is enqueued on the context's stream (it has waited for
 * the chunk's run count before, and again if the scratch or the table had to grow); d_xyz must stay valid until the stream
 * has passed it.  The host variant returns with the stream drained. */
tc_status tc_voxel_map_insert(tc_voxel_map *map, const float *xyz, size_t n);
tc_status tc_voxel_map_insert_device(tc_voxel_map *map, const float *d_xyz, size_t n);

/* The map's V voxels in extraction order.  Every array may be NULL; n_voxels is always written (V).
 *   keys        V x 3: kx, ky, kz
 *   counts      V
 *   sums        V x 3 f64
 *   centroids   V x 3 f32
 * Checks, in this order: a NULL map or n_voxels is TC_INVALID_DATA; with every array NULL the call only counts; otherwise
 * capacity < V is TC_INVALID_DATA and no array is written.  The map is not changed: inserting may go on afterwards.
 * The _device variant takes device pointers (keys, counts, sums, centroids); n_voxels is a host pointer in both.  Both return
 * with the stream drained. */
tc_status tc_voxel_map_extract(tc_voxel_map *map, int32_t *keys, uint32_t *counts, double *sums, float *centroids, size_t capacity,
                               size_t *n_voxels);
tc_status tc_voxel_map_extract_device(tc_voxel_map *map, int32_t *d_keys, uint32_t *d_counts, double *d_sums, float *d_centroids,
                                      size_t capacity, size_t *n_voxels);

#ifdef __cplusplus
}
#endif
#endif /* THREECRATE_HIP_VOXELMAP_H */
