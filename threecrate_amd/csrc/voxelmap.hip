// voxelmap.hip -- a voxel map that lives on the device across the chunks of a point stream (StreamingVoxelFilter,
// threecrate-algorithms/src/streaming.rs:191-285); the entry points of include/threecrate_hip_voxelmap.h, which pins the arithmetic.
// This unit is the whole of the companion library libthreecrate_hip_voxelmap.so; the host layer of tc_internal.h (ensure, stage_in,
// read_back, group_by_key, sort_pairs, exclusive_scan_u32, ProfScope) resolves from libthreecrate_hip.so.
//   The table: open addressing, linear probing, power-of-two slots, three arrays -- packed keys (u64, all ones = empty; a packed key
//   never has bit 63), counts (u32), sums (3 f64 per slot).  Load factor <= 1/2 after every insert.
//   One road per chunk:
//   vm_key          a thread per point: the biased key (kx + 2^20) << 42 | (ky + 2^20) << 21 | (kz + 2^20) and the point's index; a key
//                   out of range raises the chunk's flag (one atomic per wave that has such a lane)
//   group_by_key (grid.hip)   stable: the points of a voxel stay in stream order; one run per distinct voxel
//   vm_long_list    the runs longer than kVoxelMapLongRun, listed for the wave-per-run kernel
//   -- one read-back: the run count R, the flag, the long-run count (and the new-voxel count of the insert before) --
//   vm_rehash       only when 2 (V + R) > slots: a thread per OLD slot re-inserts it into the cleared new table
//   vm_insert       a thread per run.  The keys of one launch are distinct, so a slot is claimed by one 64-bit atomicCAS from empty
//                   to the key; a thread that finds its key already there owns that slot for this launch.  The owner folds its run in
//                   sorted = stream order starting from the slot's sums: the adds are sequential, eight gathers in flight at a time
//                   (fold_run_lane, run_fold.h).  New voxels: one integer atomic per block
//   vm_insert_long  a wave per long run: 64 coalesced index loads + gathers at once, the adds sequential on broadcast values
//                   (fold_run_wave, run_fold.h)
//   Extraction: vm_occupied (flags) -> exclusive_scan_u32 -> vm_compact (packed key, slot) -> sort_pairs on all 63 bits -> vm_gather.
#include "tc_internal.h"
#include "run_fold.h"
#include "../../include/threecrate_hip_voxelmap.h"

#include <algorithm>
#include <cmath>

namespace tc {

// scratch slots of a tc_voxel_map (grow-only, owned by the handle)
enum VoxelMapSlot {
    VM_KEYS, VM_KEYS_SORTED,    // insert: packed keys of the chunk | sorted (u64 * n); extraction: of the occupied slots | sorted (u64 * V)
    VM_INDEX, VM_ORDER,         // insert: point indices | in sorted order (u32 * n); extraction: slot numbers | in sorted order (u32 * V)
    VM_HEAD,                    // insert: run heads, then the list of long runs (u32 * n); extraction: occupied flags (u32 * slots)
    VM_RUNPOS,                  // insert: run number of every sorted position (n + 1, [n] = R); extraction: output position of every slot (slots + 1)
    VM_RSTART,                  // insert: first sorted position of every run (n + 1)
    VM_SORT_TEMP, VM_BLOCKSUM,  // rocPRIM's temporary storage (bytes); the scan's block sums
    VM_STAGE,                   // host extraction: the outputs before they are copied back
    VM_SLOTS
};

}  // namespace tc

struct tc_voxel_map {
    tc_context *ctx = nullptr;
    float voxel_size = 0.0f, inv = 0.0f;
    size_t slots = 0;               // power of two
    size_t n_voxels = 0;            // V, without the outstanding count
    uint64_t n_points = 0;
    bool pending = false;           // counters[2] holds the new voxels of the last insert, not yet added to n_voxels
    tc::DevBuf keys, counts, sums;  // the table: u64 * slots, u32 * slots, f64 * 3 slots; blocks of exactly their size, owned
    tc::DevBuf counters;            // u32: [0] out-of-range flag, [1] long runs, [2] new voxels of the last insert
    tc::DevBuf scratch[tc::VM_SLOTS];
};

namespace tc {

constexpr uint32_t kVoxelMapLongRun = 96;       // points; a longer run gets a wave (kLongVoxel of voxel.hip)
constexpr uint64_t kVmEmpty = ~0ull;
constexpr int kVmBias = TC_VOXEL_MAP_KEY_LIMIT; // 2^20
constexpr int kVmLongBlocks = 1024;             // the wave-per-run kernel's grid is capped; its waves stride over the list

struct VmTable {
    uint64_t *keys;
    uint32_t *counts;
    double   *sums;
    uint32_t  shift;            // 64 - log2(slots)
    uint32_t  mask;             // slots - 1 (slots <= 2^28)
};

__device__ __forceinline__ uint32_t vm_home(const VmTable &t, uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> t.shift) & t.mask; }

// The slot of `key`: claimed from empty, or found.  Every key of one launch is distinct and the table has an empty slot (load factor <= 1/2),
// so the walk ends.  A slot's key word only ever changes from empty to a key: a relaxed read that sees a key sees the final one, and a stale
// "empty" is settled by the compare-and-swap.
__device__ __forceinline__ uint32_t vm_claim(const VmTable &t, uint64_t key, bool &is_new) {
    uint32_t s = vm_home(t, key);
    for (;;) {
        uint64_t cur = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kVmEmpty) cur = atomicCAS((unsigned long long *)&t.keys[s], (unsigned long long)kVmEmpty, (unsigned long long)key);
        if (cur == kVmEmpty) { is_new = true; return s; }
        if (cur == key) { is_new = false; return s; }
        s = (s + 1u) & t.mask;
    }
}

// streaming.rs:231-239 per axis: p = x * inv (f32), floor, `as i32` (NaN -> 0); ok = false when the key leaves [-2^20, 2^20)
__device__ __forceinline__ int vm_axis_key(float x, float inv, bool &ok) {
    const float p = x * inv;
    if (p != p) return 0;
    const float f = floorf(p);
    if (!(f >= -(float)kVmBias && f < (float)kVmBias)) { ok = false; return 0; }
    return (int)f;
}

__global__ void __launch_bounds__(256) vm_key_kernel(const float *__restrict__ xyz, uint32_t n, float inv, uint64_t *__restrict__ keys,
                                                    uint32_t *__restrict__ idx, uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = true;
    if (i < n) {
        const int kx = vm_axis_key(xyz[3 * (size_t)i], inv, ok), ky = vm_axis_key(xyz[3 * (size_t)i + 1], inv, ok),
                  kz = vm_axis_key(xyz[3 * (size_t)i + 2], inv, ok);
        keys[i] = ((uint64_t)(uint32_t)(kx + kVmBias) << 42) | ((uint64_t)(uint32_t)(ky + kVmBias) << 21) | (uint64_t)(uint32_t)(kz + kVmBias);
        idx[i] = i;
    }
    if (__ballot(!ok) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flag, 1u);
}

__global__ void __launch_bounds__(256) vm_long_list_kernel(const uint32_t *__restrict__ rstart, const uint32_t *__restrict__ n_runs,
                                                          uint32_t *__restrict__ long_list, uint32_t list_cap, uint32_t *__restrict__ long_count) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= *n_runs) return;
    if (rstart[r + 1] - rstart[r] > kVoxelMapLongRun) append_long_run(long_list, list_cap, long_count, r);
}

__global__ void __launch_bounds__(256) vm_insert_kernel(VmTable t, const float *__restrict__ xyz, const uint64_t *__restrict__ keys_sorted,
                                                       const uint32_t *__restrict__ order, const uint32_t *__restrict__ rstart, uint32_t n_runs,
                                                       uint32_t *__restrict__ new_count) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool is_new = false;
    if (r < n_runs) {
        const uint32_t s = rstart[r], e = rstart[r + 1];
        if (e - s <= kVoxelMapLongRun) {                        // (a long run is claimed and folded by its wave)
            const uint32_t slot = vm_claim(t, keys_sorted[s], is_new);
            double *sum = t.sums + 3 * (size_t)slot;
            XyzSum acc{sum[0], sum[1], sum[2]};                 // the slot's running sums: zero in a fresh slot
            fold_run_lane<8>(s, e, [&](uint32_t j) { return load_xyz_point(xyz, order, j); }, [&](const XyzPoint &p) { acc.add(p); });
            sum[0] = acc.x; sum[1] = acc.y; sum[2] = acc.z;
            t.counts[slot] += e - s;
        }
    }
    const int fresh = __syncthreads_count(is_new ? 1 : 0);
    if (threadIdx.x == 0 && fresh) atomicAdd(new_count, (uint32_t)fresh);
}

__global__ void __launch_bounds__(256) vm_insert_long_kernel(VmTable t, const float *__restrict__ xyz, const uint64_t *__restrict__ keys_sorted,
                                                            const uint32_t *__restrict__ order, const uint32_t *__restrict__ rstart,
                                                            const uint32_t *__restrict__ long_list, uint32_t n_long, uint32_t *__restrict__ new_count) {
    __shared__ uint32_t fresh;
    if (threadIdx.x == 0) fresh = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0u;
    // (the list walk of for_each_listed_run, run_fold.h, written out: inside its callable the probe loop of vm_claim compiled to another body)
    const uint32_t nwaves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t entry = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); entry < n_long; entry += nwaves) {     // wave-uniform
        const uint32_t r = long_list[entry];
        const uint32_t s = rstart[r], e = rstart[r + 1];
        uint32_t slot = 0u;
        if (lane == 0u) {
            bool is_new = false;
            slot = vm_claim(t, keys_sorted[s], is_new);
            mine += is_new ? 1u : 0u;
        }
        slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        double *sum = t.sums + 3 * (size_t)slot;
        XyzSum acc{sum[0], sum[1], sum[2]};                     // every lane runs the same chain
        // (32-bit trips, as the kernel was written: right while a chunk has fewer than 2^32 - 64 points; the entry check admits 48 more)
        fold_run_wave<uint32_t>(s, e, lane, [&](uint32_t j) { return load_xyz_point(xyz, order, j); }, [&](const XyzPoint &p) { acc.add(p); });
        if (lane == 0u) {
            sum[0] = acc.x; sum[1] = acc.y; sum[2] = acc.z;
            t.counts[slot] += e - s;
        }
    }
    if (lane == 0u && mine) atomicAdd(&fresh, mine);
    __syncthreads();
    if (threadIdx.x == 0 && fresh) atomicAdd(new_count, fresh);
}

// a thread per slot of the old table: the keys are distinct, the new table is cleared and at least twice as large
__global__ void __launch_bounds__(256) vm_rehash_kernel(const uint64_t *__restrict__ old_keys, const uint32_t *__restrict__ old_counts,
                                                       const double *__restrict__ old_sums, uint32_t old_slots, VmTable t) {
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= old_slots) return;
    const uint64_t key = old_keys[o];
    if (key == kVmEmpty) return;
    bool is_new;
    const uint32_t slot = vm_claim(t, key, is_new);
    t.counts[slot] = old_counts[o];
    t.sums[3 * (size_t)slot] = old_sums[3 * (size_t)o]; t.sums[3 * (size_t)slot + 1] = old_sums[3 * (size_t)o + 1];
    t.sums[3 * (size_t)slot + 2] = old_sums[3 * (size_t)o + 2];
}

__global__ void __launch_bounds__(256) vm_occupied_kernel(const uint64_t *__restrict__ keys, uint32_t slots, uint32_t *__restrict__ flag) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < slots) flag[s] = keys[s] != kVmEmpty ? 1u : 0u;
}

__global__ void __launch_bounds__(256) vm_compact_kernel(const uint64_t *__restrict__ keys, uint32_t slots, const uint32_t *__restrict__ pos,
                                                        uint64_t *__restrict__ out_keys, uint32_t *__restrict__ out_slot) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= slots) return;
    const uint64_t key = keys[s];
    if (key == kVmEmpty) return;
    out_keys[pos[s]] = key;
    out_slot[pos[s]] = s;
}

// voxel v of the extraction order; every output optional.  finalize (streaming.rs:270-275): (sum / n) as f32, a true division
__global__ void __launch_bounds__(256) vm_gather_kernel(const uint64_t *__restrict__ keys_sorted, const uint32_t *__restrict__ slot_sorted, uint32_t nv,
                                                       const uint32_t *__restrict__ counts, const double *__restrict__ sums, int32_t *__restrict__ out_keys,
                                                       uint32_t *__restrict__ out_counts, double *__restrict__ out_sums, float *__restrict__ out_centroids) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const uint32_t slot = slot_sorted[v];
    const uint32_t cnt = counts[slot];
    const double sx = sums[3 * (size_t)slot], sy = sums[3 * (size_t)slot + 1], sz = sums[3 * (size_t)slot + 2];
    if (out_keys) {
        const uint64_t key = keys_sorted[v];
        out_keys[3 * (size_t)v] = (int32_t)((key >> 42) & 0x1FFFFFu) - kVmBias;
        out_keys[3 * (size_t)v + 1] = (int32_t)((key >> 21) & 0x1FFFFFu) - kVmBias;
        out_keys[3 * (size_t)v + 2] = (int32_t)(key & 0x1FFFFFu) - kVmBias;
    }
    if (out_counts) out_counts[v] = cnt;
    if (out_sums) { out_sums[3 * (size_t)v] = sx; out_sums[3 * (size_t)v + 1] = sy; out_sums[3 * (size_t)v + 2] = sz; }
    if (out_centroids) {
        const double nd = (double)cnt;
        out_centroids[3 * (size_t)v] = (float)(sx / nd); out_centroids[3 * (size_t)v + 1] = (float)(sy / nd); out_centroids[3 * (size_t)v + 2] = (float)(sz / nd);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static VmTable vm_table(const DevBuf &keys, const DevBuf &counts, const DevBuf &sums, size_t slots) {
    VmTable t;
    t.keys = (uint64_t *)keys.p; t.counts = (uint32_t *)counts.p; t.sums = (double *)sums.p;
    unsigned lg = 0;
    while (((size_t)1 << lg) < slots) ++lg;
    t.shift = 64u - lg; t.mask = (uint32_t)(slots - 1);
    return t;
}

// blocks of exactly the table's size from the device, not padded ones from the pool: the table is large and lives long
static tc_status vm_alloc_table(tc_context *ctx, size_t slots, DevBuf &keys, DevBuf &counts, DevBuf &sums) {
    const std::pair<DevBuf *, size_t> want[] = {{&keys, slots * sizeof(uint64_t)}, {&counts, slots * sizeof(uint32_t)}, {&sums, slots * 3 * sizeof(double)}};
    for (const auto &[b, bytes] : want) {
        if (hipMalloc(&b->p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            b->p = nullptr;
            free_buf(keys); free_buf(counts); free_buf(sums);
            return fail(ctx, TC_GPU, "voxel_map: out of device memory");
        }
        b->cap = bytes;
    }
    return TC_OK;
}

static tc_status vm_clear_table(tc_context *ctx, size_t slots, DevBuf &keys, DevBuf &counts, DevBuf &sums) {
    TC_HIP_TRY(ctx, hipMemsetAsync(keys.p, 0xFF, slots * sizeof(uint64_t), ctx->stream));
    TC_HIP_TRY(ctx, hipMemsetAsync(counts.p, 0, slots * sizeof(uint32_t), ctx->stream));
    TC_HIP_TRY(ctx, hipMemsetAsync(sums.p, 0, slots * 3 * sizeof(double), ctx->stream));
    return TC_OK;
}

static void vm_take_pending(tc_voxel_map *map, uint32_t n_new) {
    if (map->pending) { map->n_voxels += n_new; map->pending = false; }
}

// V on the host: the outstanding count of the last insert is read back when there is one
static tc_status vm_settle(tc_voxel_map *map) {
    if (!map->pending) return TC_OK;
    tc_context *ctx = map->ctx;
    VoxelMapOut *h = &pinned_host(ctx)->voxelmap_out;
    if (tc_status s = read_back(ctx, &h->n_new, (const uint32_t *)map->counters.p + 2, sizeof(uint32_t))) return s;
    vm_take_pending(map, h->n_new);
    return TC_OK;
}

static tc_status vm_grow(tc_voxel_map *map, size_t new_slots) {
    tc_context *ctx = map->ctx;
    DevBuf keys, counts, sums;
    if (tc_status s = vm_alloc_table(ctx, new_slots, keys, counts, sums)) return s;
    tc_status s = vm_clear_table(ctx, new_slots, keys, counts, sums);
    if (s == TC_OK) {
        ProfScope ps(ctx, "voxel_map_rehash");
        hipLaunchKernelGGL(vm_rehash_kernel, dim3(blocks_for(map->slots)), dim3(256), 0, ctx->stream, (const uint64_t *)map->keys.p,
                           (const uint32_t *)map->counts.p, (const double *)map->sums.p, (uint32_t)map->slots, vm_table(keys, counts, sums, new_slots));
    }
    if (s == TC_OK && hipGetLastError() != hipSuccess) s = fail(ctx, TC_GPU, "voxel_map: the rehash launch was refused");
    if (s == TC_OK) s = synced(ctx);                            // the old table is read until here
    if (s != TC_OK) { free_buf(keys); free_buf(counts); free_buf(sums); return s; }
    free_buf(map->keys); free_buf(map->counts); free_buf(map->sums);
    map->keys = keys; map->counts = counts; map->sums = sums; map->slots = new_slots;
    return TC_OK;
}

static tc_status vm_insert_device(tc_voxel_map *map, const float *d_xyz, size_t n) {
    tc_context *ctx = map->ctx;
    hipStream_t st = ctx->stream;
    auto &B = map->scratch;
    const uint32_t n32 = (uint32_t)n;
    if (tc_status s = ensure(ctx, B[VM_KEYS], n * sizeof(uint64_t))) return s;
    if (tc_status s = ensure(ctx, B[VM_INDEX], n * sizeof(uint32_t))) return s;
    uint64_t *keys = (uint64_t *)B[VM_KEYS].p;
    uint32_t *idx = (uint32_t *)B[VM_INDEX].p, *ctr = (uint32_t *)map->counters.p;
    KeyGroups g;
    TC_HIP_TRY(ctx, hipMemsetAsync(ctr, 0, 2 * sizeof(uint32_t), st));       // flag, long runs; [2] may still be outstanding
    {
        ProfScope ps(ctx, "voxel_map_sort");
        hipLaunchKernelGGL(vm_key_kernel, dim3(blocks_for(n)), dim3(256), 0, st, d_xyz, n32, map->inv, keys, idx, ctr);
        if (tc_status s = group_by_key(ctx, keys, idx, n, 63u,
                                       GroupBufs{B[VM_KEYS_SORTED], B[VM_ORDER], B[VM_HEAD], B[VM_RUNPOS], B[VM_RSTART], B[VM_SORT_TEMP], B[VM_BLOCKSUM]}, g)) return s;
        // the head flags are no longer needed: their n words take the list of long runs
        hipLaunchKernelGGL(vm_long_list_kernel, dim3(blocks_for(n)), dim3(256), 0, st, g.rstart, g.n_runs, g.head, n32, ctr + 1);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    // the one read-back: flag | long runs | new voxels of the insert before, then the run count (which drains the stream)
    VoxelMapOut *h = &pinned_host(ctx)->voxelmap_out;
    TC_HIP_TRY(ctx, hipMemcpyAsync(&h->out_of_range, ctr, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    if (tc_status s = read_back(ctx, &h->runs, g.n_runs, sizeof(uint32_t))) return s;
    vm_take_pending(map, h->n_new);
    if (h->out_of_range) return fail(ctx, TC_UNSUPPORTED, "voxel_map_insert: a point's voxel key is outside [-2^20, 2^20) on some axis");
    const size_t R = h->runs, n_long = h->n_long;
    size_t slots = map->slots;
    while (2 * (map->n_voxels + R) > slots) {
        if (slots >= TC_VOXEL_MAP_MAX_CAPACITY) return fail(ctx, TC_UNSUPPORTED, "voxel_map_insert: the table would grow beyond 2^28 slots");
        slots *= 2;
    }
    if (slots != map->slots) if (tc_status s = vm_grow(map, slots)) return s;
    const VmTable t = vm_table(map->keys, map->counts, map->sums, map->slots);
    TC_HIP_TRY(ctx, hipMemsetAsync(ctr + 2, 0, sizeof(uint32_t), st));
    {
        ProfScope ps(ctx, "voxel_map_insert");
        hipLaunchKernelGGL(vm_insert_kernel, dim3(blocks_for(R)), dim3(256), 0, st, t, d_xyz, g.keys_sorted, g.order, g.rstart, (uint32_t)R, ctr + 2);
    }
    if (n_long) {
        ProfScope ps(ctx, "voxel_map_insert_long");
        const unsigned blocks = (unsigned)std::min<size_t>((n_long + 3) / 4, kVmLongBlocks);
        hipLaunchKernelGGL(vm_insert_long_kernel, dim3(blocks), dim3(256), 0, st, t, d_xyz, g.keys_sorted, g.order, g.rstart, (const uint32_t *)g.head,
                           (uint32_t)n_long, ctr + 2);
    }
    // from here on the map has changed: the counters follow even if the launch error below is reported
    map->pending = true;
    map->n_points += n;
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

// the caller's arrays, each optional, are device arrays, or -- on_host -- host arrays that are filled through the handle's staging block
static tc_status vm_extract(tc_voxel_map *map, int32_t *keys, uint32_t *counts, double *sums, float *centroids, size_t capacity, size_t *n_voxels, bool on_host) {
    tc_context *ctx = map->ctx;
    hipStream_t st = ctx->stream;
    if (tc_status s = vm_settle(map)) return s;
    const size_t V = map->n_voxels, slots = map->slots;
    *n_voxels = V;
    if (!keys && !counts && !sums && !centroids) return TC_OK;
    if (capacity < V) return fail(ctx, TC_INVALID_DATA, "voxel_map_extract: capacity is smaller than the number of voxels");
    if (V == 0) return TC_OK;
    auto &B = map->scratch;
    const std::pair<VoxelMapSlot, size_t> need[] = {{VM_KEYS, V * sizeof(uint64_t)}, {VM_KEYS_SORTED, V * sizeof(uint64_t)}, {VM_INDEX, V * sizeof(uint32_t)},
                                                    {VM_ORDER, V * sizeof(uint32_t)}, {VM_HEAD, slots * sizeof(uint32_t)}, {VM_RUNPOS, (slots + 1) * sizeof(uint32_t)}};
    for (const auto &[slot, bytes] : need) if (tc_status s = ensure(ctx, B[slot], bytes)) return s;
    const size_t b_keys = V * 3 * sizeof(int32_t), b_counts = V * sizeof(uint32_t), b_sums = V * 3 * sizeof(double), b_cent = V * 3 * sizeof(float);
    int32_t *d_keys = keys; uint32_t *d_counts = counts; double *d_sums = sums; float *d_cent = centroids;
    if (on_host) {
        if (tc_status s = ensure(ctx, B[VM_STAGE], b_sums + b_keys + b_counts + b_cent)) return s;      // the f64 block first: aligned
        char *p = (char *)B[VM_STAGE].p;
        d_sums = sums ? (double *)p : nullptr; p += b_sums;
        d_keys = keys ? (int32_t *)p : nullptr; p += b_keys;
        d_counts = counts ? (uint32_t *)p : nullptr; p += b_counts;
        d_cent = centroids ? (float *)p : nullptr;
    }
    uint64_t *ckeys = (uint64_t *)B[VM_KEYS].p, *ckeys_sorted = (uint64_t *)B[VM_KEYS_SORTED].p;
    uint32_t *cslot = (uint32_t *)B[VM_INDEX].p, *cslot_sorted = (uint32_t *)B[VM_ORDER].p, *flag = (uint32_t *)B[VM_HEAD].p, *pos = (uint32_t *)B[VM_RUNPOS].p;
    {
        ProfScope ps(ctx, "voxel_map_extract");
        hipLaunchKernelGGL(vm_occupied_kernel, dim3(blocks_for(slots)), dim3(256), 0, st, (const uint64_t *)map->keys.p, (uint32_t)slots, flag);
        if (tc_status s = exclusive_scan_u32(ctx, flag, (uint32_t)slots, pos, B[VM_BLOCKSUM])) return s;
        hipLaunchKernelGGL(vm_compact_kernel, dim3(blocks_for(slots)), dim3(256), 0, st, (const uint64_t *)map->keys.p, (uint32_t)slots, (const uint32_t *)pos,
                           ckeys, cslot);
        if (tc_status s = sort_pairs(ctx, ckeys, ckeys_sorted, cslot, cslot_sorted, V, 63u, B[VM_SORT_TEMP])) return s;
        hipLaunchKernelGGL(vm_gather_kernel, dim3(blocks_for(V)), dim3(256), 0, st, (const uint64_t *)ckeys_sorted, (const uint32_t *)cslot_sorted, (uint32_t)V,
                           (const uint32_t *)map->counts.p, (const double *)map->sums.p, d_keys, d_counts, d_sums, d_cent);
    }
    TC_HIP_TRY(ctx, hipGetLastError());
    if (on_host) {
        if (keys) TC_HIP_TRY(ctx, hipMemcpyAsync(keys, d_keys, b_keys, hipMemcpyDeviceToHost, st));
        if (counts) TC_HIP_TRY(ctx, hipMemcpyAsync(counts, d_counts, b_counts, hipMemcpyDeviceToHost, st));
        if (sums) TC_HIP_TRY(ctx, hipMemcpyAsync(sums, d_sums, b_sums, hipMemcpyDeviceToHost, st));
        if (centroids) TC_HIP_TRY(ctx, hipMemcpyAsync(centroids, d_cent, b_cent, hipMemcpyDeviceToHost, st));
    }
    return synced(ctx);
}

static tc_status vm_reset(tc_voxel_map *map) {
    if (tc_status s = vm_clear_table(map->ctx, map->slots, map->keys, map->counts, map->sums)) return s;
    map->n_voxels = 0; map->n_points = 0; map->pending = false;
    return synced(map->ctx);
}

static void vm_free(tc_voxel_map *map) {
    free_buf(map->keys); free_buf(map->counts); free_buf(map->sums);
    recycle(map->ctx, map->counters);
    for (auto &b : map->scratch) recycle(map->ctx, b);
    delete map;
}

}  // namespace tc

using namespace tc;

// ---- entry points (include/threecrate_hip_voxelmap.h) -----------------------------------------------------------------------------
static tc_status vm_check_insert(tc_voxel_map *map, const float *xyz, size_t n, bool *nothing) {
    *nothing = false;
    if (!map) return TC_INVALID_DATA;
    if (n == 0) { *nothing = true; return TC_OK; }
    if (!xyz) return fail(map->ctx, TC_INVALID_DATA, "voxel_map_insert: xyz is NULL");
    return check_point_count(map->ctx, n);
}

static tc_status vm_check_extract(tc_voxel_map *map, size_t *n_voxels) {
    if (!map || !n_voxels) return TC_INVALID_DATA;
    *n_voxels = 0;
    return TC_OK;
}

extern "C" {

tc_status tc_voxel_map_create(tc_context *ctx, const tc_voxel_map_config *config, tc_voxel_map **out) try {
    if (!out) return TC_INVALID_DATA;
    *out = nullptr;
    if (!config) return ctx ? fail(ctx, TC_INVALID_DATA, "voxel_map: config is NULL") : TC_INVALID_DATA;
    if (!(config->voxel_size > 0.0f)) return ctx ? fail(ctx, TC_INVALID_DATA, "voxel_size must be positive") : TC_INVALID_DATA;     // streaming.rs:251-253
    if (config->initial_capacity > TC_VOXEL_MAP_MAX_CAPACITY)
        return ctx ? fail(ctx, TC_UNSUPPORTED, "voxel_map: initial_capacity is above 2^28 slots") : TC_UNSUPPORTED;
    if (!ctx) return TC_INVALID_DATA;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t slots = TC_VOXEL_MAP_MIN_CAPACITY;
    const size_t want = config->initial_capacity ? config->initial_capacity : TC_VOXEL_MAP_DEFAULT_CAPACITY;
    while (slots < want) slots *= 2;
    tc_voxel_map *map = new tc_voxel_map();
    map->ctx = ctx; map->voxel_size = config->voxel_size; map->inv = 1.0f / config->voxel_size; map->slots = slots;
    tc_status s = vm_alloc_table(ctx, slots, map->keys, map->counts, map->sums);
    if (s == TC_OK) s = ensure(ctx, map->counters, 256);
    if (s == TC_OK) s = vm_reset(map);
    if (s != TC_OK) { vm_free(map); return s; }
    *out = map;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

void tc_voxel_map_destroy(tc_voxel_map *map) try {
    if (!map) return;
    (void)hipSetDevice(map->ctx->device);
    (void)hipStreamSynchronize(map->ctx->stream);
    vm_free(map);
} TC_CATCH_VOID

tc_status tc_voxel_map_reset(tc_voxel_map *map) try {
    if (!map) return TC_INVALID_DATA;
    TC_HIP_TRY(map->ctx, hipSetDevice(map->ctx->device));
    return vm_reset(map);
} TC_CATCH_STATUS(map ? map->ctx : nullptr)

size_t tc_voxel_map_size(tc_voxel_map *map) try {
    if (!map) return 0;
    if (hipSetDevice(map->ctx->device) != hipSuccess || vm_settle(map) != TC_OK) return 0;
    return map->n_voxels;
} TC_CATCH_VALUE(0)

uint64_t tc_voxel_map_points(tc_voxel_map *map) try {
    return map ? map->n_points : 0;
} TC_CATCH_VALUE(0)

tc_status tc_voxel_map_insert_device(tc_voxel_map *map, const float *d_xyz, size_t n) try {
    bool nothing;
    if (tc_status s = vm_check_insert(map, d_xyz, n, &nothing)) return s;
    if (nothing) return TC_OK;
    TC_HIP_TRY(map->ctx, hipSetDevice(map->ctx->device));
    return vm_insert_device(map, d_xyz, n);
} TC_CATCH_STATUS(map ? map->ctx : nullptr)

tc_status tc_voxel_map_insert(tc_voxel_map *map, const float *xyz, size_t n) try {
    bool nothing;
    if (tc_status s = vm_check_insert(map, xyz, n, &nothing)) return s;
    if (nothing) return TC_OK;
    tc_context *ctx = map->ctx;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = vm_insert_device(map, (const float *)ctx->in_a.p, n)) return s;
    return synced(ctx);                                         // the staging buffer is free, the map is updated
} TC_CATCH_STATUS(map ? map->ctx : nullptr)

tc_status tc_voxel_map_extract_device(tc_voxel_map *map, int32_t *d_keys, uint32_t *d_counts, double *d_sums, float *d_centroids, size_t capacity,
                                      size_t *n_voxels) try {
    if (tc_status s = vm_check_extract(map, n_voxels)) return s;
    TC_HIP_TRY(map->ctx, hipSetDevice(map->ctx->device));
    return vm_extract(map, d_keys, d_counts, d_sums, d_centroids, capacity, n_voxels, false);
} TC_CATCH_STATUS(map ? map->ctx : nullptr)

tc_status tc_voxel_map_extract(tc_voxel_map *map, int32_t *keys, uint32_t *counts, double *sums, float *centroids, size_t capacity,
                               size_t *n_voxels) try {
    if (tc_status s = vm_check_extract(map, n_voxels)) return s;
    TC_HIP_TRY(map->ctx, hipSetDevice(map->ctx->device));
    return vm_extract(map, keys, counts, sums, centroids, capacity, n_voxels, true);
} TC_CATCH_STATUS(map ? map->ctx : nullptr)

}  // extern "C"
