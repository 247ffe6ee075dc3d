// voxel.hip -- voxel_grid_filter (threecrate-algorithms/src/filtering.rs:38-133): one centroid per
// occupied voxel, f64 accumulation, keys = floor((p - bbox_min) / voxel_size) per axis.
//
// The reference folds the cloud into a HashMap in input order, so every voxel's f64 sum runs in
// ascending original index and the output order is unspecified.  Here: dense voxel grid (x-major
// linear id => output sorted by (kx, ky, kz)), counting sort by voxel id with the arrival-rank
// scatter + stable re-rank of grid.hip (points of a voxel end up in ascending original index), then
// one lane per occupied voxel folds its points in that order in f64: bit-identical centroids.
// Boxes too large for a dense grid, or many points per voxel: group_by_key (grid.hip) instead of the counting sort, the folds of run_fold.h.
// Scratch of both paths and of the range filter: tc_context::vox (enum VoxSlot, tc_internal.h).
#include "tc_internal.h"
#include "run_fold.h"

#include <algorithm>
#include <cmath>

namespace tc {

struct VoxGeom {
    float minx, miny, minz, voxel;
    int gx, gy, gz;
    uint32_t ncell;
};

// voxel coordinates of a point, filtering.rs:96-101: ((p - min) / voxel_size).floor() as i32 (true division, not * 1/voxel), clamped into
// the box.  G: VoxGeom or VoxBits
template <class G>
__device__ __forceinline__ void voxel_coords(const G &v, float x, float y, float z, int &kx, int &ky, int &kz) {
    kx = (int)floorf((x - v.minx) / v.voxel); ky = (int)floorf((y - v.miny) / v.voxel); kz = (int)floorf((z - v.minz) / v.voxel);
    kx = min(max(kx, 0), v.gx - 1); ky = min(max(ky, 0), v.gy - 1); kz = min(max(kz, 0), v.gz - 1);
}

__device__ __forceinline__ uint32_t voxel_id(const VoxGeom &v, float x, float y, float z) {
    int kx, ky, kz;
    voxel_coords(v, x, y, z, kx, ky, kz);
    return ((uint32_t)kx * v.gy + ky) * v.gz + kz;       // x-major: ascending id = (kx, ky, kz) order
}

__global__ void __launch_bounds__(256) vox_hist_kernel(const float *__restrict__ xyz, uint32_t n, VoxGeom v,
                                                      uint32_t *__restrict__ cell_of, uint32_t *__restrict__ hist,
                                                      uint32_t *__restrict__ arrival) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = voxel_id(v, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    cell_of[i] = c;
    arrival[i] = atomicAdd(&hist[c], 1u);
}

__global__ void __launch_bounds__(256) vox_scatter_kernel(const uint32_t *__restrict__ cell_of, uint32_t n,
                                                         const uint32_t *__restrict__ cell_start,
                                                         const uint32_t *__restrict__ arrival, uint32_t *__restrict__ slot) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    slot[cell_start[cell_of[i]] + arrival[i]] = i;
}

// stable order inside the voxel: ascending original index
__global__ void __launch_bounds__(256) vox_rank_kernel(uint32_t n, const uint32_t *__restrict__ cell_of,
                                                      const uint32_t *__restrict__ cell_start,
                                                      const uint32_t *__restrict__ slot, uint32_t *__restrict__ order) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t i = slot[p];
    const uint32_t c = cell_of[i];
    const uint32_t s = cell_start[c], e = cell_start[c + 1];
    uint32_t rank = 0;
    for (uint32_t j = s; j < e; ++j) rank += (slot[j] < i) ? 1u : 0u;
    order[s + rank] = i;
}

__global__ void __launch_bounds__(256) vox_flag_kernel(const uint32_t *__restrict__ cell_start, uint32_t ncell,
                                                      uint32_t *__restrict__ flag) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    flag[c] = (cell_start[c + 1] > cell_start[c]) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) vox_centroid_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ cell_start,
                                                          uint32_t ncell, const uint32_t *__restrict__ order,
                                                          const uint32_t *__restrict__ outpos, float *__restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell) return;
    const uint32_t s = cell_start[c], e = cell_start[c + 1];
    if (e == s) return;
    double sx = 0.0, sy = 0.0, sz = 0.0;          // filtering.rs:108-118
    for (uint32_t j = s; j < e; ++j) {
        const size_t i = order[j];
        sx += (double)xyz[3 * i]; sy += (double)xyz[3 * i + 1]; sz += (double)xyz[3 * i + 2];
    }
    const double inv = 1.0 / (double)(e - s);      // filtering.rs:122-128
    float *o = out + 3 * (size_t)outpos[c];
    o[0] = (float)(sx * inv); o[1] = (float)(sy * inv); o[2] = (float)(sz * inv);
}

// ---- sort path: bounding boxes too large for a dense grid, or many points per voxel ---------------
// key = (kx, ky, kz) packed into bx + by + bz bits; a stable LSD radix sort of (key, original index) leaves the
// voxels in (kx, ky, kz) order and the points of a voxel in ascending original index, like the dense path.
struct VoxBits {
    float minx, miny, minz, voxel;
    int sy, sz;             // shifts: key = kx << sx | ky << sz... (kz in the low bits)
    int gx, gy, gz;
};

__global__ void __launch_bounds__(256) vox_key_kernel(const float *__restrict__ xyz, uint32_t n, VoxBits v,
                                                     uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int kx, ky, kz;
    voxel_coords(v, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], kx, ky, kz);
    keys[i] = ((uint64_t)kx << v.sy) | ((uint64_t)ky << v.sz) | (uint64_t)kz;
    idx[i] = i;
}

// the sort path's two folds (run_fold.h): a record is a point's three coordinates, the sums are f64 (filtering.rs:108-118)
constexpr uint32_t kLongVoxel = 96;     // points; longer voxels go to the wave-per-voxel kernel

// filtering.rs:122-128
__device__ __forceinline__ void vox_store_centroid(const XyzSum &sum, float *__restrict__ out, uint32_t v, uint32_t count) {
    const double inv = 1.0 / (double)count;
    float *o = out + 3 * (size_t)v;
    o[0] = (float)(sum.x * inv); o[1] = (float)(sum.y * inv); o[2] = (float)(sum.z * inv);
}

// one lane per voxel folds the voxel's points in sorted = original order, eight gathers in flight at a time; the long voxels are listed
__global__ void __launch_bounds__(256) vox_centroid_sorted_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ order,
                                                                 const uint32_t *__restrict__ vstart, const uint32_t *__restrict__ n_vox,
                                                                 float *__restrict__ out, uint32_t *__restrict__ long_list, uint32_t list_cap,
                                                                 uint32_t *__restrict__ long_count) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= *n_vox) return;
    const uint32_t s = vstart[v], e = vstart[v + 1];
    if (e - s > kLongVoxel) { append_long_run(long_list, list_cap, long_count, v); return; }
    XyzSum sum;
    fold_run_lane<8>(s, e, [&](uint32_t j) { return load_xyz_point(xyz, order, j); }, [&](const XyzPoint &p) { sum.add(p); });
    vox_store_centroid(sum, out, v, e - s);
}

// Voxels with many points (0.2 m voxels on a depth frame: ~1000 each): one WAVE per voxel, the same bits.
// (32-bit trips, as the kernel was written: right while the call has fewer than 2^32 - 64 points; the entry check admits 48 more)
__global__ void __launch_bounds__(256) vox_centroid_long_kernel(const float *__restrict__ xyz, const uint32_t *__restrict__ order,
                                                               const uint32_t *__restrict__ vstart, const uint32_t *__restrict__ long_list,
                                                               const uint32_t *__restrict__ long_count, float *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    for_each_listed_run(long_list, *long_count, [&](uint32_t v) {
        const uint32_t s = vstart[v], e = vstart[v + 1];
        XyzSum sum;
        fold_run_wave<uint32_t>(s, e, lane, [&](uint32_t j) { return load_xyz_point(xyz, order, j); }, [&](const XyzPoint &p) { sum.add(p); });
        if (lane == 0) vox_store_centroid(sum, out, v, e - s);
    });
}

static tc_status voxel_filter_sorted(tc_context *ctx, const float *d_xyz, size_t n, float voxel, const float mn[3], const double dims[3],
                                     float *d_out, size_t *n_out) {
    hipStream_t st = ctx->stream;
    for (int c = 0; c < 3; ++c)
        if (!(dims[c] < 2097152.0)) return fail(ctx, TC_UNSUPPORTED, "voxel_grid_filter: more than 2^21 voxels along one axis of the bounding box");
    VoxBits v;
    v.minx = mn[0]; v.miny = mn[1]; v.minz = mn[2]; v.voxel = voxel;
    v.gx = (int)dims[0]; v.gy = (int)dims[1]; v.gz = (int)dims[2];
    const int bx = (int)bits_for_value((uint64_t)v.gx - 1), by = (int)bits_for_value((uint64_t)v.gy - 1), bz = (int)bits_for_value((uint64_t)v.gz - 1);
    v.sz = bz; v.sy = by + bz;
    auto &B = ctx->vox;             // (what each slot holds: enum VoxSlot, tc_internal.h)
    const uint32_t n32 = (uint32_t)n;
    const unsigned nb = blocks_for(n);
    const std::pair<VoxSlot, size_t> need[] = {{VOX_KEYS, n * sizeof(uint64_t)}, {VOX_INDEX, n * sizeof(uint32_t)}, {VOX_POS, (n + 2) * sizeof(uint32_t)}};
    for (const auto &[slot, bytes] : need) if (tc_status s = ensure(ctx, B[slot], bytes)) return s;
    uint64_t *keys = (uint64_t *)B[VOX_KEYS].p;
    uint32_t *idx = (uint32_t *)B[VOX_INDEX].p;
    ProfScope ps(ctx, "voxel_grid_filter_sorted");
    hipLaunchKernelGGL(vox_key_kernel, dim3(nb), dim3(256), 0, st, d_xyz, n32, v, keys, idx);
    KeyGroups g;
    if (tc_status s = group_by_key(ctx, keys, idx, n, (unsigned)(bx + by + bz),
                                   GroupBufs{B[VOX_KEYS_SORTED], B[VOX_ORDER], B[VOX_FLAG], B[VOX_POS], B[VOX_START], B[VOX_SORT_TEMP], B[VOX_BLOCKSUM]}, g)) return s;
    uint32_t *outpos = g.runpos, *long_list = g.head;           // the head flags are no longer needed: n words, more than there are long voxels
    TC_HIP_TRY(ctx, hipMemsetAsync(outpos + n + 1, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(vox_centroid_sorted_kernel, dim3(nb), dim3(256), 0, st, d_xyz, g.order, g.rstart, g.n_runs, d_out, long_list, n32, outpos + n + 1);
    hipLaunchKernelGGL(vox_centroid_long_kernel, dim3(1024), dim3(256), 0, st, d_xyz, g.order, g.rstart, (const uint32_t *)long_list,
                       (const uint32_t *)(outpos + n + 1), d_out);
    if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, outpos + n, sizeof(uint32_t))) return s;
    *n_out = pinned_host(ctx)->count;
    return TC_OK;
}

tc_status voxel_filter_device(tc_context *ctx, const float *d_xyz, size_t n, float voxel, float *d_out, size_t *n_out) {
    hipStream_t st = ctx->stream;
    float mn[3], mx[3];
    if (tc_status s = cloud_bbox(ctx, d_xyz, n, mn, mx)) return s;
    for (int c = 0; c < 3; ++c)
        if (!(mn[c] <= mx[c]) || !std::isfinite(mn[c]) || !std::isfinite(mx[c]))
            return fail(ctx, TC_INVALID_DATA, "voxel_grid_filter: non-finite coordinates");
    VoxGeom v;
    v.minx = mn[0]; v.miny = mn[1]; v.minz = mn[2]; v.voxel = voxel;
    double dims[3];
    for (int c = 0; c < 3; ++c) dims[c] = std::floor((double)((mx[c] - mn[c]) / voxel)) + 1.0;
    const double ncd = dims[0] * dims[1] * dims[2];
    // the dense grid pays O(voxels in the box) and a quadratic re-rank inside a voxel: boxes with more than 2^25
    // voxels (0.05 m voxels on a LiDAR sweep) or many points per voxel (0.2 m voxels on a depth frame) are sorted
    if (!(ncd < 33554432.0) || (double)n > 8.0 * ncd) return voxel_filter_sorted(ctx, d_xyz, n, voxel, mn, dims, d_out, n_out);
    v.gx = (int)dims[0]; v.gy = (int)dims[1]; v.gz = (int)dims[2];
    v.ncell = (uint32_t)ncd;
    auto &B = ctx->vox;
    const uint32_t n32 = (uint32_t)n;
    const unsigned nb = blocks_for(n), ncb = blocks_for(v.ncell);
    const size_t u32 = sizeof(uint32_t), nc = v.ncell;
    const std::pair<VoxSlot, size_t> need[] = {{VOX_KEYS, n * u32}, {VOX_KEYS_SORTED, n * u32}, {VOX_INDEX, n * u32}, {VOX_ORDER, n * u32},
                                               {VOX_FLAG, nc * u32}, {VOX_POS, (nc + 1) * u32}, {VOX_START, (nc + 1) * u32}};
    for (const auto &[slot, bytes] : need) if (tc_status s = ensure(ctx, B[slot], bytes)) return s;
    uint32_t *cell_of = (uint32_t *)B[VOX_KEYS].p, *slot = (uint32_t *)B[VOX_KEYS_SORTED].p, *arrival = (uint32_t *)B[VOX_INDEX].p,
             *order = (uint32_t *)B[VOX_ORDER].p, *hist = (uint32_t *)B[VOX_FLAG].p, *cell_start = (uint32_t *)B[VOX_POS].p, *outpos = (uint32_t *)B[VOX_START].p;
    TC_HIP_TRY(ctx, hipMemsetAsync(hist, 0, nc * u32, st));
    ProfScope ps(ctx, "voxel_grid_filter");
    hipLaunchKernelGGL(vox_hist_kernel, dim3(nb), dim3(256), 0, st, d_xyz, n32, v, cell_of, hist, arrival);
    if (tc_status s = exclusive_scan_u32(ctx, hist, v.ncell, cell_start, B[VOX_BLOCKSUM])) return s;
    hipLaunchKernelGGL(vox_scatter_kernel, dim3(nb), dim3(256), 0, st, (const uint32_t *)cell_of, n32, (const uint32_t *)cell_start,
                       (const uint32_t *)arrival, slot);
    hipLaunchKernelGGL(vox_rank_kernel, dim3(nb), dim3(256), 0, st, n32, (const uint32_t *)cell_of, (const uint32_t *)cell_start,
                       (const uint32_t *)slot, order);
    uint32_t *flag = hist;               // the histogram is no longer needed
    hipLaunchKernelGGL(vox_flag_kernel, dim3(ncb), dim3(256), 0, st, (const uint32_t *)cell_start, v.ncell, flag);
    if (tc_status s = exclusive_scan_u32(ctx, flag, v.ncell, outpos, B[VOX_BLOCKSUM])) return s;
    hipLaunchKernelGGL(vox_centroid_kernel, dim3(ncb), dim3(256), 0, st, d_xyz, (const uint32_t *)cell_start, v.ncell, (const uint32_t *)order,
                       (const uint32_t *)outpos, d_out);
    if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, outpos + v.ncell, sizeof(uint32_t))) return s;
    *n_out = pinned_host(ctx)->count;
    return TC_OK;
}

// ---- range_filter (kiss_icp.rs:56-70): keep points with min_r^2 <= |p|^2 <= max_r^2, order preserved ----
__global__ void __launch_bounds__(256) range_flag_kernel(const float *__restrict__ xyz, uint32_t n, float min_sq, float max_sq,
                                                        uint32_t *__restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
    const float r2 = x * x + y * y + z * z;                 // magnitude_squared, no FMA (-ffp-contract=off)
    flag[i] = (r2 >= min_sq && r2 <= max_sq) ? 1u : 0u;
}

tc_status range_filter_device(tc_context *ctx, const float *d_xyz, size_t n, float min_range, float max_range, float *d_out, size_t *n_out) {
    *n_out = 0;
    if (n == 0) return TC_OK;
    if (tc_status s = check_point_count(ctx, n)) return s;
    auto &B = ctx->vox;
    if (tc_status s = ensure(ctx, B[VOX_FLAG], n * sizeof(uint32_t))) return s;
    if (tc_status s = ensure(ctx, B[VOX_POS], (n + 1) * sizeof(uint32_t))) return s;
    uint32_t *flag = (uint32_t *)B[VOX_FLAG].p, *pos = (uint32_t *)B[VOX_POS].p;
    hipStream_t st = ctx->stream;
    const unsigned nb = blocks_for(n);
    ProfScope ps(ctx, "range_filter");
    hipLaunchKernelGGL(range_flag_kernel, dim3(nb), dim3(256), 0, st, d_xyz, (uint32_t)n, min_range * min_range, max_range * max_range, flag);
    if (tc_status s = compact_flagged(ctx, d_xyz, (uint32_t)n, flag, pos, B[VOX_BLOCKSUM], d_out, nullptr)) return s;
    if (tc_status s = read_back(ctx, &pinned_host(ctx)->count, pos + n, sizeof(uint32_t))) return s;
    *n_out = pinned_host(ctx)->count;
    return TC_OK;
}

}   // namespace tc

using namespace tc;

// ---- voxel_grid_filter (filtering.rs:38-133) --------------------------------------------------
static tc_status voxel_validate(tc_context *ctx, size_t n, float voxel, size_t *n_out, bool *empty) {
    *empty = false;
    if (!ctx || !n_out) return TC_INVALID_DATA;
    *n_out = 0;
    if (n == 0) { *empty = true; return TC_OK; }                                              // filtering.rs:42-44
    if (!(voxel > 0.0f)) return fail(ctx, TC_INVALID_DATA, "voxel_size must be positive");    // :46-50
    return check_point_count(ctx, n);
}

extern "C" {
tc_status tc_voxel_grid_filter_device(tc_context *ctx, const float *d_xyz, size_t n, float voxel_size, float *d_out, size_t *n_out) try {
    bool empty;
    if (tc_status s = voxel_validate(ctx, n, voxel_size, n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return voxel_filter_device(ctx, d_xyz, n, voxel_size, d_out, n_out);
} TC_CATCH_STATUS(ctx)

tc_status tc_voxel_grid_filter(tc_context *ctx, const float *xyz, size_t n, float voxel_size, float *out, size_t *n_out) try {
    bool empty;
    if (tc_status s = voxel_validate(ctx, n, voxel_size, n_out, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->out_a, n * 3 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = voxel_filter_device(ctx, (const float *)ctx->in_a.p, n, voxel_size, (float *)ctx->out_a.p, n_out)) return s;
    return stage_out(ctx, out, ctx->out_a.p, *n_out * 3 * sizeof(float));
} TC_CATCH_STATUS(ctx)
}  // extern "C"
