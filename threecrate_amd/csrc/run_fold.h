// run_fold.h -- the device half of grouping by key: fold every run of a sorted list in a fixed sequential order.  Included by the units that
// group (voxel.hip, voxelmap.hip, ndt.hip, mesh.hip, simplify.hip) and by nobody else; the host half is group_by_key (grid.hip).
//   A unit's key kernel writes (key, value); group_by_key sorts them and finds the runs; then
//   append_long_run      the runs longer than the unit's threshold are listed (one guarded append)
//   fold_run_lane        a lane folds a short run: UNROLL gathers in flight, the adds in ascending order
//   for_each_listed_run  the waves of a grid stride over the listed runs
//   fold_run_wave        a wave folds a long run: 64 items loaded at once, every lane runs the same add chain on broadcast values
// Both folds call `add` once per item in ascending position, so a run has the same bits on either road: that order is the contract, and
// this file is its one home.  What a record is, what `add` accumulates and what happens to the sums stay with the unit.
// Everything is a __forceinline__ template over callables: no call, no pointer to code, no state in memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tc {

// the value lane l holds; l is wave-uniform: v_readlane with a scalar lane select
__device__ __forceinline__ float lane_f(float v, int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l)); }
__device__ __forceinline__ uint32_t lane_u(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
// a record of 32-bit words, word by word (a word nobody reads costs nothing)
template <class Rec>
__device__ __forceinline__ Rec lane_record(const Rec &r, int l) {
    static_assert(sizeof(Rec) % sizeof(int) == 0, "a record is made of 32-bit words");
    struct Words { int w[sizeof(Rec) / sizeof(int)]; };
    const Words in = __builtin_bit_cast(Words, r);
    Words out;
#pragma unroll
    for (unsigned k = 0; k < sizeof(Rec) / sizeof(int); ++k) out.w[k] = __builtin_amdgcn_readlane(in.w[k], l);
    return __builtin_bit_cast(Rec, out);
}

// Run r is longer than the caller's threshold: onto the list.  `cap` words is what the list has; a list of items / (threshold + 1) + 1 words
// (or more) holds every such run of `items` items, so the guard never acts there and a reader may take the counter as it is.
__device__ __forceinline__ void append_long_run(uint32_t *__restrict__ list, uint32_t cap, uint32_t *__restrict__ counter, uint32_t r) {
    const uint32_t at = atomicAdd(counter, 1u);
    if (at < cap) list[at] = r;
}

// One lane folds the items [s, e): load(j) brings item j's record (its index, then the gather), add(rec) accumulates it.  UNROLL loads are in
// flight at a time; the adds are sequential, ascending in j.  j + UNROLL stays below 2^32: e is at most kMaxPoints = 2^32 - 16.
template <int UNROLL, class Load, class Add>
__device__ __forceinline__ void fold_run_lane(uint32_t s, uint32_t e, Load load, Add add) {
    static_assert(UNROLL >= 1 && UNROLL <= 16, "");
    uint32_t j = s;
    for (; j + UNROLL <= e; j += UNROLL) {
        decltype(load(j)) rec[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) rec[u] = load(j + u);
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) add(rec[u]);
    }
    for (; j < e; ++j) add(load(j));
}

// One wave folds the items [s, e), 64 per trip: lane `lane` loads item base + lane where that is below e and holds the record's zero value
// otherwise; then add() is called min(64, e - base) times, on the record of lane 0, 1, ... in turn -- by every lane, on broadcast values, so all 64 hold the sums a
// single lane would have.  Lanes past the end contribute nothing: their record is never broadcast.  s, e and the callables' captures are
// wave-uniform.
// Index: the type of `base`.  base + 64 passes 2^32 where e lies within 64 of it, and a 32-bit base would then never reach e: uint64_t is
// right for every e.  uint32_t is the loop counter two older kernels were written with (one scalar add and compare less per trip); a user
// of it says at its call why its e stays below 2^32 - 64.
template <class Index = uint64_t, class Load, class Add>
__device__ __forceinline__ void fold_run_wave(uint32_t s, uint32_t e, uint32_t lane, Load load, Add add) {
    for (Index base = s; base < e; base += 64) {
        const Index j = base + lane;
        decltype(load(0u)) r{};
        if (j < e) r = load((uint32_t)j);
        const int cnt = (int)min((Index)64, (Index)(e - base));
        for (int l = 0; l < cnt; ++l) add(lane_record(r, l));
    }
}

// The waves of the grid (blocks of whole waves) stride over the first `count` entries of the list; body(run) with a wave-uniform run.
// count is at most the list's capacity, far below 2^32 - waves: entry does not wrap.  (The block size as launched, not blockDim.x: every
// block of these grids is whole, and blockDim.x's care for a partial last block costs a vector load in the prologue.)
template <class Body>
__device__ __forceinline__ void for_each_listed_run(const uint32_t *__restrict__ list, uint32_t count, Body body) {
    const uint32_t wpb = (uint32_t)__builtin_amdgcn_workgroup_size_x() >> 6, nwaves = gridDim.x * wpb;
    for (uint32_t entry = blockIdx.x * wpb + (threadIdx.x >> 6); entry < count; entry += nwaves) body(list[entry]);
}

// the record and the sums of the two units that fold points into f64 centroid sums (voxel.hip, voxelmap.hip): item j is point order[j]
struct XyzPoint { float x, y, z; };
struct XyzSum {
    double x = 0.0, y = 0.0, z = 0.0;
    __device__ __forceinline__ void add(const XyzPoint &p) { x = x + (double)p.x; y = y + (double)p.y; z = z + (double)p.z; }
};
__device__ __forceinline__ XyzPoint load_xyz_point(const float *__restrict__ xyz, const uint32_t *__restrict__ order, uint32_t j) {
    const size_t i = order[j];
    return XyzPoint{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
}

// the caller's 12-byte points as 16-byte records (x, y, z, 0): the body of a unit's pack kernel, a thread per point.  CHECK: a coordinate that
// is not finite ORs `bit` into *flags (one atomic per wave that has such a lane)
template <bool CHECK>
__device__ __forceinline__ void pack_xyz_records(const float *__restrict__ xyz, uint32_t n, float4 *__restrict__ rec, uint32_t *__restrict__ flags, uint32_t bit) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
        if constexpr (CHECK) bad = !(fabsf(x) <= 3.4028234664e38f && fabsf(y) <= 3.4028234664e38f && fabsf(z) <= 3.4028234664e38f);
        rec[i] = make_float4(x, y, z, 0.0f);
    }
    if constexpr (CHECK) { if (__ballot(bad) != 0ull && (threadIdx.x & 63u) == 0u) atomicOr(flags, bit); }
}

}  // namespace tc
