// tc_internal.h -- shared host/device declarations of libthreecrate_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <new>
#include <exception>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/threecrate_hip.h"

namespace tc {

// ------------------------------------------------------------------------------------------
// Uniform-grid spatial index over one cloud (replaces KdTree, nearest_neighbor.rs:29-33).
// Cells are ordered x-fastest, so a run of cells along x is ONE contiguous range of the
// cell-sorted point array: a (2R+1)^3 neighbourhood is (2R+1)^2 contiguous spans.
// ------------------------------------------------------------------------------------------
struct GridGeom {
    float minx, miny, minz;     // bbox min (cell origin)
    float maxx, maxy, maxz;     // bbox max
    float h, inv_h;             // cell edge and 1/h
    int   gx, gy, gz;           // cells per axis
    uint32_t ncell;             // gx*gy*gz
    uint32_t n;                 // points indexed
    float cx, cy, cz;           // bbox centre (shift origin for the p2p Kabsch sums)
    int   clamped;              // the box is narrower than the cloud (far outliers): points beyond it live in the
                                // boundary cells, which then extend to infinity for every distance bound
};

// Tiles of TX x TY x TZ cells.  A workgroup owns one tile of QUERIES and stages the tile +
// halo region of the cell-sorted target records into LDS.  The ICP source cloud is sorted by
// the tile-major id (tile index * cells_per_tile + x-fastest local cell) so that the queries of
// one tile are one contiguous range.
struct TileGeom {
    int tx, ty, tz;             // cells per tile along each axis
    int ntx, nty, ntz;          // tiles per axis (grid dims rounded up)
    uint32_t cpt;               // cells per tile
    uint32_t ntiles;
};

struct GridView {
    GridGeom g;
    const float4   *pts;        // cell-sorted points: x, y, z, w = bit pattern of the original index
    const uint32_t *cell_start; // ncell + 1 exclusive prefix sums
    const float    *pts12;      // the same records as packed 12-byte x, y, z (only once the index has served as an ICP target; else null)
};

// device-side ICP state (one per running registration); mirrors the loop variables of
// registration.rs:278-340 / :533-593.
struct IcpState {
    float    q[4];          // current_transform rotation (i j k w)
    float    t[3];          // current_transform translation
    float    prev_mse;      // previous_mse (starts +inf)
    float    mse;           // mse of the last executed iteration
    uint32_t iterations;    // executed iterations
    int32_t  converged;
    int32_t  status;        // tc_status
    int32_t  done;          // converged or failed: later launches exit immediately
    uint32_t n_corr;        // valid pairs of the last executed iteration
    float    conv_thr;
    float    max_dist;      // < 0 : none
    int32_t  kiss;          // KISS-ICP rules (kiss_icp.rs): mse after the update, |H| check, last mse when not converged
    uint32_t refine_total;  // statistics: queries served by the refine pass (sum / max over iterations)
    uint32_t refine_max;
    uint32_t refine_ring_hist[8];   // TC_REFINE_STATS builds only: exit ring of the refine queries
    float    d_ang;         // the last update moved a point x by at most d_ang |x| + d_t (2 |sin(theta / 2)| and |translation| of the delta);
    float    d_t;           // d_ang < 0: the second-neighbour certificate is off (the update is still large: icp.hip compose())
    uint32_t d_run;         // consecutive updates small enough for it: the main pass maintains the bounds from 1 on and USES them from 2 on
    uint32_t searchers;     // lanes of the last main pass that had to search (its rows' spare column, summed by icp_finalize): the certificate's gate
    double   sums[TC_ICP_SUMS_STRIDE];   // packed, fully reduced sums of the current iteration
};

static_assert(offsetof(IcpState, refine_ring_hist) % 8 == 4 && offsetof(IcpState, sums) % 8 == 0,
              "refine_ring_hist[3..4] is ONE 64-bit counter of the statistics instantiation (icp.hip): it must sit on an 8-byte boundary");

// What plane segmentation (plane.hip) brings back from the device in one copy: the winner, or found == 0
struct PlaneOut {
    float    coeff[4];      // a, b, c, d
    uint32_t count, index;  // the winner's score and iteration
    uint32_t found, pad;
};

// NDT registration (ndt.hip).  The loop's device-resident state (ndt_registration.rs:211-252), which is also what a chunk of iterations
// brings back in one copy; and what the voxel build brings back before it sizes its tables.
struct NdtState {
    float    q[4], t[3];        // the pose (rotation i j k w, translation)
    float    rot[9];            // its rotation matrix, row-major (to_rotation_matrix), kept by the finalize kernel for the evaluation
    float    score;             // of the last evaluation
    uint32_t iterations;        // executed iterations
    int32_t  converged;
    int32_t  done;              // converged or the solve failed: later launches return at once
    uint32_t n_hits;            // source points of the last evaluation that fell into a voxel
    float    step_size, epsilon;
    uint32_t pad;
};
static_assert(sizeof(NdtState) == 96, "");
struct NdtBuildOut {
    int32_t  kmin[3], kmax[3];  // key range of the finite target points
    uint32_t n_finite, n_runs, n_voxels, pad[7];
};
static_assert(sizeof(NdtBuildOut) == 64, "");

// TSDF volumes (tsdf.hip): what an integration and an extraction bring back, one word each
struct TsdfOut {
    uint32_t n_updated;         // voxels the last counted integration updated
    uint32_t n_points;          // points of the last extraction's count pass
    uint32_t pad[14];
};
static_assert(sizeof(TsdfOut) == 64, "");

// RANSAC over correspondences (global.hip, the companion library): the loop's device-resident state, folded chunk by chunk, which is also
// what the call brings back in one copy
struct RansacOut {
    float    transform[12];     // the winner's stored R (row-major) and t
    uint32_t count, index;      // its score and iteration
    uint32_t found;             // some candidate with a model scored above 0
    uint32_t exit;              // the winner reached the early-exit count: later chunks leave at once
};
static_assert(sizeof(RansacOut) == 64, "");

// Streaming voxel map (voxelmap.hip, the second companion library): what an insert brings back in one stream synchronisation before it
// touches the table
struct VoxelMapOut {
    uint32_t runs;              // distinct voxels of the chunk (key_runs)
    uint32_t out_of_range;      // some point of the chunk has a key outside [-2^20, 2^20)
    uint32_t n_long;            // runs longer than kVoxelMapLongRun
    uint32_t n_new;             // voxels the PREVIOUS insert added (the device counts them; read with the next call's read-back)
    uint32_t pad[12];
};
static_assert(sizeof(VoxelMapOut) == 64, "");

// Colorization (color.hip, the third companion library): what a counted call brings back in one copy
constexpr int kColorSlices = 16;
struct ColorOut {
    uint32_t slice[kColorSlices];   // coloured points, counted by block b into slice b % kColorSlices; the host adds them up
};
static_assert(sizeof(ColorOut) == 64, "");

// Mesh smoothing (mesh.hip, the fourth companion library): what the adjacency build brings back in one copy
struct MeshOut {
    uint32_t bad_index;         // some face index is >= n_vertices
    uint32_t n_long;            // vertices whose ring exceeds kMeshLongRing
    uint32_t n_entries;         // entries of the CSR (distinct directed pairs)
    uint32_t pad[13];
};
static_assert(sizeof(MeshOut) == 64, "");

// Mesh simplification (simplify.hip, the fifth companion library): what the class stage and the face stage bring back, one copy each
struct SimplifyOut {
    uint32_t flags;             // bit 0: some face index is >= n_vertices; bit 1: some vertex coordinate is not finite
    uint32_t n_long;            // clusters of more than kSimplifyLongCluster members (device-side only: the wave kernel reads it)
    uint32_t n_out_vertices;    // clusters that occur in a surviving face
    uint32_t n_out_faces;       // surviving faces
    uint32_t pad[12];
};
static_assert(sizeof(SimplifyOut) == 64, "");

// Marching cubes (mc.hip, the sixth companion library): what the count stage brings back in one copy
struct McOut {
    uint32_t n_cubes;           // emitting cubes
    uint32_t n_vertices;        // output vertices (per crossing edge of every emitting cube, or per referenced grid edge when welded)
    uint32_t n_faces;           // output triangles
    uint32_t pad[13];
};
static_assert(sizeof(McOut) == 64, "");

// Quadric-error simplification (qem.hip, the seventh companion library): what the set-up, every round and the count stage bring back, one copy each
struct QemOut {
    uint32_t flags;             // bit 0: some face index is >= n_vertices; bit 1: some vertex coordinate is not finite
    uint32_t n_long;            // vertices whose ring exceeds kQemLongRing (device-side only: the wave kernel reads it)
    uint32_t alive;             // faces alive: after the drop of the input's degenerate faces, then after every round
    uint32_t taken;             // edges the last round collapsed
    uint32_t n_out_vertices;    // vertices that occur in a surviving face
    uint32_t pad[11];
};
static_assert(sizeof(QemOut) == 64, "");

// Alpha-shape reconstruction (alpha.hip, the eighth companion library): what the list stage, the count stage and the face stage bring back, one copy each
struct AlphaOut {
    uint32_t flags;             // bit 0: some coordinate is not finite
    uint32_t boundary;          // boundary candidates among the remaining ones
    uint64_t pairs;             // neighbour pairs (i, j) with j > i, over all i
    uint64_t candidates;        // candidates before the cap
    uint32_t faces;             // output faces
    uint32_t pad[9];
};
static_assert(sizeof(AlphaOut) == 64, "");

// Ground segmentation (ground.hip, the ninth companion library): what a call brings back, one word
struct GroundOut {
    uint32_t n_ground;          // points labelled ground (the total of the ground flags' scan)
    uint32_t pad[15];
};
static_assert(sizeof(GroundOut) == 64, "");

// The context's pinned host block (tc_context::pinned; pinned_host() is the host's view, pinned_dev_ptr() the device's), one member per
// region.  A context serves one call at a time, and every entry point that uses a region has synchronised the stream or seen the
// region's flag word before it returns: no region is live across two calls.  What is shared INSIDE a call is said at the member.
constexpr size_t kIcpMaxFlags = 200;            // chunks of one registration that report through a word of their own (run_chunked)
struct PinnedBlock {
    char     reserved[256];         // free
    IcpState icp_staged;            // icp_setup: the initial state, uploaded asynchronously; tc_icp_shard_finish: its read-back (the
                                    // upload is long over by then)
    IcpState icp_result;            // the state after icp_finish_kernel (finish_registration).  NOT the staged slot: the upload of a short
                                    // run that was enqueued in one go may still be pending when the result is prepared
    union {
        // run_chunked: word c = 1 / 2 / 3 once chunk c of the enqueue schedule has run (polled)
        volatile int32_t icp_flags[kIcpMaxFlags];
        // One word copied back and read under a stream synchronisation: the output count of the voxel and range filters, the cluster
        // count, FPFH's fallback count, tc_icp_shard_done.  None of them runs while run_chunked polls: filters, clustering and FPFH
        // return before a registration starts (KISS-ICP, multiscale ICP: filter, THEN icp_run, on one host thread), and a shard
        // handle's loop is driven by the caller, not by run_chunked; run_chunked zeroes word c before it enqueues chunk c.
        uint32_t count;
        // the outlier filters (outlier.hip), read the same way: [0] = kept points, [1] = the bits of the threshold used
        uint32_t filter_out[2];
        // plane segmentation (plane.hip), read the same way: the winner kernel's record, copied back at the end of the call
        PlaneOut plane_out;
    };
    char     pad_flags[1024 - kIcpMaxFlags * sizeof(int32_t)];
    float    bbox[30];              // cloud_bbox: [0..6) exact box, [6..30) sample boxes (the slot once held 8 KiB of per-block partials)
    char     pad_bbox[8192 - 30 * sizeof(float)];
    volatile uint32_t occ[2];       // build_index: [0] = occupied cells, [1] = written (ONE 8-byte word for the device)
    char     pad_occ[56];
    uint32_t big_cell;              // build_index(strict_order): some cell holds more than kRankQuadraticMax points
    char     pad_big[60];
    uint32_t agree;                 // comm_agree: this rank's flag out, the ranks' sum back
    char     pad_agree[60];
    volatile uint32_t bbox_done;    // cloud_bbox: bbox[] is written (polled)
    char     pad_done[60];
    volatile uint32_t bin_max[2];   // build_index, binned placement: [0] = largest bin, [1] = written (ONE 8-byte word for the device)
    char     pad_bin[56];
    NdtBuildOut ndt_build;          // NDT (ndt.hip): the voxel build's key range and counts, copied back and read under a stream synchronisation
    NdtState ndt_state;             // NDT: the loop's state after a chunk of iterations, read the same way.  A region of its own: not in the union
    TsdfOut  tsdf_out;              // TSDF (tsdf.hip): the updated-voxel count of an integration, the point count of an extraction, copied back
                                    // and read under a stream synchronisation.  A region of its own: not in the union
    RansacOut ransac_out;           // RANSAC over correspondences (global.hip): the state after the last fold, copied back and read under a
                                    // stream synchronisation.  A region of its own: not in the union
    VoxelMapOut voxelmap_out;       // streaming voxel map (voxelmap.hip): a chunk's run count, range flag and long-run count, and the new-voxel
                                    // count of the insert before, copied back and read under a stream synchronisation.  A region of its own
    ColorOut color_out;             // colorization (color.hip): the count slices of a counted call, copied back and read under a stream
                                    // synchronisation.  A region of its own
    MeshOut  mesh_out;              // mesh smoothing (mesh.hip): the adjacency build's index flag, long-ring count and entry count, copied
                                    // back and read under a stream synchronisation.  A region of its own
    SimplifyOut simplify_out;       // mesh simplification (simplify.hip): the flags of the device-side checks, then the output counts, copied
                                    // back and read under a stream synchronisation.  A region of its own
    McOut    mc_out;                // marching cubes (mc.hip): the cube, vertex and face counts, copied back and read under a stream
                                    // synchronisation.  A region of its own
    QemOut   qem_out;               // quadric-error simplification (qem.hip): the flags and the first face count, then every round's face count
                                    // and collapses, then the vertex count, copied back and read under a stream synchronisation.  A region of its own
    AlphaOut alpha_out;             // alpha-shape reconstruction (alpha.hip): the finite flag and the pair total, then the candidate total, then the
                                    // boundary and face counts, copied back and read under a stream synchronisation.  A region of its own
    GroundOut ground_out;           // ground segmentation (ground.hip): the ground count, copied back and read under a stream synchronisation.  A
                                    // region of its own
};
constexpr size_t kPinnedBytes = 1 << 16;          // what tc_context_create allocates
// The offsets are the numbers the sites used to spell out.  A new region takes `reserved` or the end of the block; an IcpState that
// grows moves icp_staged down into `reserved` (STATE.md, "Who owns which bytes of the pinned block").
static_assert(offsetof(PinnedBlock, icp_staged) == 256 && offsetof(PinnedBlock, icp_result) == 640 && offsetof(PinnedBlock, icp_flags) == 1024 &&
              offsetof(PinnedBlock, count) == 1024 && offsetof(PinnedBlock, filter_out) == 1024 && offsetof(PinnedBlock, plane_out) == 1024 &&
              sizeof(PlaneOut) <= sizeof(PinnedBlock::icp_flags) && offsetof(PinnedBlock, bbox) == 2048 && offsetof(PinnedBlock, occ) == 2048 + 8192 &&
              offsetof(PinnedBlock, big_cell) == 2048 + 8192 + 64 && offsetof(PinnedBlock, agree) == 2048 + 8192 + 128 &&
              offsetof(PinnedBlock, bbox_done) == 2048 + 8192 + 192 && offsetof(PinnedBlock, bin_max) == 2048 + 8192 + 256 &&
              offsetof(PinnedBlock, ndt_build) == 2048 + 8192 + 320 && offsetof(PinnedBlock, ndt_state) == 2048 + 8192 + 384 &&
              offsetof(PinnedBlock, tsdf_out) == 2048 + 8192 + 480 && offsetof(PinnedBlock, ransac_out) == 2048 + 8192 + 544 &&
              offsetof(PinnedBlock, voxelmap_out) == 2048 + 8192 + 608 && offsetof(PinnedBlock, color_out) == 2048 + 8192 + 672 &&
              offsetof(PinnedBlock, mesh_out) == 2048 + 8192 + 736 && offsetof(PinnedBlock, simplify_out) == 2048 + 8192 + 800 &&
              offsetof(PinnedBlock, mc_out) == 2048 + 8192 + 864 && offsetof(PinnedBlock, qem_out) == 2048 + 8192 + 928 &&
              offsetof(PinnedBlock, alpha_out) == 2048 + 8192 + 992 && offsetof(PinnedBlock, ground_out) == 2048 + 8192 + 1056,
              "a region of the pinned block has moved");
static_assert(offsetof(PinnedBlock, icp_result) - offsetof(PinnedBlock, icp_staged) >= sizeof(IcpState) &&
              offsetof(PinnedBlock, icp_flags) - offsetof(PinnedBlock, icp_result) >= sizeof(IcpState),
              "an IcpState slot of the pinned block is too small: the staged state would run into the result, the result into the chunk flags");
static_assert(sizeof(PinnedBlock::icp_flags) == kIcpMaxFlags * sizeof(int32_t) &&
              offsetof(PinnedBlock, icp_flags) + sizeof(PinnedBlock::icp_flags) <= offsetof(PinnedBlock, bbox), "the chunk flags run into the bounding box");
static_assert(sizeof(PinnedBlock) <= kPinnedBytes, "the pinned block outgrew its allocation");
constexpr int kIcpBlock = 256;
// TSDF volumes (tsdf.hip): a wave owns a run of kTsdfRun voxels (cubes) along x of one (y, z) row -- one contiguous 512-byte run of the
// state --, a block kTsdfBlock / kTsdfRun consecutive runs; a cube block of the extraction is kTsdfRun x kTsdfBlock / kTsdfRun (runs) cubes
constexpr int kTsdfBlock = 256, kTsdfRun = 64;
constexpr size_t kTsdfMaxVoxels = (size_t)1 << 28;   // 12 points per cube in a 32-bit scan
// padding behind the sorted records / the prefix sums: the ICP search reads a few entries past a
// span (4-wide steps) and 16-byte windows of cell_start without clamping
constexpr size_t kPtsPad = 4, kCellStartPad = 4;
constexpr size_t kCellStartFront = 4;            // zero entries in front of the prefix sums (16-byte aligned start)
constexpr uint32_t kRankQuadraticMax = 1u << 20; // cells up to this population are re-ranked by original index in O(m^2) (rerank_kernel; 65536 until round 4)
constexpr int kMaxPartialBlocks = 1024;         // plan_launch: one round of 4 blocks per CU
// clouds from this size on get the occupancy-adapted cell edge (one host round trip + possibly a rebuild)
constexpr uint32_t kAdaptMinPoints = 1u << 18;   // 2^17: a 230 k-point depth frame gets slower (normals 0.67 -> 0.71 ms, 10 ICP iterations 1.5 -> 2.8 ms)

// ---- device helpers -----------------------------------------------------------------------
#if defined(__HIPCC__)
__device__ __forceinline__ uint32_t tile_major_id(const TileGeom &t, int cx, int cy, int cz) {
    const int ax = cx / t.tx, ay = cy / t.ty, az = cz / t.tz;
    const int lx = cx - ax * t.tx, ly = cy - ay * t.ty, lz = cz - az * t.tz;
    const uint32_t tile = ((uint32_t)az * t.nty + ay) * t.ntx + ax;
    return tile * t.cpt + ((uint32_t)lz * t.ty + ly) * t.tx + lx;
}
__device__ __forceinline__ float d2_nc(float ax, float ay, float az, float bx, float by, float bz) {
    // nearest_neighbor.rs:162-167: (a - b) per component, dx*dx + dy*dy + dz*dz, left to right,
    // NO fma contraction (the library is built with -ffp-contract=off).
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ int cell_coord(float v, float mn, float inv_h, int g) {
    float f = (v - mn) * inv_h;
    int c = (f >= 0.0f) ? (int)f : 0;          // NaN -> 0
    return c < g ? c : g - 1;
}
// nalgebra UnitQuaternion * Point3 (q = i j k w): t2 = (qv x p) * 2; p' = (t2 * w + qv x t2) + p; then + translation
__device__ __forceinline__ void isometry_apply(const float q[4], const float t[3], float x, float y, float z,
                                               float &ox, float &oy, float &oz) {
    float tx = (q[1] * z - q[2] * y) * 2.0f;
    float ty = (q[2] * x - q[0] * z) * 2.0f;
    float tz = (q[0] * y - q[1] * x) * 2.0f;
    float cx = q[1] * tz - q[2] * ty;
    float cy = q[2] * tx - q[0] * tz;
    float cz = q[0] * ty - q[1] * tx;
    ox = ((tx * q[3] + cx) + x) + t[0];
    oy = ((ty * q[3] + cy) + y) + t[1];
    oz = ((tz * q[3] + cz) + z) + t[2];
}
// point i of a flagged cloud to its scanned position o: the store of every compaction (grid.hip, outlier.hip); either output may be null
__device__ __forceinline__ void store_compacted(const float *__restrict__ xyz, uint32_t i, uint32_t o, float *__restrict__ out_xyz,
                                                uint32_t *__restrict__ out_index) {
    if (out_xyz) {
        out_xyz[3 * (size_t)o] = xyz[3 * (size_t)i]; out_xyz[3 * (size_t)o + 1] = xyz[3 * (size_t)i + 1]; out_xyz[3 * (size_t)o + 2] = xyz[3 * (size_t)i + 2];
    }
    if (out_index) out_index[o] = i;
}
// a 12-byte record as one value (raw_buffer_load_b96)
typedef float f32x3 __attribute__((ext_vector_type(3)));
// raw buffer descriptor over a whole allocation (no range check: 4 GiB window): buffer loads take a
// 32-bit byte offset per lane (no 64-bit address arithmetic) and accept dword-aligned 16-byte reads
__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, 0xFFFFFFFF, 0x00020000);
}
#endif

// ---- host side ----------------------------------------------------------------------------
struct DevBuf {
    void  *p = nullptr;
    size_t cap = 0;
};

// A function-local temporary: goes where ensure() takes a DevBuf &; its block is released (hipFree, not the context's pool) when the scope ends,
// on every return and when an exception unwinds into the entry point's handler.  Members of handles and of the context stay plain DevBufs.
struct ScopedBuf : DevBuf {
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf &) = delete; ScopedBuf &operator=(const ScopedBuf &) = delete;
    ~ScopedBuf() { if (p) (void)hipFree(p); }
};

struct KernelTimer {
    std::string name;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    uint64_t launches = 0;
    double   total_ms = 0.0;
    double   min_ms = 1e300, max_ms = 0.0;
};

// One indexed cloud living in device memory.
struct DeviceIndex {
    GridGeom geom{};
    TileGeom tile{};    // only meaningful for a tile-major (query-side) ordering
    float exact_min[3] = {0, 0, 0}, exact_max[3] = {0, 0, 0};   // the cloud's exact box (geom may be clamped)
    DevBuf pts;         // float4 * n   (cell-sorted, w = original index bits)
    DevBuf cell_start;  // u32 * (ncell+1)
    DevBuf normals;     // float4 * n   (cell-sorted target normals; optional)
    DevBuf vor;         // float4 * n   (ICP target: x, y, z + inscribed-ball bound, icp_target_nn_bound_kernel; optional)
    bool vor_valid = false;     // vor belongs to the current contents of pts (build_index resets it)
    DevBuf pts12;       // float * 3 (n + 16): the sorted records again as packed 12-byte x, y, z -- the ICP candidate loop reads four
                        // of them with THREE 16-byte reads (made by icp_setup when the index first serves as an ICP target)
    bool pts12_valid = false;   // (build_index resets it)
    uint32_t occ_host = 0;      // occupied cells of the final grid, when the build read them back (edge adaptation: clouds of >= 2^18 points)
    bool occ_host_valid = false;
    DevBuf cell_of;     // u32 * n      (scratch: cell id per original point)
    DevBuf slot;        // u32 * n      (scratch: atomic scatter order)
    DevBuf arrival;     // u32 * n      (scratch: arrival rank of a point inside its cell)
    DevBuf fill;        // u32 * ncell  (scratch: histogram / fill counters)
    DevBuf blocksum;    // u32 * nblocks (scan scratch)
};
// What a caller asks of build_index: filled by named assignment, everything else at its default (the grids that recur: knn_grid, ball_grid)
struct IndexSpec {
    float cell_factor = 0.0f;                   // cell edge = cell_factor x the spacing of n points filling the box's volume ...
    float min_cell_edge = 0.0f;                 // ... and at least this (0: no minimum)
    float target_ppo = 0.0f;                    // > 0: points per OCCUPIED cell wanted; a cloud of >= 2^18 points is read back and re-gridded towards it
    const GridGeom *reuse_geom = nullptr;       // index into THIS grid (the ICP source in its target's), no box pass
    const IcpState *state_transform = nullptr;  // device: a point's key is taken after this state's transform (the records keep the input's coordinates)
    const TileGeom *tile_major = nullptr;       // tile-major key order (the ICP source, a block's queries contiguous)
    bool strict_order = false;                  // the same order on every rank, also inside a cell of more than kRankQuadraticMax points (one host round trip)
};
// cells further than this many rings from a query's (clamped) cell hold no point of its ball
__host__ __device__ inline int ball_rings(const GridGeom &g, float radius) {
    const int gyz = g.gy > g.gz ? g.gy : g.gz;
    return (int)fminf(ceilf(radius * g.inv_h) + 1.0f, (float)(g.gx > gyz ? g.gx : gyz));
}
// The buffers of a DeviceIndex, each named ONCE: what only a build needs, and all of them (free_index, recycle_index, the scratch
// drop of a finished search index).  A new DevBuf member goes into one of the two lists.
template <class F> void for_each_scratch_buf(DeviceIndex &ix, F f) { for (DevBuf *b : {&ix.cell_of, &ix.slot, &ix.arrival, &ix.fill, &ix.blocksum}) f(*b); }
template <class F> void for_each_buf(DeviceIndex &ix, F f) {
    for (DevBuf *b : {&ix.pts, &ix.cell_start, &ix.normals, &ix.vor, &ix.pts12}) f(*b);
    for_each_scratch_buf(ix, f);
}

// Scratch slots of tc_context::clu (cluster.hip).  u32 * n each unless said otherwise.
enum CluSlot {
    CLU_PARENT, CLU_SIZE, CLU_MIN_INDEX,    // union-find parent; component size and smallest original index of a root
    CLU_FLAG, CLU_POS,                      // qualifying root flag; its exclusive prefix sum (n + 1)
    CLU_KEYS,                               // TWO element types: u64 keys | sorted keys of the rank sort (2n), then u32 keys | sorted keys of the member sort
    CLU_ROOTS,                              // roots | sorted roots of the rank sort (2n), then the member sort's original indices (first n)
    CLU_RANK_OF, CLU_SIZES,                 // rank of a qualifying root; sizes in rank order | their prefix sum (2n + 1)
    CLU_LABELS, CLU_SORT_TEMP, CLU_COMP,    // labels when the caller passes none; rocPRIM's temporary storage (bytes); final root of every point
    CLU_SLOTS
};
// Scratch slots of tc_context::fpfh (fpfh.hip)
enum FpfhSlot {
    FPFH_XYZ, FPFH_SPFH, FPFH_MODE,                 // positions (n x 3); SPFH rows in sorted order; mode (u32 * n)
    FPFH_FB_POS, FPFH_FB_XYZ, FPFH_FB_COUNT,        // fallback queries: sorted positions (u32 * n), positions (n x 3), their count (4 x u32)
    FPFH_SORTED_OF,                                 // sorted position of every original index (u32 * n)
    FPFH_KNN_IDX, FPFH_KNN_DIST, FPFH_KNN_COUNT,    // k-NN lists of one chunk of fallback queries
    FPFH_SLOTS
};

// Scratch slots of tc_context::vox (voxel.hip): the voxel filter's dense path (counting sort over the box's `cells` voxels), its sort path
// (sort_pairs + key_runs over n keys) and the range filter.  u32 * n each unless said otherwise.
enum VoxSlot {
    VOX_KEYS,           // dense: voxel id of every point; sort: TWO element types, here packed u64 keys (u64 * n)
    VOX_KEYS_SORTED,    // dense: the points in atomic scatter order; sort: the sorted keys (u64 * n)
    VOX_INDEX,          // dense: arrival rank of a point inside its voxel; sort: the original indices that go into the sort
    VOX_ORDER,          // both: original indices voxel by voxel, ascending inside a voxel
    VOX_FLAG,           // dense: histogram, then occupied-voxel flags (cells); sort: run heads, then the list of long voxels; range: keep flags
    VOX_POS,            // dense: first point of every voxel (cells + 1); sort: run number of every sorted position (n + 2: [n] = voxels,
                        // [n + 1] = long-voxel counter); range: output positions (n + 1, [n] = points kept)
    VOX_START,          // dense: output slot of every voxel (cells + 1, [cells] = voxels); sort: first sorted position of every run (n + 1)
    VOX_SORT_TEMP,      // sort: rocPRIM's temporary storage (bytes)
    VOX_BLOCKSUM,       // all three: the scan's block sums (exclusive_scan_u32)
    VOX_SLOTS
};

}  // namespace tc

struct tc_context {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string last_error;
    int profiling = 0;          // 0 off, 1 every kernel, 2 only the dominant kernel, every 17th launch
    uint32_t prof_tick = 0;
    std::vector<tc::KernelTimer> timers;
    std::vector<hipEvent_t> event_pool;
    // device blocks given back by destroyed handles (tc_cloud, tc_search_index), reused by the next allocation of a similar
    // size: a handle per frame must not cost a hipMalloc / hipFree pair per buffer per frame (milliseconds)
    std::vector<tc::DevBuf> pool;
    size_t pool_bytes = 0;
    size_t pool_largest = 0;                // largest block ever parked: the pool's cap is a multiple of it (api.hip: recycle)
    hipEvent_t order_event = nullptr;       // tc_context_wait_stream
    hipEvent_t release_event = nullptr;     // tc_stream_wait_context
    std::vector<hipEvent_t> chunk_events;   // hipEventDisableTiming events of the ICP loop's chunk polling, reused across calls
    // host entry points: the caller's source (+ normals) are uploaded on a second stream while the context's stream indexes the
    // target; upload_pending = the context's stream has to wait for upload_event before it touches them (icp_setup does)
    hipStream_t copy_stream = nullptr;
    hipEvent_t upload_event = nullptr;
    bool upload_pending = false;
    bool upload_used_copy_stream = false;   // some upload of the current call went to the copy stream (small ones do not)

    // persistent (grow-only) device buffers, reused across calls
    tc::DeviceIndex tgt_index;      // target / normals cloud
    tc::DeviceIndex src_index;      // source ordered by target cell (ICP)
    tc::DevBuf in_a, in_b, in_c;    // staged host inputs
    tc::DevBuf out_a;               // staged outputs
    tc::DevBuf bbox;                // 6 x u32 (ordered-int encoded floats)
    tc::DevBuf state;               // IcpState
    tc::DevBuf partials;            // double * kMaxPartialBlocks * TC_ICP_SUMS_STRIDE
    tc::DevBuf corr;                // u32 * n_source
    tc::DevBuf gicp_src_cov;        // GICP: source covariances in the sorted source order (2 float4 per point)
    tc::DevBuf icp_wsrc;            // float4 * n_source: the ICP loop's working copy of the ordered source: x, y, z + the position of the
                                    // current match in w (one 16-byte read per point and iteration instead of record + match)
    tc::DevBuf dbg_times;           // TC_DEBUG & 1024: per-block stamps of the main pass
    tc::DevBuf overflow;            // scratch (build_index, strict_order: the sorted keys of the re-sort, u32 * n)
    tc::DevBuf build_tmp;           // index build: the records in arrival order, before the in-cell re-rank (float4 * n)
    tc::DevBuf normals_hard;        // normals: count + positions of the points handed to the wave-per-point kernel
    unsigned long long stat_indexed_points = 0, stat_index_builds = 0;   // tc_debug_counter
    // search statistics of the ICP main pass, summed over the calls made in profiling mode 3 (tc_profile_enable(ctx, 3)):
    // iterations, wave trips, trips without a search, searches, candidate steps needed, candidate steps taken (slowest lanes)
    unsigned long long stat_icp[6] = {0, 0, 0, 0, 0, 0};
    bool icp_cert = false;          // run_chunked: the chunks being enqueued run the certificate's instantiation of the main pass
    bool icp_cert_hint = false;     // ... and what the context's previous registration ended with (the next one starts with it)
    bool normals_hard_clean = false; // its header (count, exit ticket) is known to be zero: the last serving launch went through
    tc::DevBuf vox[tc::VOX_SLOTS];  // voxel and range filter scratch (voxel.hip): keys, orders, flags, positions, run starts, sort temporary
    tc::DevBuf clu[tc::CLU_SLOTS];  // cluster extraction scratch (cluster.hip): union-find parents, per-root statistics, ranks, sort buffers
    tc::DevBuf fpfh[tc::FPFH_SLOTS]; // FPFH scratch (fpfh.hip): positions, SPFH rows, modes, fallback lists, k-NN lists
    tc::DevBuf fpfh_np;             // FPFH from xyz: the estimated normals (n x 6) between the two stages
    void *pinned = nullptr;         // pinned host scratch of tc::kPinnedBytes, laid out as a tc::PinnedBlock (tc::pinned_host)
    void *pinned_dev = nullptr;     // the device's address of the same block
};
// Every device buffer the context owns, named ONCE (tc_context_destroy): a new DevBuf member goes in here, a new vox / clu / fpfh slot into its enum.
template <class F> void for_each_buf(tc_context &c, F f) {
    for (tc::DeviceIndex *ix : {&c.tgt_index, &c.src_index}) tc::for_each_buf(*ix, f);
    for (auto &b : c.vox) f(b);
    for (auto &b : c.clu) f(b);
    for (auto &b : c.fpfh) f(b);
    for (tc::DevBuf *b : {&c.fpfh_np, &c.in_a, &c.in_b, &c.in_c, &c.out_a, &c.bbox, &c.state, &c.partials, &c.corr, &c.gicp_src_cov,
                          &c.overflow, &c.normals_hard, &c.build_tmp, &c.dbg_times, &c.icp_wsrc}) f(*b);
}

struct tc_comm {
    tc_context *ctx = nullptr;
    int rank = 0, nranks = 1;
    void *nccl = nullptr;               // ncclComm_t (RCCL), or null
    bool own_nccl = false;
    tc_host_collective_fn host_fn = nullptr;
    void *host_user = nullptr;
    void *agree_word = nullptr;         // one device u32: comm_agree
};

namespace tc {

// error plumbing
tc_status fail(tc_context *ctx, tc_status st, const std::string &msg);
tc_status fail_nothrow(tc_context *ctx, tc_status st, const char *msg) noexcept;
void fault_point(const char *site);       // TC_FAULT: test-only fault injection (api.hip)
// No C++ exception crosses the C ABI (threecrate-core/src/error.rs:7-28: every failure is an Error value; unwinding into a Rust or C
// caller is undefined behaviour): every extern "C" entry point with a body that can allocate is a function-try-block closed by one
// of these, and every thread body catches for itself.
#define TC_CATCH_STATUS(CTX)                                                                                            \
    catch (const std::bad_alloc &) { return tc::fail_nothrow((CTX), TC_GPU, "out of host memory"); }                    \
    catch (const std::exception &e_) { return tc::fail_nothrow((CTX), TC_GPU, e_.what()); }                             \
    catch (...) { return tc::fail_nothrow((CTX), TC_GPU, "unknown C++ exception"); }
#define TC_CATCH_VOID catch (...) { }
#define TC_CATCH_VALUE(V) catch (...) { return V; }
#define TC_HIP_TRY(ctx, expr)                                                                  \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return tc::fail((ctx), TC_GPU, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

tc_status ensure(tc_context *ctx, DevBuf &b, size_t bytes);
// limits of the 32-bit indices and of the k-NN list kernels; the point-count check of every entry point
constexpr size_t kMaxPoints = 0xFFFFFFF0ull, kMaxK = 2048;
inline tc_status check_point_count(tc_context *ctx, size_t a, size_t b = 0) {
    return (a >= kMaxPoints || b >= kMaxPoints) ? fail(ctx, TC_UNSUPPORTED, "more than 2^32 points") : TC_OK;
}
// host -> device on the context's copy stream (created on first use), followed by tc::uploads_issued(): the context's stream
// waits for everything issued so far the next time tc::wait_uploads is called
tc_status upload_async(tc_context *ctx, void *d_dst, const void *h_src, size_t bytes);
tc_status uploads_issued(tc_context *ctx);
tc_status wait_uploads(tc_context *ctx);
// Device -> host words without a copy kernel or a stream synchronisation: a kernel stores into the context's pinned (host-coherent)
// block through its device address and raises a flag word there last (system scope); the host spins on the flag -- with a
// hipStreamQuery now and then, never on a dead device.  pinned_host: the block as the host addresses it; pinned_dev_ptr: the
// device's view of a host address inside it, pinned_dev_ptr(ctx, &pinned_host(ctx)->member).
inline PinnedBlock *pinned_host(tc_context *ctx) { return static_cast<PinnedBlock *>(ctx->pinned); }
void *pinned_dev_ptr(tc_context *ctx, const void *host_addr);
bool pinned_poll_enabled();       // TC_NO_PINNED_POLL=1: copies + stream synchronisations as before round 4 (A/B)
tc_status wait_pinned_word(tc_context *ctx, volatile uint32_t *word, const char *what);
// a few words into a member of the pinned block, the stream drained, the last launch error asked for; then read pinned_host(ctx)->member
tc_status read_back(tc_context *ctx, void *host_dst, const void *dev_src, size_t bytes);
// a host entry point's input: room in a staging buffer of the context and the copy enqueued; its end: the stream drained, [the result copied back first]
tc_status stage_in(tc_context *ctx, DevBuf &b, const void *h_src, size_t bytes);
tc_status synced(tc_context *ctx);
tc_status stage_out(tc_context *ctx, void *h_dst, const void *d_src, size_t bytes);
// hand a block back to the context's pool (the caller has made sure no work in flight uses it)
void recycle(tc_context *ctx, DevBuf &b);

// profiling scope: records hipEvents around one kernel launch on ctx->stream.
// A `dominant` scope (the ICP main pass: the kernel of the bench line's roofline) hands its two events to the launch itself
// (hipExtLaunchKernelGGL(.., e0, e1, ..): they take the kernel's own start and end stamps, no marker packets on the stream -- what
// rocprofv3's kernel trace reads; events recorded AROUND the launch measured 2.3 us more than the kernel ran and put a bubble on
// either side of it): the launch site tests active() and launches through launch_timed().
struct ProfScope {
    tc_context *ctx; int idx = -1; hipEvent_t e0 = nullptr, e1 = nullptr; bool ext = false;
    ProfScope(tc_context *c, const char *name, bool dominant = false);
    ~ProfScope();
    bool active() const { return idx >= 0; }
};

// grid.hip
tc_status build_index(tc_context *ctx, DeviceIndex &ix, const float *d_xyz, size_t n, const IndexSpec &spec);
TileGeom make_tiles(const GridGeom &g, int tx, int ty, int tz);
tc_status gather_normals(tc_context *ctx, DeviceIndex &ix, const float *d_normals, size_t stride);
GridView view_of(const DeviceIndex &ix);
// A kernel that judges distances to cell boxes has two instantiations: with a clamped box (GridGeom::clamped) the boundary cells
// are open on the outer side (costs 4 % on the gap tests).  One place picks:
//   with_clamped(gv, [&](auto ext) { hipLaunchKernelGGL((some_kernel<decltype(ext)::value>), ...); });
template <class F> void with_clamped(const GridView &gv, F launch) {
    if (gv.g.clamped) launch(std::true_type{});
    else launch(std::false_type{});
}

// grid.hip: the steps every unit shares
tc_status exclusive_scan_u32(tc_context *ctx, const uint32_t *d_in, uint32_t n, uint32_t *d_out /* n+1 */, DevBuf &blocksum, uint32_t *occ_out = nullptr,
                             unsigned long long *occ_host = nullptr);
tc_status cloud_bbox(tc_context *ctx, const float *d_xyz, size_t n, float mn[3], float mx[3]);
// flag -> scan -> compact: pos (n + 1 words) = the prefix sums of flag, pos[n] the number kept; the flagged points and / or their indices in input order
tc_status compact_flagged(tc_context *ctx, const float *d_xyz, uint32_t n, const uint32_t *d_flag, uint32_t *d_pos, DevBuf &blocksum, float *d_out_xyz,
                          uint32_t *d_out_index);

// bits that hold 0..v, at least 1 (a range of dim values per axis: v = dim - 1)
unsigned bits_for_value(uint64_t v);
// stable LSD radix sort of (key, value) on key bits [0, end_bit); `temp` grows to rocPRIM's temporary storage.  Instantiated for u64 and u32 keys
template <class K>
tc_status sort_pairs(tc_context *ctx, const K *keys, K *keys_out, const uint32_t *vals, uint32_t *vals_out, size_t n, unsigned end_bit, DevBuf &temp);
// runs of equal keys in a sorted list of n > 0 keys: head[p] = 1 where a run begins; runpos = its exclusive scan (n + 1 words, runpos[n] = R, the number of runs);
// rstart[r] = first position of run r, rstart[R] = n (R + 1 <= n + 1 words)
tc_status key_runs(tc_context *ctx, const uint64_t *keys_sorted, uint32_t n, uint32_t *head, uint32_t *runpos, uint32_t *rstart, DevBuf &blocksum);
// Grouping by key, the host half (the device half: run_fold.h): the n > 0 (key, value) pairs a unit's key kernel has written are sorted on key
// bits [0, key_bits) and their runs found -- sort_pairs, then key_runs, in buffers that stay with their owner (the context's slots, a handle's
// scratch, a call's ScopedBufs) and are grown here: for max(n, room) items, so a call that groups twice can size them once.
struct GroupBufs { DevBuf &keys_sorted, &vals_sorted, &head, &runpos, &rstart, &sort_temp, &blocksum; };
struct KeyGroups {
    const uint64_t *keys_sorted;    // n
    const uint32_t *order;          // n: the values, run by run, in input order inside a run (the sort is stable)
    uint32_t *head, *runpos;        // n | n + 1, as key_runs leaves them; runpos[n] = R.  (The heads are often overwritten next: a unit's list)
    const uint32_t *rstart;         // R + 1 <= n + 1
    const uint32_t *n_runs;         // the device address of R (runpos + n)
};
tc_status group_by_key(tc_context *ctx, const uint64_t *keys, const uint32_t *vals, size_t n, unsigned key_bits, const GroupBufs &b, KeyGroups &g, size_t room = 0);
// blocks of 256 threads that cover n items
inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

// voxel.hip
tc_status voxel_filter_device(tc_context *ctx, const float *d_xyz, size_t n, float voxel, float *d_out, size_t *n_out);
tc_status range_filter_device(tc_context *ctx, const float *d_xyz, size_t n, float min_range, float max_range, float *d_out, size_t *n_out);

// cluster.hip: labels / members / offsets of a validated call (n >= 1, tol * tol finite or NaN); device pointers, n_clusters on the host
tc_status cluster_extract_device(tc_context *ctx, const float *d_xyz, size_t n, float tol, size_t min_size, size_t max_size,
                                 uint32_t *d_labels, uint32_t *d_members, uint64_t *d_offsets, size_t *n_clusters);

// fpfh.hip: descriptors of a validated call (n >= 1, k <= 2047); d_np6 = n x 6 (position, normal), d_out = n x 33, device pointers
tc_status fpfh_device(tc_context *ctx, const float *d_np6, size_t n, float radius, size_t k, float *d_out);

// outlier.hip: validated calls (n >= 1); device pointers, each output optional; n_out / threshold_used on the host
tc_status sor_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k, bool with_threshold, float param, float *d_out_xyz,
                     uint32_t *d_kept_index, float *d_mean, size_t *n_out, float *threshold_used);
tc_status radius_outlier_device(tc_context *ctx, const float *d_xyz, size_t n, float radius, size_t min_neighbors, float *d_out_xyz,
                                uint32_t *d_kept_index, size_t *n_out);

// plane.hip: a validated call (n >= 3, 1 <= n_samples <= 2^20); device pointers, d_samples null = the seeded generator from
// state0, d_inlier_index optional; coefficients / n_inliers / best_iteration on the host
tc_status plane_segment_device(tc_context *ctx, const float *d_xyz, size_t n, float threshold, const uint32_t *d_samples, size_t n_samples,
                               uint64_t state0, float *coefficients, uint32_t *d_inlier_index, size_t *n_inliers, uint32_t *best_iteration);

// normals.hip
tc_status launch_normals(tc_context *ctx, const DeviceIndex &ix, const float *d_xyz, const tc_normal_config &cfg,
                         const float vp[3], float *d_out6, size_t p_begin = 0, size_t p_end = (size_t)-1, bool slice_out = false,
                         float4 *d_sorted_nrm = nullptr, float4 *d_vor = nullptr);
// api.hip: index (into `ix`) + normals of a device-resident cloud
tc_status normals_on_index(tc_context *ctx, DeviceIndex &ix, bool build, float cell_factor_override, const float *d_xyz, size_t n,
                           const tc_normal_config *cfg, float *d_out6, size_t p_begin, size_t p_end, bool slice_out, float4 *d_sorted_nrm,
                           bool with_bounds = false);
float normals_cell_factor(size_t k, bool large);
float normals_target_ppo(size_t k);
// the grid of launch_knn's callers for lists of list_len entries (the k-NN exports, GICP's covariances, the statistical outlier filter)
IndexSpec knn_grid(size_t list_len);
// the grid of a ball walk: cell edge max(0.5 x volume spacing, radius / 2) -- the ball spans ~5 cells per axis, pruned to the rows it reaches.
// A radius whose square is NaN (finite_only: or infinite) has no such ball: the volume-based edge alone, no adaptation
IndexSpec ball_grid(float radius, bool finite_only);
// cell-edge factor of the ICP target grid (build_index's cell_factor): ~1.45 pts/cell, ring 1 exact for ~99.8 % of uniform queries.
// Scanned again after the main / refine split (50-iteration ICP, 1 M points): 0.8 -> 6.55 ms, 0.9 -> 5.55, 1.0 -> 5.00,
// 1.13 -> 4.75, 1.25 -> 4.72, 1.4 -> 4.72 (flat: the main pass grows as the refine pass shrinks)
constexpr float kIcpCellFactor = 1.13f;
void free_buf(DevBuf &b);                                  // hipFree, not the pool
void free_index(DeviceIndex &ix);
void recycle_index(tc_context *ctx, DeviceIndex &ix);       // blocks back to the context's pool
tc_status launch_normals_unsort(tc_context *ctx, const DeviceIndex &ix, const float *d_sorted6, float *d_out6);

// search.hip (its entry points: tc_knn, tc_radius_search, tc_search_index_*)
tc_status launch_radius_all(tc_context *ctx, const DeviceIndex &ix, const float *d_queries, size_t nq, float radius, uint32_t *d_counts,
                            const unsigned long long *d_offsets, uint32_t *d_idx, float *d_dist);
tc_status launch_knn(tc_context *ctx, const DeviceIndex &ix, const float *d_queries, size_t nq, size_t k,
                     uint32_t *d_idx, float *d_dist, uint32_t *d_count, float radius_sq = INFINITY);

// TC_DEBUG bit mask, read from the environment once per process
int debug_flags();

// comm.hip: collectives of a tc_comm on the context's stream (RCCL) or through the host callback (blocking)
tc_status comm_allreduce_f64(tc_comm *comm, double *d_buf, size_t count);
tc_status comm_allreduce_u32(tc_comm *comm, uint32_t *d_buf, size_t count);
tc_status comm_allgather(tc_comm *comm, void *d_buf, size_t bytes_per_rank);     // in place: rank r's part at r * bytes_per_rank
// Every rank calls it with the status of its own fallible set-up (allocations, index builds) BEFORE the first collective of a
// loop: one all-reduce of a flag; a rank that failed returns its own status, every other rank TC_GPU "a peer failed" -- nobody is
// left waiting in a collective its peer never enters.  One rank: returns `local`.
tc_status comm_agree(tc_comm *comm, tc_status local);

// icp.hip (its callers: the registration entry points, registration.hip)
// One registration, as the entry points hand it over: filled by named assignment, everything else at its default.
struct IcpJob {
    int mode = 0;                                       // 0 point-to-point, 1 point-to-plane, 2 GICP
    const float *src = nullptr, *tgt = nullptr;         // device clouds, xyz
    size_t ns = 0, nt = 0;
    const float *nrm = nullptr;                         // mode 1: the target's normals in input order, nstride floats apart (not with tgt_prebuilt)
    size_t nstride = 0;
    const float *cov_src = nullptr, *cov_tgt = nullptr; // mode 2: per-point covariances, 8 floats per point, input order
    const float *init = nullptr;                        // 7 floats: rotation i j k w, translation
    size_t max_iters = 0;
    float max_dist = -1.0f, conv_thr = 0.0f;            // (max_dist < 0: none)
    int kiss = 0;                                       // KISS-ICP's rules (IcpState::kiss)
    bool corr_on_device = true;                         // res->corr_target is a device array (icp_run; icp_run_sharded always writes one)
    // an index of the target built by the caller (a cloud handle; with its cell-sorted normals when mode 1), else the target is
    // indexed into ctx->tgt_index
    DeviceIndex *tgt_prebuilt = nullptr;
    // an index of the SOURCE the caller already has (a cloud handle that was indexed for its own normals): its cell-sorted records
    // are walked as they are instead of sorting the source again (icp_run, modes 0 and 1; GICP and the sharded road sort)
    const DeviceIndex *src_presorted = nullptr;
};
tc_status icp_run(tc_context *ctx, const IcpJob &job, tc_icp_result *res);
tc_status icp_run_sharded(tc_context *ctx, tc_comm *comm, int shard_mode, const IcpJob &job, tc_icp_result *res);

}  // namespace tc
