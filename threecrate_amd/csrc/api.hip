// api.hip -- the plumbing every surface of libthreecrate_hip shares: error mapping, the buffer pool, host<->device staging
// (ensure, stage_in, stage_out, synced, read_back, the overlapped upload), the pinned-word wait, the grids that recur; and the
// entry points of the context, of normal estimation and of profiling.  Every other entry point lives with its surface
// (registration.hip, search.hip, voxel.hip, cluster.hip, fpfh.hip, outlier.hip, plane.hip, cloud.hip, stream.hip, comm.hip,
// icp.hip's shard handle).  No CPU fallback exists: every compute entry point needs a HIP device and returns TC_GPU otherwise.
#include "tc_internal.h"
#include <sched.h>
#include <time.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

namespace tc {

// TC_DEBUG in the SHIPPED library: only the bits that print or count (8 the counting instantiation of the main pass, 64 refine
// statistics, 256 the grid decisions, 1024 block stamps) -- none of them changes a result or the road to it.  The bits that do
// (1 no warm start, 4 no inscribed-ball test, 16 no sums, 32 transform frozen, 512 no edge adaptation, 2048 exact box only, 8192 shells
// only: timing experiments and A/B switches) exist only in the development build, `make dev` ->
// variants/libthreecrate_hip_dev.so (this file compiled with -DTC_DEV, every other object shared with the shipped library): an
// inherited environment variable cannot turn the product into a wrong-answer build (tests/test_debug_bits.py).
[[maybe_unused]] constexpr int kDebugPrintOnlyBits = 8 | 64 | 256 | 1024;
int debug_flags() {
    static const int flags = [] {
        const char *e = getenv("TC_DEBUG");
        const int f = e ? atoi(e) : 0;
#ifdef TC_DEV
        return f;
#else
        return f & kDebugPrintOnlyBits;
#endif
    }();
    return flags;
}

tc_status fail(tc_context *ctx, tc_status st, const std::string &msg) {
    fault_point("fail");
    if (ctx) ctx->last_error = msg;
    return st;
}

// The handlers of the C ABI's function-try-blocks (TC_CATCH_STATUS): must not throw themselves.  The context's message buffer is
// reserved at creation (256 bytes), so that storing a short message allocates nothing; if even that fails the old message stays.
tc_status fail_nothrow(tc_context *ctx, tc_status st, const char *msg) noexcept {
    if (ctx) {
        try { ctx->last_error.assign(msg ? msg : "", std::min<size_t>(msg ? std::strlen(msg) : 0, 240)); } catch (...) { }
    }
    return st;
}

// Fault injection for the tests of those handlers (tests/test_abi_exceptions.py): TC_FAULT=<site>[,<site>...] makes the named sites
// throw std::bad_alloc -- "fail" (every error return that builds a message), "context" (tc_context_create), "batch_thread" (the
// second worker of tc_batch_icp fails to start), "stream_worker" (the frame streamer's thread body), "kitti" (tc_read_kitti_bin).
// Read per call: a test sets it after the library has been loaded.  DEVELOPMENT BUILD ONLY (-DTC_DEV, `make dev`): in the shipped
// library this is an empty function -- an inherited TC_FAULT cannot turn error returns into throws, and no worker thread calls
// getenv next to a host that may be changing its environment.
void fault_point(const char *site) {
#ifdef TC_DEV
    const char *e = getenv("TC_FAULT");
    if (!e || !*e) return;
    const size_t n = std::strlen(site);
    for (const char *p = e; *p;) {
        const char *q = std::strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : std::strlen(p);
        if (len == n && std::strncmp(p, site, n) == 0) throw std::bad_alloc();
        p = q ? q + 1 : p + len;
    }
#else
    (void)site;            // the shipped library never reads TC_FAULT (no getenv on worker threads, no injected throw)
#endif
}

// The pool parks what destroyed handles give back so that a handle per frame costs no hipMalloc.  Its cap follows the blocks it has
// seen -- a few handles' worth (a handle holds about a dozen buffers of at most `pool_largest` bytes) -- instead of a flat 32 GB:
// memory parked here is invisible to every other allocator of the process (torch's caching allocator, RCCL, a second context),
// which would run out of memory next to it.  tc_context_trim releases it on demand.
constexpr size_t kPoolMaxBytes = (size_t)32 << 30, kPoolMinBytes = (size_t)256 << 20, kPoolMaxBlocks = 96;

void recycle(tc_context *ctx, DevBuf &b) {
    if (!b.p) return;
    ctx->pool_largest = std::max(ctx->pool_largest, b.cap);
    const size_t cap_bytes = std::min(kPoolMaxBytes, std::max(kPoolMinBytes, 48 * ctx->pool_largest));
    if (ctx->pool.size() >= kPoolMaxBlocks || ctx->pool_bytes + b.cap > cap_bytes) {
        (void)hipFree(b.p);
    } else {
        ctx->pool.push_back(b);
        ctx->pool_bytes += b.cap;
    }
    b.p = nullptr; b.cap = 0;
}

tc_status ensure(tc_context *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap && b.p) return TC_OK;
    if (b.p) {
        // buffers may still be referenced by work in flight on the stream
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return fail(ctx, TC_GPU, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
        recycle(ctx, b);
    }
    // best fit from the pool: the smallest block that holds the request without wasting more than the request itself
    int best = -1;
    for (int i = 0; i < (int)ctx->pool.size(); ++i) {
        const size_t cap = ctx->pool[i].cap;
        if (cap >= bytes && cap <= 2 * bytes + 4096 && (best < 0 || cap < ctx->pool[best].cap)) best = i;
    }
    if (best >= 0) {
        b = ctx->pool[best];
        ctx->pool_bytes -= b.cap;
        ctx->pool.erase(ctx->pool.begin() + best);
        return TC_OK;
    }
    size_t want = std::max<size_t>(bytes + bytes / 4, 256);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess && !ctx->pool.empty()) {          // out of memory with blocks parked in the pool: release them, try again
        (void)hipGetLastError();
        for (auto &pb : ctx->pool) (void)hipFree(pb.p);
        ctx->pool.clear(); ctx->pool_bytes = 0;
        e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(ctx, TC_GPU, std::string("hipMalloc(") + std::to_string(want) + "): " + hipGetErrorString(e));
    }
    b.cap = want;
    return TC_OK;
}

ProfScope::ProfScope(tc_context *c, const char *name, bool dominant) : ctx(c) {
    if (ctx->profiling != 1 && ctx->profiling != 2) return;          // (3 = search statistics: no events)
    // (mode 2: every 37th launch of the dominant kernel (17th until round 6: the bubbles were 36 us of a 2.8 ms step) -- a stride coprime to the usual 50 iterations per call, so that the sampled
    // iteration indices walk through all of 0 .. 49 over the calls and the cold first pass is sampled as often as any other.  An event on the stream is a ~5.7 us bubble on either side of the kernel --
    // every 4th launch, as until round 4, was 2.9 us per ICP iteration = 5 % of the timed region, not the 1 % once estimated.)
    if (ctx->profiling == 2 && (!dominant || (ctx->prof_tick++ % 37u) != 0)) return;
    for (size_t i = 0; i < ctx->timers.size(); ++i)
        if (ctx->timers[i].name == name) { idx = (int)i; break; }
    if (idx < 0) { ctx->timers.push_back(KernelTimer{name, {}, 0, 0.0, 1e300, 0.0}); idx = (int)ctx->timers.size() - 1; }
    auto get = [&]() {
        hipEvent_t e = nullptr;
        if (!ctx->event_pool.empty()) { e = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else (void)hipEventCreate(&e);
        return e;
    };
    e0 = get(); e1 = get();
    ext = dominant;                                   // (the launch records both events itself: see the struct)
    if (!ext) (void)hipEventRecord(e0, ctx->stream);
}
ProfScope::~ProfScope() {
    if (idx < 0) return;
    if (!ext) (void)hipEventRecord(e1, ctx->stream);
    ctx->timers[idx].pending.emplace_back(e0, e1);
}

bool pinned_poll_enabled() {
    // (read per call like the other switches: a test or tools/dev/paths_stress.py sets it after the library has already run)
    const char *e = getenv("TC_NO_PINNED_POLL");
    return !(e && atoi(e) != 0);
}

void *pinned_dev_ptr(tc_context *ctx, const void *host_addr) {
    if (!ctx->pinned_dev) {
        void *d = nullptr;
        if (hipHostGetDevicePointer(&d, ctx->pinned, 0) != hipSuccess) return nullptr;
        ctx->pinned_dev = d;
    }
    return (char *)ctx->pinned_dev + ((const char *)host_addr - (const char *)ctx->pinned);
}

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield" ::: "memory");
#else
    sched_yield();
#endif
}

// Three regimes: the words that arrive within a kernel or two (bounding box, occupancy: ~10-100 us) are caught spinning; a wait
// that outlasts ~4 k spins yields the core between looks (the ranks of one host share its cores with each other and with
// RCCL's proxy threads); a wait of more than ~2 ms -- the tail of a long registration -- sleeps 50 us between looks instead of
// keeping a core busy for tens of milliseconds (the overshoot is noise at that length).
tc_status wait_pinned_word(tc_context *ctx, volatile uint32_t *word, const char *what) {
    struct timespec t0 = {0, 0};
    bool sleeping = false;
    for (unsigned spins = 0; *word == 0u; ++spins) {
        // spinning / yielding: one stream query per 1024 looks; sleeping: one per look (a look is 50 us by then, so a faulted stream
        // or one that drained without writing the word is noticed within a look, not after 50 ms -- ADVICE r5)
        if (sleeping || (spins & 1023u) == 1023u) {
            const hipError_t q = hipStreamQuery(ctx->stream);
            if (q == hipSuccess) { if (*word == 0u) return fail(ctx, TC_GPU, std::string("internal error: ") + what + ": the stream drained without the word being written"); break; }
            if (q != hipErrorNotReady) return fail(ctx, TC_GPU, std::string(what) + ": " + hipGetErrorString(q));
            if (!sleeping && spins >= 4096u) {
                struct timespec t;
                clock_gettime(CLOCK_MONOTONIC, &t);
                if (t0.tv_sec == 0 && t0.tv_nsec == 0) t0 = t;
                sleeping = (t.tv_sec - t0.tv_sec) * 1000000000ll + (t.tv_nsec - t0.tv_nsec) > 2000000ll;
            }
        }
        if (sleeping) { const struct timespec d = {0, 50000}; nanosleep(&d, nullptr); }
        else if (spins > 4096u) sched_yield();
        else cpu_relax();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return TC_OK;
}

void free_buf(DevBuf &b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

// NormalEstimationConfig -> cell edge factor: ring R0 = 2 must cover the (k+1)-NN sphere for all
// but ~1e-3 of the queries of a locally uniform cloud (Poisson tail), the rest take the overflow pass.
tc_status upload_async(tc_context *ctx, void *d_dst, const void *h_src, size_t bytes) {
    // small uploads stay on the context's stream: a few hundred microseconds of copy have nothing to hide under (measured no
    // difference either way on a 230 k-point pair), and one stream less is one thing less to go wrong
    if (bytes < ((size_t)8 << 20)) {
        TC_HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return TC_OK;
    }
    ctx->upload_used_copy_stream = true;
    if (!ctx->copy_stream) TC_HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->upload_event) TC_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->upload_event, hipEventDisableTiming));
    // the destination may still be read by work the context's stream holds from an earlier call: entry points return
    // synchronised, so nothing is in flight here
    TC_HIP_TRY(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    return TC_OK;
}
tc_status uploads_issued(tc_context *ctx) {
    if (!ctx->upload_used_copy_stream) return TC_OK;
    ctx->upload_used_copy_stream = false;
    TC_HIP_TRY(ctx, hipEventRecord(ctx->upload_event, ctx->copy_stream));
    ctx->upload_pending = true;
    return TC_OK;
}
tc_status wait_uploads(tc_context *ctx) {
    if (!ctx->upload_pending) return TC_OK;
    ctx->upload_pending = false;
    TC_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->upload_event, 0));
    return TC_OK;
}

tc_status stage_in(tc_context *ctx, DevBuf &b, const void *h_src, size_t bytes) {
    if (tc_status s = ensure(ctx, b, bytes)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(b.p, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return TC_OK;
}

tc_status synced(tc_context *ctx) {
    TC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TC_OK;
}
tc_status stage_out(tc_context *ctx, void *h_dst, const void *d_src, size_t bytes) {
    TC_HIP_TRY(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return synced(ctx);
}
tc_status read_back(tc_context *ctx, void *host_dst, const void *dev_src, size_t bytes) {
    if (tc_status s = stage_out(ctx, host_dst, dev_src, bytes)) return s;
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

float normals_cell_factor(size_t k, bool large) {
    const double K1 = (double)k + 1.0;
    const double lam = K1 + 3.1 * std::sqrt(K1) + 2.0;
    const double c = std::cbrt(lam / 4.18879);
    // multiplier scanned on the 1 M-point uniform cloud (k = 16, whole call): 0.8 -> 0.95 ms, 0.9 -> 0.83, 0.95 -> 0.79,
    // 1.0 -> 0.75, 1.1 -> 0.75, 1.2 -> 0.79, 1.3 -> 0.84 (the in-place ring continuation made the overflow tail cheap);
    // again at 7 waves per SIMD: 0.9 -> 0.70, 0.95 -> 0.67, 1.0 -> 0.655, 1.03 -> 0.65, 1.1 -> 0.71
    // after the centre-out pruned list pass (round 2; kernel only): 0.8 -> 537 us, 0.9 -> 479, 1.0 -> 445,
    // 1.03 -> 444, 1.1 -> 440, 1.2 -> 442, 1.3 -> 465: flat between 1.0 and 1.2
    // Applied to clouds of >= 2^18 points (those whose edge is also adapted to the measured occupancy); smaller clouds keep
    // 0.95: they are not adapted, and on surface-like frames (24 k-point voxel-filtered LiDAR) the larger edge costs 5 %.
    return (float)((large ? 1.03 : 0.95) * c / 2.0);
}

// points per occupied cell wanted on a SURFACE: the disc of radius ~1.9 h (ring 2) must hold the same
// lambda(k) points the volumetric factor above puts into the ring-2 sphere: sigma h^2 = lambda / (pi 1.9^2)
float normals_target_ppo(size_t k) {
    const double K1 = (double)k + 1.0;
    return (float)((K1 + 3.1 * std::sqrt(K1) + 2.0) / 11.3);
}

IndexSpec knn_grid(size_t list_len) {
    IndexSpec spec; spec.cell_factor = normals_cell_factor(list_len > 1 ? list_len - 1 : 1, false) * 2.0f;
    return spec;
}
IndexSpec ball_grid(float radius, bool finite_only) {
    const float r2 = radius * radius;                               // nearest_neighbor.rs:259
    IndexSpec spec; spec.cell_factor = 0.5f;
    if (r2 <= r2 && (!finite_only || r2 <= 3.0e38f)) { spec.min_cell_edge = 0.5f * radius; spec.target_ppo = 2.0f; }
    return spec;
}

void recycle_index(tc_context *ctx, DeviceIndex &ix) {
    for_each_buf(ix, [ctx](DevBuf &b) { recycle(ctx, b); });
    ix.pts12_valid = false; ix.vor_valid = false;
}

void free_index(DeviceIndex &ix) { for_each_buf(ix, free_buf); }

// build == false: `ix` already indexes this cloud (a cloud handle)
tc_status normals_on_index(tc_context *ctx, DeviceIndex &ix, bool build, float cell_factor_override, const float *d_xyz, size_t n,
                           const tc_normal_config *cfg, float *d_out, size_t p_begin, size_t p_end, bool slice_out, float4 *d_sorted_nrm,
                           bool with_bounds) {
    if (build) {
        // radius mode: ring 2 must cover the radius ball, so the cell edge is at least radius / 2
        const float min_h = cfg->has_radius ? cfg->radius * 0.5005f : 0.0f;
        const float f = cell_factor_override > 0.0f ? cell_factor_override : normals_cell_factor(cfg->k_neighbors, n >= kAdaptMinPoints);
        // a SLICE of the cell-sorted order is some rank's share of it: every rank has to build the same order (strict_order)
        IndexSpec spec; spec.cell_factor = f; spec.min_cell_edge = min_h; spec.target_ppo = normals_target_ppo(cfg->k_neighbors); spec.strict_order = slice_out;
        if (tc_status s = build_index(ctx, ix, d_xyz, n, spec)) return s;
    }
    float vp[3];
    if (cfg->has_viewpoint) {
        vp[0] = cfg->viewpoint[0]; vp[1] = cfg->viewpoint[1]; vp[2] = cfg->viewpoint[2];
    } else {   // normals.rs:275-303 (f32, same operation order; min/max are order independent)
        const float *bmn = ix.exact_min, *bmx = ix.exact_max;      // the cloud's exact box (the grid's may be clamped)
        const float cx = (bmn[0] + bmx[0]) / 2.0f, cy = (bmn[1] + bmx[1]) / 2.0f, cz = (bmn[2] + bmx[2]) / 2.0f;
        const float ex = bmx[0] - bmn[0], ey = bmx[1] - bmn[1], ez = bmx[2] - bmn[2];
        const float extent = std::sqrt(ex * ex + ey * ey + ez * ez);
        vp[0] = cx + 0.0f; vp[1] = cy + 0.0f; vp[2] = cz + extent;
    }
    // the inscribed-ball bounds of the ICP main pass fall out of the same k-NN lists (k-NN mode, whole cloud, the list must hold
    // the query and at least one other record)
    float4 *d_vor = nullptr;
    const bool knn_mode = !(cfg->has_radius && cfg->radius > 0.0f);
    if (with_bounds && knn_mode && p_begin == 0 && p_end >= n) {
        if (tc_status s = ensure(ctx, ix.vor, n * sizeof(float4))) return s;
        d_vor = (float4 *)ix.vor.p;
    }
    if (tc_status s = launch_normals(ctx, ix, d_xyz, *cfg, vp, d_out, p_begin, p_end, slice_out, d_sorted_nrm, d_vor)) return s;
    ix.vor_valid = d_vor != nullptr;
    return TC_OK;
}

static tc_status normals_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_normal_config *cfg, float *d_out,
                                size_t p_begin = 0, size_t p_end = (size_t)-1, bool slice_out = false) {
    return normals_on_index(ctx, ctx->tgt_index, true, 0.0f, d_xyz, n, cfg, d_out, p_begin, p_end, slice_out, nullptr);
}

}  // namespace tc

using namespace tc;

extern "C" {

int tc_abi_version(void) { return TC_ABI_VERSION; }

int tc_device_count(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} TC_CATCH_VALUE(0)

static tc_status context_create(int device, void *stream, bool own, tc_context **out) {
    if (!out) return TC_INVALID_DATA;
    *out = nullptr;
    fault_point("context");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return TC_GPU;
    if (hipSetDevice(device) != hipSuccess) return TC_GPU;
    std::unique_ptr<tc_context> holder(new tc_context());          // (an exception below must not leak it)
    tc_context *ctx = holder.get();
    ctx->last_error.reserve(256);          // fail_nothrow stores its messages without allocating
    ctx->device = device;
    ctx->own_stream = own;
    if (own) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return TC_GPU;
    } else {
        ctx->stream = (hipStream_t)stream;
    }
    if (hipHostMalloc(&ctx->pinned, kPinnedBytes, hipHostMallocDefault) != hipSuccess) {
        if (own) (void)hipStreamDestroy(ctx->stream);
        return TC_GPU;
    }
    *out = holder.release();
    return TC_OK;
}

tc_status tc_context_create(int device, tc_context **out) try { return context_create(device, nullptr, true, out); } TC_CATCH_STATUS(nullptr)
tc_status tc_context_create_on_stream(int device, void *hip_stream, tc_context **out) try {
    return context_create(device, hip_stream, false, out);
} TC_CATCH_STATUS(nullptr)

tc_status tc_context_wait_stream(tc_context *ctx, void *other_hip_stream) try {
    if (!ctx) return TC_INVALID_DATA;
    hipStream_t other = (hipStream_t)other_hip_stream;
    if (other == ctx->stream) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->order_event) TC_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->order_event, hipEventDisableTiming));
    TC_HIP_TRY(ctx, hipEventRecord(ctx->order_event, other));
    TC_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->order_event, 0));
    return TC_OK;
} TC_CATCH_STATUS(ctx)

// the other direction: work enqueued on `other` AFTER this call waits for everything the context's stream holds now (a caller that
// is about to overwrite or free a buffer it just handed to tc_cloud_upload_device: no host wait)
tc_status tc_stream_wait_context(tc_context *ctx, void *other_hip_stream) try {
    if (!ctx) return TC_INVALID_DATA;
    hipStream_t other = (hipStream_t)other_hip_stream;
    if (other == ctx->stream) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->release_event) TC_HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->release_event, hipEventDisableTiming));
    TC_HIP_TRY(ctx, hipEventRecord(ctx->release_event, ctx->stream));
    TC_HIP_TRY(ctx, hipStreamWaitEvent(other, ctx->release_event, 0));
    return TC_OK;
} TC_CATCH_STATUS(ctx)

void tc_context_destroy(tc_context *ctx) try {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->copy_stream) { (void)hipStreamSynchronize(ctx->copy_stream); (void)hipStreamDestroy(ctx->copy_stream); }
    if (ctx->upload_event) (void)hipEventDestroy(ctx->upload_event);
    for_each_buf(*ctx, free_buf);
    for (auto &pb : ctx->pool) (void)hipFree(pb.p);
    for (auto e : ctx->chunk_events) (void)hipEventDestroy(e);
    if (ctx->order_event) (void)hipEventDestroy(ctx->order_event);
    if (ctx->release_event) (void)hipEventDestroy(ctx->release_event);
    for (auto &t : ctx->timers) for (auto &p : t.pending) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
} TC_CATCH_VOID

tc_status tc_context_trim(tc_context *ctx) try {
    if (!ctx) return TC_INVALID_DATA;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    TC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &pb : ctx->pool) (void)hipFree(pb.p);
    ctx->pool.clear();
    ctx->pool_bytes = 0;
    ctx->pool_largest = 0;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

const char *tc_last_error_message(const tc_context *ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }

tc_status tc_synchronize(tc_context *ctx) try {
    if (!ctx) return TC_INVALID_DATA;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

void tc_normal_config_default(tc_normal_config *cfg) try {
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->k_neighbors = 10;            // normals.rs:28-36
    cfg->has_radius = 0;
    cfg->consistent_orientation = 1;
    cfg->has_viewpoint = 0;
} TC_CATCH_VOID

// ---- normals --------------------------------------------------------------------------------
static tc_status normals_validate(tc_context *ctx, size_t n, const tc_normal_config *cfg, bool *empty) {
    *empty = false;
    if (!ctx || !cfg) return TC_INVALID_DATA;
    if (n == 0) { *empty = true; return TC_OK; }                                        // normals.rs:261-263
    if (cfg->k_neighbors < 3) return fail(ctx, TC_INVALID_DATA, "k_neighbors must be at least 3");   // :265-269
    return TC_OK;
}

tc_status tc_estimate_normals_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_normal_config *cfg,
                                     float *d_out) try {
    bool empty;
    if (tc_status s = normals_validate(ctx, n, cfg, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = normals_device(ctx, d_xyz, n, cfg, d_out)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

// ---- sharded normals of one big cloud over several GPUs ----
tc_status tc_estimate_normals_slice_device(tc_context *ctx, const float *d_xyz, size_t n, const tc_normal_config *cfg, size_t begin,
                                           size_t end, float *d_slice_out) try {
    bool empty;
    if (tc_status s = normals_validate(ctx, n, cfg, &empty)) return s;
    if (empty) return TC_OK;
    if (begin > end || end > n) return fail(ctx, TC_INVALID_DATA, "normals slice: need begin <= end <= n");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = normals_device(ctx, d_xyz, n, cfg, d_slice_out, begin, end, true)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_normals_unsort_device(tc_context *ctx, const float *d_sorted_all, size_t n, float *d_out) try {
    if (!ctx) return TC_INVALID_DATA;
    if (n == 0) return TC_OK;
    if (ctx->tgt_index.geom.n != n || !ctx->tgt_index.pts.p)
        return fail(ctx, TC_INVALID_DATA, "normals unsort: call tc_estimate_normals_slice_device on this context with the same cloud first");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = launch_normals_unsort(ctx, ctx->tgt_index, d_sorted_all, d_out)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

tc_status tc_estimate_normals(tc_context *ctx, const float *xyz, size_t n, const tc_normal_config *cfg, float *out) try {
    bool empty;
    if (tc_status s = normals_validate(ctx, n, cfg, &empty)) return s;
    if (empty) return TC_OK;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->out_a, n * 6 * sizeof(float))) return s;
    if (tc_status s = stage_in(ctx, ctx->in_a, xyz, n * 3 * sizeof(float))) return s;
    if (tc_status s = normals_device(ctx, (const float *)ctx->in_a.p, n, cfg, (float *)ctx->out_a.p)) return s;
    return stage_out(ctx, out, ctx->out_a.p, n * 6 * sizeof(float));
} TC_CATCH_STATUS(ctx)

// this rank's slot of ceil(n / W) cell-sorted positions -> slot_out (rows x 6); the fallible part of the sharded normals
static tc_status sharded_normals_slot(tc_context *ctx, tc_comm *comm, const float *d_xyz, size_t n, const tc_normal_config *cfg,
                                      float *slot_out, size_t &lo, size_t &hi) {
    const size_t W = (size_t)comm->nranks, r = (size_t)comm->rank;
    const size_t rows = (n + W - 1) / W;
    lo = std::min(r * rows, n); hi = std::min((r + 1) * rows, n);
    return normals_device(ctx, d_xyz, n, cfg, slot_out, lo, hi, true);
}

tc_status tc_sharded_estimate_normals_device(tc_context *ctx, tc_comm *comm, const float *d_xyz, size_t n, const tc_normal_config *cfg,
                                             float *d_out) try {
    if (!comm) return TC_INVALID_DATA;
    bool empty;
    if (tc_status s = normals_validate(ctx, n, cfg, &empty)) return s;
    if (empty) return TC_OK;
    if (comm->ctx != ctx) return fail(ctx, TC_INVALID_DATA, "the communicator belongs to another context");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t W = (size_t)comm->nranks, r = (size_t)comm->rank;
    // equal slots of `rows` records (the last ranks' ranges may be shorter or empty): the all-gather runs in place
    const size_t rows = (n + W - 1) / W;
    // everything that can fail on ONE rank (allocation, index build, launches) happens before the collective, and the ranks agree
    // on it: a rank returning early would leave its peers waiting in the all-gather for ever (comm_agree)
    tc_status local = ensure(ctx, ctx->out_a, W * rows * 6 * sizeof(float));
    float *sorted_all = (float *)ctx->out_a.p;
    size_t lo = 0, hi = 0;
    if (local == TC_OK) local = sharded_normals_slot(ctx, comm, d_xyz, n, cfg, sorted_all + r * rows * 6, lo, hi);
    if (tc_status s = comm_agree(comm, local)) return s;
    if (tc_status s = comm_allgather(comm, sorted_all, rows * 6 * sizeof(float))) return s;
    // slot q holds the cell-sorted positions [q rows, min((q + 1) rows, n)): the slots are contiguous in position
    if (tc_status s = launch_normals_unsort(ctx, ctx->tgt_index, sorted_all, d_out)) return s;
    return synced(ctx);
} TC_CATCH_STATUS(ctx)

__global__ void __launch_bounds__(256) slice_orig_index_kernel(const float4 *__restrict__ pts, uint32_t lo, uint32_t count, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = __float_as_uint(pts[lo + i].w);
}

tc_status tc_sharded_estimate_normals_local_device(tc_context *ctx, tc_comm *comm, const float *d_xyz, size_t n, const tc_normal_config *cfg,
                                                   float *d_out_slice, uint32_t *d_orig_index, size_t *first, size_t *count) try {
    if (!comm || !first || !count) return TC_INVALID_DATA;
    *first = 0; *count = 0;
    bool empty;
    if (tc_status s = normals_validate(ctx, n, cfg, &empty)) return s;
    if (empty) return TC_OK;
    if (comm->ctx != ctx) return fail(ctx, TC_INVALID_DATA, "the communicator belongs to another context");
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t lo = 0, hi = 0;
    if (tc_status s = sharded_normals_slot(ctx, comm, d_xyz, n, cfg, d_out_slice, lo, hi)) return s;
    if (d_orig_index && hi > lo) {
        hipLaunchKernelGGL(slice_orig_index_kernel, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const float4 *)ctx->tgt_index.pts.p, (uint32_t)lo, (uint32_t)(hi - lo), d_orig_index);
        TC_HIP_TRY(ctx, hipGetLastError());
    }
    TC_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *first = lo; *count = hi - lo;
    return TC_OK;
} TC_CATCH_STATUS(ctx)

unsigned long long tc_debug_counter(const tc_context *ctx, int which) try {
    if (!ctx) return 0;
    if (which >= TC_COUNTER_ICP_ITERATIONS && which <= TC_COUNTER_ICP_STEPS_TAKEN) return ctx->stat_icp[which - TC_COUNTER_ICP_ITERATIONS];
    return which == TC_COUNTER_INDEXED_POINTS ? ctx->stat_indexed_points : which == TC_COUNTER_INDEX_BUILDS ? ctx->stat_index_builds : 0ull;
} TC_CATCH_VALUE(0)

// ---- profiling ------------------------------------------------------------------------------
void tc_profile_enable(tc_context *ctx, int on) {
    if (!ctx) return;
    ctx->profiling = on;
    ctx->prof_tick = 0;
    if (on == 3) for (auto &v : ctx->stat_icp) v = 0;          // a statistics session starts from zero
}

static void profile_collect(tc_context *ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &t : ctx->timers) {
        for (auto &p : t.pending) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
                t.total_ms += ms; t.launches += 1;
                t.min_ms = std::min(t.min_ms, (double)ms); t.max_ms = std::max(t.max_ms, (double)ms);
            }
            ctx->event_pool.push_back(p.first);
            ctx->event_pool.push_back(p.second);
        }
        t.pending.clear();
    }
}

void tc_profile_reset(tc_context *ctx) try {
    if (!ctx) return;
    profile_collect(ctx);
    for (auto &t : ctx->timers) { t.launches = 0; t.total_ms = 0.0; t.min_ms = 1e300; t.max_ms = 0.0; }
} TC_CATCH_VOID

size_t tc_profile_read(tc_context *ctx, tc_kernel_stat *out, size_t cap) try {
    if (!ctx) return 0;
    profile_collect(ctx);
    size_t n = 0;
    for (auto &t : ctx->timers) {
        if (n < cap && out) {
            std::memset(&out[n], 0, sizeof(out[n]));
            std::strncpy(out[n].name, t.name.c_str(), sizeof(out[n].name) - 1);
            out[n].launches = t.launches;
            out[n].total_ms = t.total_ms;
            out[n].min_ms = t.launches ? t.min_ms : 0.0;
            out[n].max_ms = t.max_ms;
        }
        ++n;
    }
    return n;
} TC_CATCH_VALUE(0)

}  // extern "C"
