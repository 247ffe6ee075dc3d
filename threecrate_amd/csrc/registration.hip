// registration.hip -- the registration entry points, the layer above icp_run / icp_run_sharded (icp.hip): point-to-point and
// point-to-plane (single GPU, sharded), batch, multiscale, KISS-ICP, GICP with its covariance kernel.  Validation in the reference's
// order and precedence; a variant is one block: its validation, its job (p2p_job / p2plane_job + its own fields), the twins.
#include "tc_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>

namespace tc {

// compute_covariances (gicp.rs:52-86): the k nearest points INCLUDING the point itself (ascending distance),
// f32 mean and outer products in that order, / max(n - 1, 1), + 1e-4 I; fewer than 3 neighbours -> 1e-3 I.
// out: two float4 per point (xx, xy, xz, yy), (yz, zz, 0, 0), original order.
__global__ void __launch_bounds__(256) gicp_cov_kernel(const float *__restrict__ xyz, uint32_t n, const uint32_t *__restrict__ idx,
                                                      const uint32_t *__restrict__ count, uint32_t k, float4 *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = count[i];
    if (m < 3) {
        out[2 * (size_t)i] = make_float4(1e-3f, 0.f, 0.f, 1e-3f);
        out[2 * (size_t)i + 1] = make_float4(0.f, 1e-3f, 0.f, 0.f);
        return;
    }
    const uint32_t *nb = idx + (size_t)i * k;
    const float nf = (float)m;
    float mx = 0.f, my = 0.f, mz = 0.f;
    for (uint32_t j = 0; j < m; ++j) { const uint32_t q = nb[j]; mx = mx + xyz[3 * (size_t)q]; my = my + xyz[3 * (size_t)q + 1]; mz = mz + xyz[3 * (size_t)q + 2]; }
    mx /= nf; my /= nf; mz /= nf;
    float xx = 0.f, xy = 0.f, xz = 0.f, yy = 0.f, yz = 0.f, zz = 0.f;
    for (uint32_t j = 0; j < m; ++j) {
        const uint32_t q = nb[j];
        const float dx = xyz[3 * (size_t)q] - mx, dy = xyz[3 * (size_t)q + 1] - my, dz = xyz[3 * (size_t)q + 2] - mz;
        xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
    }
    const float den = fmaxf(nf - 1.0f, 1.0f);
    out[2 * (size_t)i] = make_float4(xx / den + 1e-4f, xy / den, xz / den, yy / den + 1e-4f);
    out[2 * (size_t)i + 1] = make_float4(yz / den, zz / den + 1e-4f, 0.f, 0.f);
}

static tc_status gicp_covariances_device(tc_context *ctx, const float *d_xyz, size_t n, size_t k, DevBuf &idx, DevBuf &dist, DevBuf &cnt,
                                         float *d_cov8) {
    k = std::max<size_t>(k, 4);
    if (k > kMaxK) return fail(ctx, TC_UNSUPPORTED, "GICP: k_correspondences > 2048 is not supported by this backend");
    if (tc_status s = ensure(ctx, idx, n * k * sizeof(uint32_t))) return s;
    if (tc_status s = ensure(ctx, dist, n * k * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, cnt, n * sizeof(uint32_t))) return s;
    // same grid as tc_knn (the point itself is one of its k nearest)
    if (tc_status s = build_index(ctx, ctx->tgt_index, d_xyz, n, knn_grid(k))) return s;
    if (tc_status s = launch_knn(ctx, ctx->tgt_index, d_xyz, n, k, (uint32_t *)idx.p, (float *)dist.p, (uint32_t *)cnt.p)) return s;
    ProfScope ps(ctx, "gicp_covariances");
    hipLaunchKernelGGL(gicp_cov_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_xyz, (uint32_t)n, (const uint32_t *)idx.p,
                       (const uint32_t *)cnt.p, (uint32_t)k, (float4 *)d_cov8);
    TC_HIP_TRY(ctx, hipGetLastError());
    return TC_OK;
}

}  // namespace tc

using namespace tc;

// normals != nullptr: point to plane, {n_normals, stride}; its two checks sit where the reference has them (registration.rs:517-531)
static tc_status icp_validate(tc_context *ctx, size_t ns, size_t nt, size_t max_iters, const tc_icp_result *res, const size_t *normals = nullptr) {
    if (!ctx || !res) return TC_INVALID_DATA;
    if (ns == 0 || nt == 0) return fail(ctx, TC_INVALID_DATA, "Source or target point cloud is empty");   // registration.rs:266-270
    if (normals && normals[0] != nt) return fail(ctx, TC_INVALID_DATA, "target_normals length must equal the number of target points");
    if (max_iters == 0) return fail(ctx, TC_INVALID_DATA, "Max iterations must be positive");             // :272-276
    if (normals && normals[1] < 3) return fail(ctx, TC_INVALID_DATA, "normal_stride must be >= 3");
    return check_point_count(ctx, ns, nt);
}

static tc_status p2plane_validate(tc_context *ctx, size_t ns, size_t nt, size_t nn, size_t stride, size_t max_iters,
                                  const tc_icp_result *res) {
    const size_t normals[2] = {nn, stride};
    return icp_validate(ctx, ns, nt, max_iters, res, normals);
}

// The job of a twin pair, filled ONCE from the entry point's arguments: the host twin then points it at its staged copies
static IcpJob p2p_job(const float *src, size_t ns, const float *tgt, size_t nt, const float init[7], size_t max_iters, float max_dist, float conv_thr) {
    IcpJob job;
    job.src = src; job.ns = ns; job.tgt = tgt; job.nt = nt;
    job.init = init; job.max_iters = max_iters; job.max_dist = max_dist; job.conv_thr = conv_thr;
    return job;
}
static IcpJob p2plane_job(const float *src, size_t ns, const float *tgt, size_t nt, const float *nrm, size_t stride, const float init[7],
                          size_t max_iters, float max_dist, float conv_thr) {
    IcpJob job = p2p_job(src, ns, tgt, nt, init, max_iters, max_dist, conv_thr);
    job.mode = 1; job.nrm = nrm; job.nstride = stride;
    return job;
}

// The host road of tc_icp_detailed / tc_icp_point_to_plane_detailed: `job` holds the CALLER's clouds (mode 1: n_normals rows of normals).
// The target first, on the context's stream: its index build starts as soon as it has landed; normals and source follow on the
// copy stream, under the build (icp_setup waits for them before it gathers the normals / orders the source).
static tc_status icp_from_host(tc_context *ctx, IcpJob job, size_t n_normals, tc_icp_result *result) {
    const bool plane = job.mode == 1;
    const size_t nbytes = plane ? ((n_normals - 1) * job.nstride + 3) * sizeof(float) : 0;
    if (tc_status s = ensure(ctx, ctx->in_a, job.ns * 3 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, ctx->in_b, job.nt * 3 * sizeof(float))) return s;
    if (plane) { if (tc_status s = ensure(ctx, ctx->in_c, nbytes)) return s; }
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_b.p, job.tgt, job.nt * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (plane) { if (tc_status s = upload_async(ctx, ctx->in_c.p, job.nrm, nbytes)) return s; }
    if (tc_status s = upload_async(ctx, ctx->in_a.p, job.src, job.ns * 3 * sizeof(float))) return s;
    if (tc_status s = uploads_issued(ctx)) return s;
    job.src = (const float *)ctx->in_a.p; job.tgt = (const float *)ctx->in_b.p;
    if (plane) job.nrm = (const float *)ctx->in_c.p;
    job.corr_on_device = false;
    const tc_status rc = icp_run(ctx, job, result);
    if (ctx->upload_pending) { ctx->upload_pending = false; (void)hipStreamSynchronize(ctx->copy_stream); }     // (an early error return)
    return rc;
}

// A host caller's corr_target while a device road runs (KISS-ICP, GICP, multiscale): a device array of ns words stands in, the
// caller's pointer is back on every path, and the words are copied to it ONLY after TC_OK -- a failed call leaves the caller's
// array as it was (corr_on_device = false would not: icp_run copies before fill_result can fail).
struct CorrStandIn {
    tc_icp_result *res; uint32_t *host; ScopedBuf dev;
    explicit CorrStandIn(tc_icp_result *r) : res(r), host(r->corr_target) {}
    ~CorrStandIn() { res->corr_target = host; }
    tc_status place(tc_context *ctx, size_t ns) {
        if (host) { if (tc_status s = ensure(ctx, dev, ns * 4)) return s; res->corr_target = (uint32_t *)dev.p; }
        return TC_OK;
    }
    void copy_back(tc_status st, size_t count) { if (st == TC_OK && host) (void)hipMemcpy(host, dev.p, count * 4, hipMemcpyDeviceToHost); }
};

extern "C" {

// ---- ICP ------------------------------------------------------------------------------------
tc_status tc_icp_detailed_device(tc_context *ctx, const float *d_source, size_t n_source, const float *d_target,
                                 size_t n_target, const float init[7], size_t max_iters, float max_dist, float conv_thr,
                                 tc_icp_result *result) try {
    if (tc_status s = icp_validate(ctx, n_source, n_target, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return icp_run(ctx, p2p_job(d_source, n_source, d_target, n_target, init, max_iters, max_dist, conv_thr), result);
} TC_CATCH_STATUS(ctx)

tc_status tc_icp_detailed(tc_context *ctx, const float *source, size_t n_source, const float *target, size_t n_target,
                          const float init[7], size_t max_iters, float max_dist, float conv_thr, tc_icp_result *result) try {
    if (tc_status s = icp_validate(ctx, n_source, n_target, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return icp_from_host(ctx, p2p_job(source, n_source, target, n_target, init, max_iters, max_dist, conv_thr), 0, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_icp_point_to_point(tc_context *ctx, const float *source, size_t n_source, const float *target, size_t n_target,
                                const float init[7], size_t max_iterations, float conv_thr, float max_dist,
                                tc_icp_result *result) try {
    if (tc_status s = icp_validate(ctx, n_source, n_target, max_iterations, result)) return s;
    if (!(conv_thr > 0.0f)) return fail(ctx, TC_INVALID_DATA, "Convergence threshold must be positive");   // registration.rs:665-669
    return tc_icp_detailed(ctx, source, n_source, target, n_target, init, max_iterations, max_dist, conv_thr, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_icp(tc_context *ctx, const float *source, size_t n_source, const float *target, size_t n_target,
                 const float init[7], size_t max_iters, float out[7]) try {
    if (!ctx || !out || !init) return TC_INVALID_DATA;
    tc_icp_result r;
    std::memset(&r, 0, sizeof(r));
    tc_status s = tc_icp_detailed(ctx, source, n_source, target, n_target, init, max_iters, -1.0f, 1e-6f, &r);   // registration.rs:238
    if (s == TC_OK) std::memcpy(out, r.transformation, 7 * sizeof(float));
    else std::memcpy(out, init, 7 * sizeof(float));                                                             // :240
    return TC_OK;
} TC_CATCH_STATUS(ctx)

tc_status tc_icp_point_to_plane_detailed_device(tc_context *ctx, const float *d_source, size_t n_source,
                                                const float *d_target, size_t n_target, const float *d_normals,
                                                size_t n_normals, size_t stride, const float init[7], size_t max_iters,
                                                float max_dist, float conv_thr, tc_icp_result *result) try {
    if (tc_status s = p2plane_validate(ctx, n_source, n_target, n_normals, stride, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return icp_run(ctx, p2plane_job(d_source, n_source, d_target, n_target, d_normals, stride, init, max_iters, max_dist, conv_thr), result);
} TC_CATCH_STATUS(ctx)

tc_status tc_icp_point_to_plane_detailed(tc_context *ctx, const float *source, size_t n_source, const float *target,
                                         size_t n_target, const float *normals, size_t n_normals, size_t stride,
                                         const float init[7], size_t max_iters, float max_dist, float conv_thr,
                                         tc_icp_result *result) try {
    if (tc_status s = p2plane_validate(ctx, n_source, n_target, n_normals, stride, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return icp_from_host(ctx, p2plane_job(source, n_source, target, n_target, normals, stride, init, max_iters, max_dist, conv_thr), n_normals, result);
} TC_CATCH_STATUS(ctx)

// ---- one registration / one cloud over the ranks of a communicator ----------------------------------
// what both sharded registrations check first; *ns_check = the source count their validation sees
static tc_status sharded_validate(tc_context *ctx, const tc_comm *comm, int shard_mode, const tc_icp_result *result, size_t n_source,
                                  size_t *ns_check) {
    if (!ctx || !comm || !result) return TC_INVALID_DATA;
    if (comm->ctx != ctx) return fail(ctx, TC_INVALID_DATA, "the communicator belongs to another context");
    if (shard_mode != TC_SHARD_SPATIAL && shard_mode != TC_SHARD_LOCAL && shard_mode != TC_SHARD_INDEX) return fail(ctx, TC_INVALID_DATA, "unknown shard mode");
    // a rank of a TC_SHARD_LOCAL run may own no source points (the other ranks do)
    *ns_check = (shard_mode == TC_SHARD_LOCAL && comm->nranks > 1 && n_source == 0) ? 1 : n_source;
    return TC_OK;
}

tc_status tc_sharded_icp_point_to_plane_device(tc_context *ctx, tc_comm *comm, int shard_mode, const float *d_source, size_t n_source,
                                               const float *d_target, size_t n_target, const float *d_normals, size_t n_normals,
                                               size_t stride, const float init[7], size_t max_iters, float max_dist, float conv_thr,
                                               tc_icp_result *result) try {
    size_t ns_check;
    if (tc_status s = sharded_validate(ctx, comm, shard_mode, result, n_source, &ns_check)) return s;
    if (tc_status s = p2plane_validate(ctx, ns_check, n_target, n_normals, stride, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const IcpJob job = p2plane_job(d_source, n_source, d_target, n_target, d_normals, stride, init, max_iters, max_dist, conv_thr);
    return icp_run_sharded(ctx, comm, shard_mode, job, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_sharded_icp_detailed_device(tc_context *ctx, tc_comm *comm, int shard_mode, const float *d_source, size_t n_source,
                                         const float *d_target, size_t n_target, const float init[7], size_t max_iters, float max_dist,
                                         float conv_thr, tc_icp_result *result) try {
    size_t ns_check;
    if (tc_status s = sharded_validate(ctx, comm, shard_mode, result, n_source, &ns_check)) return s;
    if (tc_status s = icp_validate(ctx, ns_check, n_target, max_iters, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    return icp_run_sharded(ctx, comm, shard_mode, p2p_job(d_source, n_source, d_target, n_target, init, max_iters, max_dist, conv_thr), result);
} TC_CATCH_STATUS(ctx)

tc_status tc_batch_icp(tc_context *const *ctxs, size_t n_ctx, const tc_batch_icp_job *jobs, size_t n_jobs,
                       tc_batch_icp_result *results) try {
    if (!ctxs || n_ctx == 0 || (!jobs && n_jobs) || (!results && n_jobs)) return TC_INVALID_DATA;
    static const float identity[7] = {0, 0, 0, 1, 0, 0, 0};   // gpu/icp.rs:202: always starts from identity
    auto worker = [&](size_t c) {
        for (size_t j = c; j < n_jobs; j += n_ctx) {
            tc_icp_result r;
            std::memset(&r, 0, sizeof(r));
            const tc_batch_icp_job &jb = jobs[j];
            tc_status s = tc_icp_point_to_point(ctxs[c], jb.source, jb.n_source, jb.target, jb.n_target, identity,
                                                jb.max_iterations, jb.convergence_threshold, jb.max_correspondence_distance, &r);
            std::memcpy(results[j].transformation, s == TC_OK ? r.transformation : identity, 7 * sizeof(float));
            results[j].final_error = r.mse;
            results[j].iterations = r.iterations;
            results[j].status = (int32_t)s;
        }
    };
    if (n_ctx == 1) { worker(0); return TC_OK; }
    // One thread per context.  A thread that cannot be started (std::system_error, std::bad_alloc) must not take the started ones
    // down with it -- destroying a joinable std::thread is std::terminate --: the contexts left without a thread are served on the
    // caller's thread, one after the other, and every started thread is joined.  (worker() itself cannot throw: it calls wrapped
    // entry points and copies plain structs.)
    std::vector<std::thread> th;
    size_t started = 0;
    try {
        th.reserve(n_ctx);
        for (; started < n_ctx; ++started) {
            if (started == 1) fault_point("batch_thread");
            th.emplace_back(worker, started);
        }
    } catch (...) { }
    for (size_t c = started; c < n_ctx; ++c) worker(c);
    for (auto &t : th) t.join();
    return TC_OK;
} TC_CATCH_STATUS(nullptr)

// ---- multiscale ICP (registration.rs:704-789) ---------------------------------------------------
tc_status tc_multiscale_icp_point_to_point(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt,
                                           const float init[7], const tc_multiscale_icp_config *cfg, tc_icp_result *result) try {
    if (!ctx || !cfg || !result || !init) return TC_INVALID_DATA;
    if (ns == 0 || nt == 0) return fail(ctx, TC_INVALID_DATA, "Source or target point cloud is empty");              // :710-714
    if (cfg->n_levels == 0) return fail(ctx, TC_INVALID_DATA, "At least one ICP scale level is required");          // :715-719
    if (!(cfg->convergence_threshold > 0.0f)) return fail(ctx, TC_INVALID_DATA, "Convergence threshold must be positive");   // :720-724
    if (cfg->final_refinement_iterations == 0) return fail(ctx, TC_INVALID_DATA, "Final refinement iterations must be positive");   // :725-729
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    // full-resolution clouds and the per-level down-sampled clouds live in caller-independent buffers
    ScopedBuf full_s, full_t, down_s, down_t;
    if (tc_status s = ensure(ctx, full_s, ns * 12)) return s;
    if (tc_status s = ensure(ctx, full_t, nt * 12)) return s;
    if (tc_status s = ensure(ctx, down_s, ns * 12)) return s;
    if (tc_status s = ensure(ctx, down_t, nt * 12)) return s;
    if (hipMemcpyAsync(full_s.p, source, ns * 12, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(full_t.p, target, nt * 12, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, TC_GPU, "multiscale ICP: uploading the caller's clouds failed");
    }
    float cur[7];
    std::memcpy(cur, init, sizeof(cur));
    uint64_t total_iters = 0;
    bool any = false;
    tc_icp_result r;
    for (size_t l = 0; l < cfg->n_levels; ++l) {
        const tc_icp_scale_level &lv = cfg->levels[l];
        if (!(lv.voxel_size > 0.0f)) return fail(ctx, TC_INVALID_DATA, "Scale voxel_size must be positive");       // :736-740
        if (lv.max_iterations == 0) return fail(ctx, TC_INVALID_DATA, "Scale max_iterations must be positive");    // :741-745
        size_t nds = 0, ndt = 0;
        if (tc_status s = voxel_filter_device(ctx, (const float *)full_s.p, ns, lv.voxel_size, (float *)down_s.p, &nds)) return s;
        if (tc_status s = voxel_filter_device(ctx, (const float *)full_t.p, nt, lv.voxel_size, (float *)down_t.p, &ndt)) return s;
        if (nds < 3 || ndt < 3) continue;                                                                             // :749-751
        std::memset(&r, 0, sizeof(r));
        const IcpJob job = p2p_job((const float *)down_s.p, nds, (const float *)down_t.p, ndt, cur, lv.max_iterations,
                                   lv.max_correspondence_distance, cfg->convergence_threshold);
        if (tc_status s = icp_run(ctx, job, &r)) return s;
        std::memcpy(cur, r.transformation, sizeof(cur));
        total_iters += r.iterations;
        any = true;
    }
    if (!any) return fail(ctx, TC_ALGORITHM, "No multiscale ICP level had enough downsampled points");   // :767-771
    tc_icp_result fin;
    std::memset(&fin, 0, sizeof(fin));
    fin.corr_target = result->corr_target;
    CorrStandIn corr(&fin);
    if (tc_status s = corr.place(ctx, ns)) return s;
    const IcpJob job = p2p_job((const float *)full_s.p, ns, (const float *)full_t.p, nt, cur, cfg->final_refinement_iterations,
                               cfg->final_max_correspondence_distance, cfg->convergence_threshold);
    const tc_status st = icp_run(ctx, job, &fin);
    if (st == TC_OK) {
        std::memcpy(result->transformation, fin.transformation, sizeof(fin.transformation));
        result->mse = fin.mse;
        result->iterations = total_iters + fin.iterations;                                                           // :782-788
        result->converged = fin.converged;
        result->n_correspondences = fin.n_correspondences;
    }
    corr.copy_back(st, ns);
    return st;
} TC_CATCH_STATUS(ctx)

// ---- KISS-ICP (kiss_icp.rs:183-300) ----------------------------------------------------------------
// range filter -> voxel down-sampling of the source -> point-to-point ICP against the full target with the
// adaptive correspondence threshold, mse measured after every update, fixed 1e-6 convergence rule
static float kiss_adaptive_threshold(const float init[7], float voxel_size) {        // :82-95, f32 like the reference
    const float trans = std::sqrt(init[4] * init[4] + init[5] * init[5] + init[6] * init[6]);
    const float imag = std::sqrt(init[0] * init[0] + init[1] * init[1] + init[2] * init[2]);
    const float motion = trans + 2.0f * imag * voxel_size;
    return std::fmin(std::fmax(3.0f * motion, 3.0f * voxel_size), 10.0f * voxel_size);
}

// the argument checks of both entry points (the host one makes them before it stages anything)
static tc_status kiss_validate(tc_context *ctx, size_t ns, size_t nt, const float init[7], const tc_kiss_icp_config *cfg,
                               const tc_icp_result *result, size_t *n_source_down) {
    if (!ctx || !cfg || !result || !init) return TC_INVALID_DATA;
    if (n_source_down) *n_source_down = 0;
    if (ns == 0 || nt == 0) return fail(ctx, TC_INVALID_DATA, "KISS-ICP: source or target point cloud is empty");     // :189-193
    if (cfg->max_iterations == 0) return fail(ctx, TC_INVALID_DATA, "KISS-ICP: max_iterations must be > 0");          // :194-198
    if (!(cfg->voxel_size > 0.0f)) return fail(ctx, TC_INVALID_DATA, "KISS-ICP: voxel_size must be > 0");             // :199-203
    return TC_OK;
}

tc_status tc_kiss_icp_device(tc_context *ctx, const float *d_source, size_t ns, const float *d_target, size_t nt, const float init[7],
                             const tc_kiss_icp_config *cfg, tc_icp_result *result, size_t *n_source_down) try {
    if (tc_status s = kiss_validate(ctx, ns, nt, init, cfg, result, n_source_down)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    ScopedBuf ranged, down;
    if (tc_status s = ensure(ctx, ranged, ns * 12)) return s;
    if (tc_status s = ensure(ctx, down, ns * 12)) return s;
    size_t nr = 0, nd = 0;
    if (tc_status s = range_filter_device(ctx, d_source, ns, cfg->min_range, cfg->max_range, (float *)ranged.p, &nr)) return s;
    if (nr == 0) return fail(ctx, TC_INVALID_DATA, "KISS-ICP: no source points remain after range filtering");   // :207-213
    if (tc_status s = voxel_filter_device(ctx, (const float *)ranged.p, nr, cfg->voxel_size, (float *)down.p, &nd)) return s;
    if (nd == 0) return fail(ctx, TC_INVALID_DATA, "KISS-ICP: no source points remain after voxel downsampling");
    if (n_source_down) *n_source_down = nd;
    const float sigma = kiss_adaptive_threshold(init, cfg->voxel_size);
    IcpJob job = p2p_job((const float *)down.p, nd, d_target, nt, init, cfg->max_iterations, sigma, 1e-6f);
    job.kiss = 1;
    return icp_run(ctx, job, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_kiss_icp(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt, const float init[7],
                      const tc_kiss_icp_config *cfg, tc_icp_result *result, size_t *n_source_down) try {
    if (tc_status s = kiss_validate(ctx, ns, nt, init, cfg, result, n_source_down)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->in_a, ns * 12)) return s;
    if (tc_status s = ensure(ctx, ctx->in_b, nt * 12)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_a.p, source, ns * 12, hipMemcpyHostToDevice, ctx->stream));      // (both on the context's stream: no overlap)
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_b.p, target, nt * 12, hipMemcpyHostToDevice, ctx->stream));
    CorrStandIn corr(result);
    if (tc_status s = corr.place(ctx, ns)) return s;
    size_t nd = 0;
    const tc_status st = tc_kiss_icp_device(ctx, (const float *)ctx->in_a.p, ns, (const float *)ctx->in_b.p, nt, init, cfg, result, &nd);
    corr.copy_back(st, nd);
    if (n_source_down) *n_source_down = nd;
    return st;
} TC_CATCH_STATUS(ctx)

// ---- GICP (gicp.rs:100-305; gicp_cov_kernel above) --------------------------------------------------
// the argument checks of both entry points (the host one makes them before it stages anything)
static tc_status gicp_validate(tc_context *ctx, size_t ns, size_t nt, const float init[7], const tc_gicp_config *cfg, const tc_icp_result *result) {
    if (!ctx || !cfg || !result || !init) return TC_INVALID_DATA;
    if (ns == 0 || nt == 0) return fail(ctx, TC_INVALID_DATA, "GICP: source or target point cloud is empty");           // :107-111
    if (cfg->max_iterations == 0) return fail(ctx, TC_INVALID_DATA, "GICP: max_iterations must be > 0");                // :112-116
    const size_t min_k = std::max<size_t>(cfg->k_correspondences, 4);
    if (ns < min_k || nt < min_k) return fail(ctx, TC_INVALID_DATA, "GICP: clouds must have at least k_correspondences points");   // :120-131
    return TC_OK;
}

tc_status tc_gicp_device(tc_context *ctx, const float *d_source, size_t ns, const float *d_target, size_t nt, const float init[7],
                         const tc_gicp_config *cfg, tc_icp_result *result) try {
    if (tc_status s = gicp_validate(ctx, ns, nt, init, cfg, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    const float *clouds[2] = {d_source, d_target};
    const size_t sizes[2] = {ns, nt};
    for (int c = 0; c < 2; ++c) {                                                                                       // :135-155
        float mn[3], mx[3];
        if (tc_status s = cloud_bbox(ctx, clouds[c], sizes[c], mn, mx)) return s;
        const float me = std::fmin(std::fmin(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
        if (me < 1e-4f) return fail(ctx, TC_INVALID_DATA, "GICP: point cloud appears to be coplanar or collinear; GICP requires 3-D structure");
    }
    ScopedBuf idx, dist, cnt, cov_s, cov_t;
    if (tc_status s = ensure(ctx, cov_s, ns * 8 * sizeof(float))) return s;
    if (tc_status s = ensure(ctx, cov_t, nt * 8 * sizeof(float))) return s;
    if (tc_status s = gicp_covariances_device(ctx, d_source, ns, cfg->k_correspondences, idx, dist, cnt, (float *)cov_s.p)) return s;
    if (tc_status s = gicp_covariances_device(ctx, d_target, nt, cfg->k_correspondences, idx, dist, cnt, (float *)cov_t.p)) return s;
    IcpJob job = p2p_job(d_source, ns, d_target, nt, init, cfg->max_iterations, cfg->max_correspondence_distance, cfg->convergence_threshold);
    job.mode = 2; job.cov_src = (const float *)cov_s.p; job.cov_tgt = (const float *)cov_t.p;
    return icp_run(ctx, job, result);
} TC_CATCH_STATUS(ctx)

tc_status tc_gicp(tc_context *ctx, const float *source, size_t ns, const float *target, size_t nt, const float init[7],
                  const tc_gicp_config *cfg, tc_icp_result *result) try {
    if (tc_status s = gicp_validate(ctx, ns, nt, init, cfg, result)) return s;
    TC_HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (tc_status s = ensure(ctx, ctx->in_a, ns * 12)) return s;
    if (tc_status s = ensure(ctx, ctx->in_b, nt * 12)) return s;
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_a.p, source, ns * 12, hipMemcpyHostToDevice, ctx->stream));      // (both on the context's stream: no overlap)
    TC_HIP_TRY(ctx, hipMemcpyAsync(ctx->in_b.p, target, nt * 12, hipMemcpyHostToDevice, ctx->stream));
    CorrStandIn corr(result);
    if (tc_status s = corr.place(ctx, ns)) return s;
    const tc_status st = tc_gicp_device(ctx, (const float *)ctx->in_a.p, ns, (const float *)ctx->in_b.p, nt, init, cfg, result);
    corr.copy_back(st, ns);
    return st;
} TC_CATCH_STATUS(ctx)

}  // extern "C"
