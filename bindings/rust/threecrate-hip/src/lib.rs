//! threecrate-hip: the normals + ICP path of threecrate on an AMD MI355X, behind the signatures of
//! threecrate-algorithms (`estimate_normals*`, `icp*`, `icp_point_to_point[_default]`, `icp_point_to_plane*`,
//! `multiscale_icp_point_to_point`, `gicp`, `kiss_icp`, `voxel_grid_filter`, `extract_euclidean_clusters[_parallel]`,
//! `extract_fpfh_features[_with_normals]`, `statistical_outlier_removal[_with_threshold]`, `radius_outlier_removal`,
//! `segment_plane`, `segment_plane_ransac`, `plane_segmentation_ransac`) and of the
//! `threecrate-gpu` facade
//! (`gpu_estimate_normals`, `gpu_icp`, `gpu_icp_point_to_plane`, `gpu_batch_icp`, `gpu_voxel_grid_filter`,
//! `gpu_find_k_nearest[_batch]`, `gpu_find_radius_neighbors`, `gpu_extract_euclidean_clusters`, `gpu_extract_clusters`, `gpu_remove_statistical_outliers`, `gpu_radius_outlier_removal`, `gpu_segment_plane`, `gpu_segment_plane_ransac`; the reference's are `async fn`s around a wgpu queue, these
//! return when the result is there).  tests/test_abi_conformance.py checks that every name listed here has its `pub fn`
//! and that ffi.rs declares every `tc_*` export of the header.  Every function takes a [`HipContext`] (the role `GpuContext` plays in
//! threecrate-gpu: one device + one stream; not thread-safe, one context per thread / GPU).
//!
//! Layout facts the zero-copy calls rely on: `Point3f` = `nalgebra::Point3<f32>` is three contiguous f32
//! (threecrate-core/src/point.rs:8), `NormalPoint3f` is `#[repr(C)] { position, normal }` (point.rs:31-36),
//! `Isometry3<f32>` is passed as (qi, qj, qk, qw, tx, ty, tz).
pub mod ffi;
pub mod ffi_filters;
pub mod ffi_segmentation;
pub mod ffi_ndt;
pub mod ffi_tsdf;
pub mod ffi_global;
pub mod ffi_voxelmap;
pub mod ffi_color;
pub mod ffi_mesh;
pub mod ffi_simplify;
pub mod ffi_mc;
pub mod ffi_qem;
pub mod ffi_alpha;
pub mod ffi_ground;
pub mod ffi_shot;
pub mod ffi_poisson;

use nalgebra::{Isometry3, Matrix4, Point3, Quaternion, Translation3, UnitQuaternion, Vector4};
use std::ffi::CStr;
use threecrate_algorithms::{ClusterExtractionResult, EuclideanClusterConfig, GicpConfig, ICPResult, IcpScaleLevel, KissIcpConfig, MultiScaleIcpConfig, NormalEstimationConfig};
use threecrate_core::{ColoredPoint3f, Error, NearestNeighborSearch, NormalPoint3f, Point3f, PointCloud, Result, Vector3f};

/// One HIP device + stream + the library's grow-only device buffers (`tc_context`).
pub struct HipContext(*mut ffi::tc_context);

// the context is only ever used from the thread that owns the value
unsafe impl Send for HipContext {}

impl HipContext {
    /// `GpuContext::new` (threecrate-gpu/src/device.rs:16-50).  `Error::Gpu` when no MI355X is usable.
    pub fn new(device: i32) -> Result<Self> {
        let mut h: *mut ffi::tc_context = std::ptr::null_mut();
        let rc = unsafe { ffi::tc_context_create(device, &mut h) };
        if rc != ffi::TC_OK || h.is_null() {
            return Err(Error::Gpu(format!("no usable HIP device {device} (tc_status {rc})")));
        }
        Ok(HipContext(h))
    }

    fn check(&self, rc: i32) -> Result<()> {
        if rc == ffi::TC_OK {
            return Ok(());
        }
        let msg = unsafe {
            let p = ffi::tc_last_error_message(self.0);
            if p.is_null() { String::new() } else { CStr::from_ptr(p).to_string_lossy().into_owned() }
        };
        Err(match rc {                                   // threecrate-core/src/error.rs:7-28
            ffi::TC_INVALID_DATA => Error::InvalidData(msg),
            ffi::TC_ALGORITHM => Error::Algorithm(msg),
            ffi::TC_UNSUPPORTED => Error::Unsupported(msg),
            _ => Error::Gpu(msg),
        })
    }
}

impl Drop for HipContext {
    fn drop(&mut self) {
        unsafe { ffi::tc_context_destroy(self.0) }
    }
}

fn iso_to7(t: &Isometry3<f32>) -> [f32; 7] {
    let q = t.rotation.quaternion().coords;              // (i, j, k, w)
    [q[0], q[1], q[2], q[3], t.translation.x, t.translation.y, t.translation.z]
}

fn iso_from7(t: &[f32; 7]) -> Isometry3<f32> {
    Isometry3::from_parts(
        Translation3::new(t[4], t[5], t[6]),
        UnitQuaternion::new_unchecked(Quaternion::new(t[3], t[0], t[1], t[2])),   // Quaternion::new(w, i, j, k)
    )
}

fn xyz(cloud: &PointCloud<Point3f>) -> *const f32 {
    cloud.points.as_ptr() as *const f32
}

fn result_from(r: &ffi::tc_icp_result, corr: &[u32], n_valid: usize) -> ICPResult {
    ICPResult {
        transformation: iso_from7(&r.transformation),
        mse: r.mse,
        iterations: r.iterations as usize,
        converged: r.converged != 0,
        correspondences: corr[..n_valid].iter().enumerate().filter(|(_, &t)| t != u32::MAX).map(|(s, &t)| (s, t as usize)).collect(),
    }
}

/// `Option<f32>` -> the ABI's encoding (< 0 = None).  A negative `Some(d)` must not alias `None`: the reference rejects every
/// pair then (`distance > d` always holds, registration.rs:100-101) and fails with "Insufficient correspondences" -- AFTER its
/// own validation (registration.rs:266-276 / :517-531: empty clouds, the normals' length, max_iterations == 0 are InvalidData
/// first), which therefore runs here in the same order before the Algorithm error is returned.
fn encode_max_dist(d: Option<f32>, ns: usize, nt: usize, max_iters: usize, normals_len: Option<usize>) -> Result<f32> {
    match d {
        None => Ok(-1.0),
        Some(v) if v < 0.0 => {
            if ns == 0 || nt == 0 {
                return Err(Error::InvalidData("Source or target point cloud is empty".to_string()));
            }
            if let Some(nn) = normals_len {
                if nn != nt {
                    return Err(Error::InvalidData("target_normals length must equal the number of target points".to_string()));
                }
            }
            if max_iters == 0 {
                return Err(Error::InvalidData("Max iterations must be positive".to_string()));
            }
            Err(Error::Algorithm("Insufficient correspondences found".to_string()))
        }
        Some(v) => Ok(v),
    }
}

fn empty_result(corr: &mut Vec<u32>) -> ffi::tc_icp_result {
    ffi::tc_icp_result { transformation: [0.0; 7], mse: 0.0, iterations: 0, converged: 0, n_correspondences: 0, corr_target: corr.as_mut_ptr() }
}

// ---- normals (threecrate-algorithms/src/normals.rs:238-380) ------------------------------------------------

/// `estimate_normals_with_config` (normals.rs:257-260)
pub fn estimate_normals_with_config(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: &NormalEstimationConfig)
    -> Result<PointCloud<NormalPoint3f>> {
    let n = cloud.points.len();
    let cfg = ffi::tc_normal_config {
        k_neighbors: config.k_neighbors as u64,
        radius: config.radius.unwrap_or(0.0),
        has_radius: config.radius.is_some() as i32,
        consistent_orientation: config.consistent_orientation as i32,
        has_viewpoint: config.viewpoint.is_some() as i32,
        viewpoint: config.viewpoint.map(|p| [p.x, p.y, p.z]).unwrap_or([0.0; 3]),
    };
    let mut out: Vec<NormalPoint3f> = Vec::with_capacity(n);
    ctx.check(unsafe { ffi::tc_estimate_normals(ctx.0, xyz(cloud), n, &cfg, out.as_mut_ptr() as *mut f32) })?;
    unsafe { out.set_len(n) };
    Ok(PointCloud::from_points(out))
}

/// `estimate_normals` (normals.rs:238-241)
pub fn estimate_normals(ctx: &HipContext, cloud: &PointCloud<Point3f>, k: usize) -> Result<PointCloud<NormalPoint3f>> {
    let config = NormalEstimationConfig { k_neighbors: k, ..Default::default() };
    estimate_normals_with_config(ctx, cloud, &config)
}

/// `estimate_normals_radius` (normals.rs:368-380)
pub fn estimate_normals_radius(ctx: &HipContext, cloud: &PointCloud<Point3f>, radius: f32, consistent_orientation: bool)
    -> Result<PointCloud<NormalPoint3f>> {
    let config = NormalEstimationConfig { k_neighbors: 10, radius: Some(radius), consistent_orientation, viewpoint: None };
    estimate_normals_with_config(ctx, cloud, &config)
}

// ---- ICP (threecrate-algorithms/src/registration.rs) ---------------------------------------------------------

/// `icp_detailed` (registration.rs:258-265)
pub fn icp_detailed(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>,
                    max_iters: usize, max_correspondence_distance: Option<f32>, convergence_threshold: f32) -> Result<ICPResult> {
    let ns = source.points.len();
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    ctx.check(unsafe {
        ffi::tc_icp_detailed(ctx.0, xyz(source), ns, xyz(target), target.points.len(), i7.as_ptr(), max_iters,
                             encode_max_dist(max_correspondence_distance, ns, target.points.len(), max_iters, None)?, convergence_threshold, &mut r)
    })?;
    Ok(result_from(&r, &corr, ns))
}

/// `icp` (registration.rs:232-242): any error returns `init`
pub fn icp(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>, max_iters: usize)
    -> Isometry3<f32> {
    match icp_detailed(ctx, source, target, init, max_iters, None, 1e-6) {
        Ok(r) => r.transformation,
        Err(_) => init,
    }
}

/// `icp_point_to_point` (registration.rs:644-680)
pub fn icp_point_to_point(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>,
                          max_iterations: usize, convergence_threshold: f32, max_correspondence_distance: Option<f32>) -> Result<ICPResult> {
    let ns = source.points.len();
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    ctx.check(unsafe {
        ffi::tc_icp_point_to_point(ctx.0, xyz(source), ns, xyz(target), target.points.len(), i7.as_ptr(), max_iterations,
                                   convergence_threshold, encode_max_dist(max_correspondence_distance, ns, target.points.len(), max_iterations, None)?, &mut r)
    })?;
    Ok(result_from(&r, &corr, ns))
}

/// `icp_point_to_point_default` (registration.rs:694-701): threshold 1e-6, no correspondence cut-off
pub fn icp_point_to_point_default(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>,
                                  max_iterations: usize) -> Result<ICPResult> {
    icp_point_to_point(ctx, source, target, init, max_iterations, 1e-6, None)
}

/// `multiscale_icp_point_to_point` (registration.rs:704-789): voxel-downsampled coarse-to-fine levels, then a final refinement on
/// the full clouds; the levels run on the device (tc_multiscale_icp_point_to_point), validation order and messages as the reference's.
/// A negative `Some(d)` cut-off of a level is passed through as `Some` (`f32::MIN_POSITIVE` keeps it from aliasing `None`; the level
/// then rejects every pair like the reference does).
pub fn multiscale_icp_point_to_point(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>,
                                     config: &MultiScaleIcpConfig) -> Result<ICPResult> {
    let ns = source.points.len();
    let enc = |d: Option<f32>| match d { None => -1.0f32, Some(v) if v < 0.0 => f32::MIN_POSITIVE, Some(v) => v };
    let levels: Vec<ffi::tc_icp_scale_level> = config.levels.iter().map(|l: &IcpScaleLevel| ffi::tc_icp_scale_level {
        voxel_size: l.voxel_size, max_iterations: l.max_iterations, max_correspondence_distance: enc(l.max_correspondence_distance),
    }).collect();
    let cfg = ffi::tc_multiscale_icp_config {
        levels: levels.as_ptr(), n_levels: levels.len(),
        final_refinement_iterations: config.final_refinement_iterations,
        final_max_correspondence_distance: enc(config.final_max_correspondence_distance),
        convergence_threshold: config.convergence_threshold,
    };
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    ctx.check(unsafe { ffi::tc_multiscale_icp_point_to_point(ctx.0, xyz(source), ns, xyz(target), target.points.len(), i7.as_ptr(), &cfg, &mut r) })?;
    Ok(result_from(&r, &corr, ns))
}

/// `icp_point_to_plane_detailed` (registration.rs:508-516)
pub fn icp_point_to_plane_detailed(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>,
                                   target_normals: &[Vector3f], init: Isometry3<f32>, max_iters: usize,
                                   max_correspondence_distance: Option<f32>, convergence_threshold: f32) -> Result<ICPResult> {
    let ns = source.points.len();
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    ctx.check(unsafe {
        ffi::tc_icp_point_to_plane_detailed(ctx.0, xyz(source), ns, xyz(target), target.points.len(),
                                            target_normals.as_ptr() as *const f32, target_normals.len(), 3, i7.as_ptr(), max_iters,
                                            encode_max_dist(max_correspondence_distance, ns, target.points.len(), max_iters, Some(target_normals.len()))?,
                                            convergence_threshold, &mut r)
    })?;
    Ok(result_from(&r, &corr, ns))
}

/// `icp_point_to_plane` (registration.rs:488-494)
pub fn icp_point_to_plane(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, target_normals: &[Vector3f],
                          init: Isometry3<f32>, max_iters: usize) -> Result<ICPResult> {
    icp_point_to_plane_detailed(ctx, source, target, target_normals, init, max_iters, None, 1e-6)
}

/// `gicp` (gicp.rs:100-105)
pub fn gicp(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>, config: GicpConfig)
    -> Result<ICPResult> {
    let ns = source.points.len();
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    let cfg = ffi::tc_gicp_config {
        max_iterations: config.max_iterations,
        max_correspondence_distance: config.max_correspondence_distance,
        convergence_threshold: config.convergence_threshold,
        k_correspondences: config.k_correspondences,
    };
    ctx.check(unsafe { ffi::tc_gicp(ctx.0, xyz(source), ns, xyz(target), target.points.len(), i7.as_ptr(), &cfg, &mut r) })?;
    Ok(result_from(&r, &corr, ns))
}

/// `kiss_icp` (kiss_icp.rs:183-188).  Correspondence source indices refer to the voxel-downsampled source.
pub fn kiss_icp(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, init: Isometry3<f32>, config: KissIcpConfig)
    -> Result<ICPResult> {
    let ns = source.points.len();
    let mut corr = vec![u32::MAX; ns.max(1)];
    let mut r = empty_result(&mut corr);
    let i7 = iso_to7(&init);
    let cfg = ffi::tc_kiss_icp_config { voxel_size: config.voxel_size, max_range: config.max_range, min_range: config.min_range,
                                        max_iterations: config.max_iterations };
    let mut n_down = 0usize;
    ctx.check(unsafe { ffi::tc_kiss_icp(ctx.0, xyz(source), ns, xyz(target), target.points.len(), i7.as_ptr(), &cfg, &mut r, &mut n_down) })?;
    Ok(result_from(&r, &corr, n_down))
}

// ---- filters / neighbour search ----------------------------------------------------------------------------

/// `voxel_grid_filter` (filtering.rs:38-133); voxels come out sorted by (kx, ky, kz)
pub fn voxel_grid_filter(ctx: &HipContext, cloud: &PointCloud<Point3f>, voxel_size: f32) -> Result<PointCloud<Point3f>> {
    let n = cloud.points.len();
    let mut out: Vec<Point3f> = Vec::with_capacity(n.max(1));
    let mut n_out = 0usize;
    ctx.check(unsafe { ffi::tc_voxel_grid_filter(ctx.0, xyz(cloud), n, voxel_size, out.as_mut_ptr() as *mut f32, &mut n_out) })?;
    unsafe { out.set_len(n_out) };
    Ok(PointCloud::from_points(out))
}

/// the kept points of an outlier filter: `call` gets (out_xyz, n_out) and returns the status
fn kept_points(ctx: &HipContext, n: usize, call: impl FnOnce(*mut f32, *mut usize) -> i32) -> Result<PointCloud<Point3f>> {
    let mut out: Vec<Point3f> = Vec::with_capacity(n.max(1));
    let mut n_out = 0usize;
    ctx.check(call(out.as_mut_ptr() as *mut f32, &mut n_out))?;
    unsafe { out.set_len(n_out) };
    Ok(PointCloud::from_points(out))
}

/// `statistical_outlier_removal` (filtering.rs:249-321): the kept points in input order.  The global mean and variance are
/// summed in f64 (include/threecrate_hip_filters.h lists the deviations).
pub fn statistical_outlier_removal(ctx: &HipContext, cloud: &PointCloud<Point3f>, k_neighbors: usize, std_dev_multiplier: f32) -> Result<PointCloud<Point3f>> {
    let n = cloud.points.len();
    kept_points(ctx, n, |out, n_out| unsafe {
        ffi_filters::tc_statistical_outlier_removal(ctx.0, xyz(cloud), n, k_neighbors, std_dev_multiplier, out, std::ptr::null_mut(),
                                                    std::ptr::null_mut(), n_out, std::ptr::null_mut())
    })
}

/// `statistical_outlier_removal_with_threshold` (filtering.rs:335-395)
pub fn statistical_outlier_removal_with_threshold(ctx: &HipContext, cloud: &PointCloud<Point3f>, k_neighbors: usize, threshold: f32) -> Result<PointCloud<Point3f>> {
    let n = cloud.points.len();
    kept_points(ctx, n, |out, n_out| unsafe {
        ffi_filters::tc_statistical_outlier_removal_with_threshold(ctx.0, xyz(cloud), n, k_neighbors, threshold, out, std::ptr::null_mut(),
                                                                   std::ptr::null_mut(), n_out)
    })
}

/// `radius_outlier_removal` (filtering.rs:167-213)
pub fn radius_outlier_removal(ctx: &HipContext, cloud: &PointCloud<Point3f>, radius: f32, min_neighbors: usize) -> Result<PointCloud<Point3f>> {
    let n = cloud.points.len();
    kept_points(ctx, n, |out, n_out| unsafe {
        ffi_filters::tc_radius_outlier_removal(ctx.0, xyz(cloud), n, radius, min_neighbors, out, std::ptr::null_mut(), n_out)
    })
}

/// `gpu_remove_statistical_outliers(&ctx, &cloud, k_neighbors, std_dev_multiplier)` (threecrate-gpu/src/filtering.rs:882-893) with
/// the CPU filter's semantics
pub fn gpu_remove_statistical_outliers(ctx: &HipContext, cloud: &PointCloud<Point3f>, k_neighbors: usize, std_dev_multiplier: f32) -> Result<PointCloud<Point3f>> {
    statistical_outlier_removal(ctx, cloud, k_neighbors, std_dev_multiplier)
}

/// `gpu_radius_outlier_removal(&ctx, &cloud, radius, min_neighbors)` (threecrate-gpu/src/filtering.rs:895-905)
pub fn gpu_radius_outlier_removal(ctx: &HipContext, cloud: &PointCloud<Point3f>, radius: f32, min_neighbors: usize) -> Result<PointCloud<Point3f>> {
    radius_outlier_removal(ctx, cloud, radius, min_neighbors)
}

/// `PlaneModel` (threecrate-algorithms/src/segmentation.rs:12-17): a*x + b*y + c*z + d = 0
#[derive(Debug, Clone, PartialEq)]
pub struct PlaneModel {
    pub coefficients: Vector4<f32>,
}

/// `PlaneSegmentationResult` (segmentation.rs:94-103)
#[derive(Debug, Clone)]
pub struct PlaneSegmentationResult {
    pub model: PlaneModel,
    pub inliers: Vec<usize>,
    pub iterations: usize,
}

/// One seeded call: coefficients, the inliers' ascending indices, the winning iteration
fn plane_call(ctx: &HipContext, cloud: &PointCloud<Point3f>, threshold: f32, max_iters: usize, seed: u64) -> Result<(Vector4<f32>, Vec<u32>, u32)> {
    let n = cloud.points.len();
    let mut coeff = [0f32; 4];
    let mut index: Vec<u32> = Vec::with_capacity(n.max(1));
    let (mut n_in, mut best) = (0usize, 0u32);
    ctx.check(unsafe {
        ffi_segmentation::tc_segment_plane(ctx.0, xyz(cloud), n, threshold, max_iters, seed, coeff.as_mut_ptr(), index.as_mut_ptr(), &mut n_in, &mut best)
    })?;
    unsafe { index.set_len(n_in) };
    Ok((Vector4::new(coeff[0], coeff[1], coeff[2], coeff[3]), index, best))
}

/// `segment_plane(&cloud, threshold, max_iters)` (segmentation.rs:117-180).  The triples come from the GPU facade's deterministic
/// generator, not from the thread's RNG: the same call returns the same plane; equal scores go to the lowest iteration.
pub fn segment_plane(ctx: &HipContext, cloud: &PointCloud<Point3f>, threshold: f32, max_iters: usize) -> Result<PlaneSegmentationResult> {
    let (coefficients, index, _) = plane_call(ctx, cloud, threshold, max_iters, 0)?;
    Ok(PlaneSegmentationResult { model: PlaneModel { coefficients }, inliers: index.into_iter().map(|i| i as usize).collect(), iterations: max_iters })
}

/// `segment_plane_ransac(&cloud, max_iters, threshold)` (segmentation.rs:297-304; note the argument order)
pub fn segment_plane_ransac(ctx: &HipContext, cloud: &PointCloud<Point3f>, max_iters: usize, threshold: f32) -> Result<(Vector4<f32>, Vec<usize>)> {
    let r = segment_plane(ctx, cloud, threshold, max_iters)?;
    Ok((r.model.coefficients, r.inliers))
}

/// `plane_segmentation_ransac` (segmentation.rs:318-324): an alias
pub fn plane_segmentation_ransac(ctx: &HipContext, cloud: &PointCloud<Point3f>, max_iters: usize, threshold: f32) -> Result<(Vector4<f32>, Vec<usize>)> {
    segment_plane_ransac(ctx, cloud, max_iters, threshold)
}

/// `GpuPlaneModel` (threecrate-gpu/src/segmentation.rs:149-152)
#[derive(Debug, Clone, PartialEq)]
pub struct GpuPlaneModel {
    pub coefficients: Vector4<f32>,
}

/// `GpuPlaneSegmentationResult` (threecrate-gpu/src/segmentation.rs:183-192): `plane` and `model` are the same model
#[derive(Debug, Clone)]
pub struct GpuPlaneSegmentationResult {
    pub plane: GpuPlaneModel,
    pub model: GpuPlaneModel,
    pub inliers: Vec<u32>,
    pub iterations: usize,
}

/// `GpuPlaneSegmentationConfig` (threecrate-gpu/src/segmentation.rs:196-213): same fields and defaults
#[derive(Debug, Clone, Copy)]
pub struct GpuPlaneSegmentationConfig {
    pub max_iterations: usize,
    pub distance_threshold: f32,
    pub min_inliers: usize,
}

impl Default for GpuPlaneSegmentationConfig {
    fn default() -> Self {
        Self { max_iterations: 1_000, distance_threshold: 0.02, min_inliers: 1 }
    }
}

/// `gpu_segment_plane_ransac(&ctx, &cloud, threshold, max_iters)` (threecrate-gpu/src/segmentation.rs:822-831).  Deviations from
/// the facade (include/threecrate_hip_segmentation.h): the first of equal scores wins, and the score divides by the normal's length.
pub fn gpu_segment_plane_ransac(ctx: &HipContext, cloud: &PointCloud<Point3f>, threshold: f32, max_iters: usize) -> Result<GpuPlaneSegmentationResult> {
    let (coefficients, inliers, _) = plane_call(ctx, cloud, threshold, max_iters, 0)?;
    let model = GpuPlaneModel { coefficients };
    Ok(GpuPlaneSegmentationResult { plane: model.clone(), model, inliers, iterations: max_iters })
}

/// `gpu_segment_plane(&ctx, &cloud, config)` (threecrate-gpu/src/segmentation.rs:304-324, :813-819, checks :853-861)
pub fn gpu_segment_plane(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: GpuPlaneSegmentationConfig) -> Result<GpuPlaneSegmentationResult> {
    if cloud.points.len() >= 3 && !(config.distance_threshold <= 0.0) && config.max_iterations != 0 && config.min_inliers == 0 {
        return Err(Error::InvalidData("min_inliers must be at least 1".to_string()));
    }
    let r = gpu_segment_plane_ransac(ctx, cloud, config.distance_threshold, config.max_iterations)?;
    if r.inliers.len() < config.min_inliers {
        return Err(Error::Algorithm(format!("Plane model has {} inliers, below required minimum {}", r.inliers.len(), config.min_inliers)));
    }
    Ok(r)
}

/// Clusters as index lists (largest first; equal sizes by smallest index; indices ascending inside a cluster)
fn cluster_indices(ctx: &HipContext, cloud: &PointCloud<Point3f>, tolerance: f32, min_size: usize, max_size: usize) -> Result<Vec<Vec<usize>>> {
    let n = cloud.points.len();
    let mut members = vec![0u32; n.max(1)];
    let mut offsets = vec![0u64; n / min_size.max(1) + 1];
    let mut n_clusters = 0usize;
    ctx.check(unsafe {
        ffi::tc_extract_euclidean_clusters(ctx.0, xyz(cloud), n, tolerance, min_size, max_size, std::ptr::null_mut(), members.as_mut_ptr(),
                                           offsets.as_mut_ptr(), &mut n_clusters)
    })?;
    Ok((0..n_clusters).map(|k| members[offsets[k] as usize..offsets[k + 1] as usize].iter().map(|&i| i as usize).collect()).collect())
}

/// `extract_euclidean_clusters` (segmentation.rs:396-455): the same clusters in the same order; inside a cluster the indices are
/// ascending (the CPU path lists them in BFS order)
pub fn extract_euclidean_clusters(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: &EuclideanClusterConfig) -> Result<ClusterExtractionResult> {
    let clusters = cluster_indices(ctx, cloud, config.tolerance, config.min_cluster_size, config.max_cluster_size)?;
    Ok(ClusterExtractionResult { clusters })
}

/// `extract_euclidean_clusters_parallel` (segmentation.rs:466-525): same result as the serial function
pub fn extract_euclidean_clusters_parallel(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: &EuclideanClusterConfig) -> Result<ClusterExtractionResult> {
    extract_euclidean_clusters(ctx, cloud, config)
}

/// `gpu_find_k_nearest_batch` (threecrate-gpu/src/nearest_neighbor.rs:345-355)
pub fn find_k_nearest_batch(ctx: &HipContext, points: &[Point3f], queries: &[Point3f], k: usize) -> Result<Vec<Vec<(usize, f32)>>> {
    let nq = queries.len();
    let kk = k.max(1);
    let (mut idx, mut dist, mut cnt) = (vec![0u32; nq * kk], vec![0f32; nq * kk], vec![0u32; nq.max(1)]);
    ctx.check(unsafe {
        ffi::tc_knn(ctx.0, points.as_ptr() as *const f32, points.len(), queries.as_ptr() as *const f32, nq, k, idx.as_mut_ptr(),
                    dist.as_mut_ptr(), cnt.as_mut_ptr())
    })?;
    Ok((0..nq).map(|q| (0..cnt[q] as usize).map(|j| (idx[q * kk + j] as usize, dist[q * kk + j])).collect()).collect())
}

/// longest neighbour list of the device k-NN kernels (threecrate_hip.h, "Limits of this backend")
pub const KNN_MAX_K: usize = 2047;

/// The `KdTree` of this backend: built once, queried many times (`KdTree::new`, nearest_neighbor.rs:37-58).
/// Implements `threecrate_core::NearestNeighborSearch` (core/traits.rs:6-12), so it drops into code that is generic
/// over the trait.  Borrows the context: destroy order is enforced by the lifetime.
pub struct HipKdTree<'a> {
    ctx: &'a HipContext,
    raw: *mut ffi::tc_search_index,
}

impl<'a> HipKdTree<'a> {
    pub fn new(ctx: &'a HipContext, points: &[Point3f]) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        ctx.check(unsafe { ffi::tc_search_index_create(ctx.0, points.as_ptr() as *const f32, points.len(), 16, &mut raw) })?;
        Ok(Self { ctx, raw })
    }

    pub fn len(&self) -> usize { unsafe { ffi::tc_search_index_size(self.raw) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }

    fn query(&self, queries: &[Point3f], k: usize, radius: f32) -> Result<Vec<Vec<(usize, f32)>>> {
        let nq = queries.len();
        let kk = k.max(1);
        let (mut idx, mut dist, mut cnt) = (vec![0u32; nq * kk], vec![0f32; nq * kk], vec![0u32; nq.max(1)]);
        self.ctx.check(unsafe {
            ffi::tc_search_index_query(self.raw, queries.as_ptr() as *const f32, nq, k, radius, idx.as_mut_ptr(), dist.as_mut_ptr(), cnt.as_mut_ptr())
        })?;
        Ok((0..nq).map(|q| (0..cnt[q] as usize).map(|j| (idx[q * kk + j] as usize, dist[q * kk + j])).collect()).collect())
    }

    /// many queries in one launch
    pub fn find_k_nearest_batch(&self, queries: &[Point3f], k: usize) -> Result<Vec<Vec<(usize, f32)>>> {
        self.query(queries, k, -1.0)
    }
}

impl NearestNeighborSearch for HipKdTree<'_> {
    /// `KdTree::find_k_nearest` (nearest_neighbor.rs:177-251): the `min(k, len())` nearest, ascending.  The device list holds up to
    /// `KNN_MAX_K` = 2047 entries (threecrate_hip.h "Limits of this backend"; a larger k is TC_UNSUPPORTED at the ABI).  The trait
    /// returns a plain Vec and the reference's tree has no cap, so a larger k is served from radius sets: the k nearest are the
    /// first k of any ball that holds at least k records -- the radius starts at the 2047th neighbour's distance scaled by
    /// cbrt(k / 2047) and doubles until the count reaches k (at most a few rounds; `f32::MAX` covers every finite cloud).
    fn find_k_nearest(&self, query: &Point3f, k: usize) -> Vec<(usize, f32)> {
        let k = k.min(self.len());
        if k == 0 { return Vec::new(); }
        if k <= KNN_MAX_K {
            return self.query(std::slice::from_ref(query), k, -1.0).map(|mut v| v.remove(0)).unwrap_or_default();
        }
        let seed = match self.query(std::slice::from_ref(query), KNN_MAX_K, -1.0) { Ok(mut v) => v.remove(0), Err(_) => return Vec::new() };
        let r0 = seed.last().map(|e| e.1).unwrap_or(0.0);
        let mut r = if r0 > 0.0 && r0.is_finite() { r0 * (k as f32 / KNN_MAX_K as f32).cbrt() * 1.05 } else { 1.0e-6 };
        let q = query as *const Point3f as *const f32;
        loop {
            let mut count = 0u32;
            if self.ctx.check(unsafe { ffi::tc_search_index_radius_count(self.raw, q, 1, r, &mut count) }).is_err() { return Vec::new(); }
            if count as usize >= k || r >= f32::MAX { break; }
            r = if r < f32::MAX / 2.0 { r * 2.0 } else { f32::MAX };
        }
        let mut out = self.find_radius_neighbors(query, r);          // ascending by distance
        out.truncate(k);
        out
    }

    /// every neighbour within `radius`, nearest first (nearest_neighbor.rs:254-298): count, then fill
    fn find_radius_neighbors(&self, query: &Point3f, radius: f32) -> Vec<(usize, f32)> {
        if !(radius > 0.0) || self.is_empty() { return Vec::new(); }
        let q = query as *const Point3f as *const f32;
        let mut count = 0u32;
        if self.ctx.check(unsafe { ffi::tc_search_index_radius_count(self.raw, q, 1, radius, &mut count) }).is_err() { return Vec::new(); }
        let total = count as usize;
        let (mut idx, mut dist, offsets) = (vec![0u32; total], vec![0f32; total], [0u64]);
        if total > 0 && self.ctx.check(unsafe {
            ffi::tc_search_index_radius_fill(self.raw, q, 1, radius, offsets.as_ptr(), total, idx.as_mut_ptr(), dist.as_mut_ptr())
        }).is_err() { return Vec::new(); }
        let mut out: Vec<(usize, f32)> = idx.into_iter().map(|i| i as usize).zip(dist).collect();
        out.sort_by(|a, b| a.1.partial_cmp(&b.1).unwrap_or(std::cmp::Ordering::Equal));
        out
    }
}

impl Drop for HipKdTree<'_> {
    fn drop(&mut self) { unsafe { ffi::tc_search_index_destroy(self.raw) } }
}

// ---- threecrate-gpu facade (gpu/normals.rs:443-447, gpu/icp.rs:977-1025) ---------------------------------------

/// `gpu_icp(&ctx, source, target, max_iterations, convergence_threshold, max_correspondence_distance)`
pub fn gpu_icp(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, max_iterations: usize,
               convergence_threshold: f32, max_correspondence_distance: f32) -> Result<Isometry3<f32>> {
    Ok(icp_point_to_point(ctx, source, target, Isometry3::identity(), max_iterations, convergence_threshold,
                          Some(max_correspondence_distance))?.transformation)
}

/// `gpu_estimate_normals(&ctx, &mut cloud, k)`
pub fn gpu_estimate_normals(ctx: &HipContext, cloud: &mut PointCloud<Point3f>, k: usize) -> Result<PointCloud<NormalPoint3f>> {
    estimate_normals(ctx, cloud, k)
}

/// `GpuPointToPlaneICPResult` (threecrate-gpu/src/icp.rs:821-828)
#[derive(Debug, Clone)]
pub struct GpuPointToPlaneICPResult {
    pub transformation: Isometry3<f32>,
    pub final_error: f32,
    pub iterations: usize,
    pub converged: bool,
}

/// `gpu_icp_point_to_plane(&ctx, source, target, target_normals, max_iterations, convergence_threshold,
/// max_correspondence_distance)` (threecrate-gpu/src/icp.rs:1017-1036); starts from the identity like the reference's.
pub fn gpu_icp_point_to_plane(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, target_normals: &[Vector3f],
                              max_iterations: usize, convergence_threshold: f32, max_correspondence_distance: f32)
    -> Result<GpuPointToPlaneICPResult> {
    let r = icp_point_to_plane_detailed(ctx, source, target, target_normals, Isometry3::identity(), max_iterations,
                                        Some(max_correspondence_distance), convergence_threshold)?;
    Ok(GpuPointToPlaneICPResult { transformation: r.transformation, final_error: r.mse, iterations: r.iterations, converged: r.converged })
}

/// `BatchICPJob` (threecrate-gpu/src/icp.rs:132-139)
#[derive(Debug, Clone)]
pub struct BatchICPJob {
    pub source: PointCloud<Point3f>,
    pub target: PointCloud<Point3f>,
    pub max_iterations: usize,
    pub convergence_threshold: f32,
    pub max_correspondence_distance: f32,
}

/// `BatchICPResult` (threecrate-gpu/src/icp.rs:142-147)
#[derive(Debug, Clone)]
pub struct BatchICPResult {
    pub transformation: Isometry3<f32>,
    pub final_error: f32,
    pub iterations: usize,
}

/// `gpu_batch_icp(&ctx, &jobs)` (threecrate-gpu/src/icp.rs:997-1002, semantics :151-185): independent pairs, each from the
/// identity.  Job i runs on `contexts[i % contexts.len()]` -- one context per GPU of the node gives one pair per GPU
/// (tc_batch_icp: a host thread per context).  A job that fails returns its error for the whole batch, like the reference's `?`.
pub fn gpu_batch_icp(contexts: &[&HipContext], jobs: &[BatchICPJob]) -> Result<Vec<BatchICPResult>> {
    if contexts.is_empty() {
        return Err(Error::InvalidData("gpu_batch_icp needs at least one context".to_string()));
    }
    let raw_ctx: Vec<*mut ffi::tc_context> = contexts.iter().map(|c| c.0).collect();
    let cj: Vec<ffi::tc_batch_icp_job> = jobs.iter().map(|j| ffi::tc_batch_icp_job {
        source: xyz(&j.source), n_source: j.source.points.len(), target: xyz(&j.target), n_target: j.target.points.len(),
        max_iterations: j.max_iterations, convergence_threshold: j.convergence_threshold,
        max_correspondence_distance: j.max_correspondence_distance,
    }).collect();
    let mut cr = vec![ffi::tc_batch_icp_result { transformation: [0.0; 7], final_error: 0.0, iterations: 0, status: ffi::TC_OK }; jobs.len()];
    let rc = unsafe { ffi::tc_batch_icp(raw_ctx.as_ptr(), raw_ctx.len(), cj.as_ptr(), cj.len(), cr.as_mut_ptr()) };
    if rc != ffi::TC_OK {
        return Err(Error::InvalidData("tc_batch_icp: bad arguments".to_string()));
    }
    cr.iter().enumerate().map(|(i, r)| {
        contexts[i % contexts.len()].check(r.status)?;
        Ok(BatchICPResult { transformation: iso_from7(&r.transformation), final_error: r.final_error, iterations: r.iterations as usize })
    }).collect()
}

/// `gpu_voxel_grid_filter(&ctx, &cloud, voxel_size)` (threecrate-gpu/src/filtering.rs:908-917) with the CPU filter's semantics
/// (centroid per occupied voxel, filtering.rs:38-133 -- not the wgpu shader's hash-bucket "first point wins")
pub fn gpu_voxel_grid_filter(ctx: &HipContext, cloud: &PointCloud<Point3f>, voxel_size: f32) -> Result<PointCloud<Point3f>> {
    voxel_grid_filter(ctx, cloud, voxel_size)
}

/// `GpuEuclideanClusterConfig` (threecrate-gpu/src/segmentation.rs:217-237): same fields and defaults.  `max_neighbors` is
/// validated (>= 1) and otherwise ignored: the search here is exact, no neighbour of a point is dropped.
#[derive(Debug, Clone)]
pub struct GpuEuclideanClusterConfig {
    pub tolerance: f32,
    pub min_cluster_size: usize,
    pub max_cluster_size: usize,
    pub max_neighbors: usize,
}

impl Default for GpuEuclideanClusterConfig {
    fn default() -> Self {
        Self { tolerance: 0.02, min_cluster_size: 100, max_cluster_size: 25_000, max_neighbors: 64 }
    }
}

/// `GpuClusterConfig` (threecrate-gpu/src/segmentation.rs:267)
pub type GpuClusterConfig = GpuEuclideanClusterConfig;

/// `GpuClusterExtractionResult` (threecrate-gpu/src/segmentation.rs:271-292)
#[derive(Debug, Clone)]
pub struct GpuClusterExtractionResult {
    pub clusters: Vec<Vec<usize>>,
}

impl GpuClusterExtractionResult {
    pub fn num_clusters(&self) -> usize {
        self.clusters.len()
    }

    pub fn get_cluster_cloud(&self, cloud: &PointCloud<Point3f>, index: usize) -> Option<PointCloud<Point3f>> {
        self.clusters.get(index).map(|indices| PointCloud::from_points(indices.iter().map(|&i| cloud.points[i]).collect()))
    }
}

/// `gpu_extract_euclidean_clusters(&ctx, &cloud, &config)` (threecrate-gpu/src/segmentation.rs:843-851, checks :885-913)
pub fn gpu_extract_euclidean_clusters(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: &GpuEuclideanClusterConfig) -> Result<GpuClusterExtractionResult> {
    if !cloud.points.is_empty() && config.tolerance > 0.0 && config.min_cluster_size != 0 && config.min_cluster_size <= config.max_cluster_size
        && config.max_neighbors == 0 {
        return Err(Error::InvalidData("max_neighbors must be at least 1".to_string()));
    }
    let clusters = cluster_indices(ctx, cloud, config.tolerance, config.min_cluster_size, config.max_cluster_size)?;
    Ok(GpuClusterExtractionResult { clusters })
}

/// `gpu_extract_clusters(&ctx, &cloud, config)` (threecrate-gpu/src/segmentation.rs:834-841): one cloud per cluster, largest first
pub fn gpu_extract_clusters(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: GpuClusterConfig) -> Result<Vec<PointCloud<Point3f>>> {
    let r = gpu_extract_euclidean_clusters(ctx, cloud, &config)?;
    Ok(r.clusters.iter().map(|idx| PointCloud::from_points(idx.iter().map(|&i| cloud.points[i]).collect())).collect())
}

/// `FPFH_DIM` (threecrate-algorithms/src/features.rs:15): 3 sub-histograms x 11 bins
pub const FPFH_DIM: usize = 33;

/// `FpfhConfig` (threecrate-algorithms/src/features.rs:18-33): same fields and defaults
#[derive(Debug, Clone)]
pub struct FpfhConfig {
    pub search_radius: f32,
    pub k_neighbors: usize,
}

impl Default for FpfhConfig {
    fn default() -> Self {
        Self { search_radius: 0.1, k_neighbors: 10 }
    }
}

/// `extract_fpfh_features_with_normals` (features.rs:173-259): one descriptor per point, in input order.  Points with a non-finite
/// coordinate get an all-zero descriptor and are nobody's neighbour (the kd-tree's result for them is arbitrary).
pub fn extract_fpfh_features_with_normals(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>, config: &FpfhConfig) -> Result<Vec<[f32; FPFH_DIM]>> {
    let n = cloud.points.len();
    let mut out = vec![[0.0f32; FPFH_DIM]; n];
    ctx.check(unsafe {
        ffi::tc_extract_fpfh_features_with_normals(ctx.0, cloud.points.as_ptr() as *const f32, n, config.search_radius, config.k_neighbors,
                                                   out.as_mut_ptr() as *mut f32)
    })?;
    Ok(out)
}

/// `extract_fpfh_features` (features.rs:268-285): normals from the 10 nearest neighbours, then the default `FpfhConfig`
pub fn extract_fpfh_features(ctx: &HipContext, cloud: &PointCloud<Point3f>) -> Result<Vec<Vec<f32>>> {
    let n = cloud.points.len();
    if n == 0 {
        return Ok(Vec::new());
    }
    if n < 3 {
        return Err(Error::InvalidData("At least 3 points are required to estimate normals for FPFH".to_string()));
    }
    let config = FpfhConfig::default();
    let mut out = vec![0.0f32; n * FPFH_DIM];
    ctx.check(unsafe { ffi::tc_extract_fpfh_features(ctx.0, xyz(cloud), n, config.search_radius, 10, out.as_mut_ptr()) })?;
    Ok(out.chunks(FPFH_DIM).map(|c| c.to_vec()).collect())
}

/// `gpu_find_k_nearest(&ctx, points, &query, k)` (threecrate-gpu/src/nearest_neighbor.rs:332-342)
pub fn gpu_find_k_nearest(ctx: &HipContext, points: &[Point3f], query: &Point3f, k: usize) -> Result<Vec<(usize, f32)>> {
    Ok(find_k_nearest_batch(ctx, points, std::slice::from_ref(query), k)?.into_iter().next().unwrap_or_default())
}

/// `gpu_find_k_nearest_batch(&ctx, points, query_points, k)` (threecrate-gpu/src/nearest_neighbor.rs:345-355)
pub fn gpu_find_k_nearest_batch(ctx: &HipContext, points: &[Point3f], query_points: &[Point3f], k: usize) -> Result<Vec<Vec<(usize, f32)>>> {
    find_k_nearest_batch(ctx, points, query_points, k)
}

/// `gpu_find_radius_neighbors(&ctx, points, &query, radius)` (threecrate-gpu/src/nearest_neighbor.rs:358-367): the reference asks
/// its kernel for the 32 nearest and keeps those within `radius`; same rule here (tc_radius_search with k_max = 32), nearest first.
pub fn gpu_find_radius_neighbors(ctx: &HipContext, points: &[Point3f], query: &Point3f, radius: f32) -> Result<Vec<(usize, f32)>> {
    const K_MAX: usize = 32;
    let (mut idx, mut dist, mut cnt) = (vec![0u32; K_MAX], vec![0f32; K_MAX], [0u32; 1]);
    ctx.check(unsafe {
        ffi::tc_radius_search(ctx.0, points.as_ptr() as *const f32, points.len(), query as *const Point3f as *const f32, 1, radius, K_MAX,
                              idx.as_mut_ptr(), dist.as_mut_ptr(), cnt.as_mut_ptr())
    })?;
    Ok((0..cnt[0] as usize).map(|j| (idx[j] as usize, dist[j])).collect())
}


// ---- device-resident cloud handles (include/threecrate_hip.h "tc_cloud": SURVEY.md 8b) ---------------------------------

/// A cloud that lives in HBM, is indexed once and keeps its normals in the layout the ICP kernels read.
/// `let prev = HipCloud::upload(&ctx, &frame0)?; prev.estimate_normals(16)?; let cur = HipCloud::upload(&ctx, &frame1)?;
///  let r = cur.icp_point_to_plane(&prev, Isometry3::identity(), 50, None, 1e-6)?;`
pub struct HipCloud<'a> { raw: *mut ffi::tc_cloud, ctx: &'a HipContext }

impl<'a> HipCloud<'a> {
    pub fn upload(ctx: &'a HipContext, cloud: &PointCloud<Point3f>) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        ctx.check(unsafe { ffi::tc_cloud_upload(ctx.0, xyz(cloud), cloud.points.len(), &mut raw) })?;
        Ok(HipCloud { raw, ctx })
    }
    pub fn len(&self) -> usize { unsafe { ffi::tc_cloud_size(self.raw) } }
    pub fn is_empty(&self) -> bool { self.len() == 0 }
    /// `estimate_normals` (normals.rs:238-241); the normals stay with the handle, nothing is copied back
    pub fn estimate_normals(&self, k: usize) -> Result<()> {
        let mut cfg = unsafe { std::mem::zeroed::<ffi::tc_normal_config>() };
        unsafe { ffi::tc_normal_config_default(&mut cfg) };
        cfg.k_neighbors = k as u64;
        self.ctx.check(unsafe { ffi::tc_cloud_estimate_normals(self.raw, &cfg, std::ptr::null_mut()) })
    }
    /// `icp_point_to_plane_detailed` (registration.rs:508-516) with `self` as the source and the target handle's normals
    pub fn icp_point_to_plane(&self, target: &HipCloud, init: Isometry3<f32>, max_iters: usize, max_correspondence_distance: Option<f32>,
                              convergence_threshold: f32) -> Result<ICPResult> {
        let mut none = Vec::new();
        let mut r = empty_result(&mut none);
        r.corr_target = std::ptr::null_mut();            // (device memory when wanted: see the header)
        let i7 = iso_to7(&init);
        self.ctx.check(unsafe {
            ffi::tc_cloud_icp_point_to_plane(self.raw, target.raw, i7.as_ptr(), max_iters,
                                             encode_max_dist(max_correspondence_distance, self.len(), target.len(), max_iters, None)?,
                                             convergence_threshold, &mut r)
        })?;
        Ok(result_from(&r, &[], 0))
    }
}

impl Drop for HipCloud<'_> {
    fn drop(&mut self) { unsafe { ffi::tc_cloud_destroy(self.raw) } }
}

// ---- one registration over the GPUs of a node: one process or thread per GPU ------------------------------

/// RCCL communicator of this rank, bound to the context's stream.  Rank 0 calls `HipComm::unique_id()`, the host distributes the
/// 128 bytes (pipe, file, MPI ...), every rank calls `HipComm::create`.
pub struct HipComm<'a> { raw: *mut ffi::tc_comm, ctx: &'a HipContext }

impl<'a> HipComm<'a> {
    pub fn unique_id() -> Result<[u8; ffi::TC_COMM_ID_BYTES]> {
        let mut id = [0u8; ffi::TC_COMM_ID_BYTES];
        match unsafe { ffi::tc_comm_unique_id(id.as_mut_ptr()) } {
            ffi::TC_OK => Ok(id),
            _ => Err(Error::Unsupported("RCCL is not available to libthreecrate_hip".to_string())),
        }
    }
    pub fn create(ctx: &'a HipContext, nranks: i32, rank: i32, id: &[u8; ffi::TC_COMM_ID_BYTES]) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        ctx.check(unsafe { ffi::tc_comm_create(ctx.0, nranks, rank, id.as_ptr(), &mut raw) })?;
        Ok(HipComm { raw, ctx })
    }
    pub fn rank(&self) -> i32 { unsafe { ffi::tc_comm_rank(self.raw) } }
    pub fn size(&self) -> i32 { unsafe { ffi::tc_comm_size(self.raw) } }

    /// `icp_point_to_plane_detailed` of ONE cloud pair over all ranks: every rank passes the same device-resident clouds
    /// (pointers to n x 3 floats in HBM), the library takes this rank's index range of the source (TC_SHARD_INDEX: each rank
    /// orders n / W points by target cell) and runs one ncclAllReduce of the packed 6x6 system per iteration on the compute
    /// stream.  Every rank returns the same result.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn icp_point_to_plane_device(&self, d_source: *const f32, n_source: usize, d_target: *const f32, n_target: usize,
                                            d_target_normals: *const f32, normal_stride: usize, init: Isometry3<f32>, max_iters: usize,
                                            max_correspondence_distance: Option<f32>, convergence_threshold: f32) -> Result<ICPResult> {
        let mut none = Vec::new();
        let mut r = empty_result(&mut none);
        r.corr_target = std::ptr::null_mut();
        let i7 = iso_to7(&init);
        self.ctx.check(ffi::tc_sharded_icp_point_to_plane_device(self.ctx.0, self.raw, ffi::TC_SHARD_INDEX, d_source, n_source, d_target,
                                                                  n_target, d_target_normals, n_target, normal_stride, i7.as_ptr(), max_iters,
                                                                  encode_max_dist(max_correspondence_distance, n_source, n_target, max_iters, None)?,
                                                                  convergence_threshold, &mut r))?;
        Ok(result_from(&r, &[], 0))
    }
}

impl Drop for HipComm<'_> {
    fn drop(&mut self) { unsafe { ffi::tc_comm_destroy(self.raw) } }
}

/// `NdtConfig` (threecrate-algorithms/src/ndt_registration.rs:15-38): same fields and defaults
#[derive(Debug, Clone)]
pub struct NdtConfig {
    pub resolution: f32,
    pub step_size: f32,
    pub max_iterations: usize,
    pub epsilon: f32,
    pub min_points_per_voxel: usize,
}

impl Default for NdtConfig {
    fn default() -> Self {
        Self { resolution: 1.0, step_size: 0.1, max_iterations: 35, epsilon: 1e-4, min_points_per_voxel: 5 }
    }
}

/// `NdtResult` (ndt_registration.rs:42-51); `score` belongs to the last pose that was evaluated
#[derive(Debug, Clone)]
pub struct NdtResult {
    pub transformation: Isometry3<f32>,
    pub score: f32,
    pub iterations: usize,
    pub converged: bool,
}

/// `ndt_registration(&source, &target, initial_transform, &config)` (ndt_registration.rs:188-260).  Deviations from the reference
/// are listed in include/threecrate_hip_ndt.h (non-finite points, the resolution check, f64 sums).
pub fn ndt_registration(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, initial_transform: Isometry3<f32>,
                        config: &NdtConfig) -> Result<NdtResult> {
    let i7 = iso_to7(&initial_transform);
    let cfg = ffi_ndt::tc_ndt_config {
        resolution: config.resolution,
        step_size: config.step_size,
        max_iterations: config.max_iterations,
        epsilon: config.epsilon,
        min_points_per_voxel: config.min_points_per_voxel,
    };
    let mut r = ffi_ndt::tc_ndt_result { transformation: [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0], score: 0.0, iterations: 0, converged: 0, n_voxels: 0, n_hits: 0 };
    ctx.check(unsafe {
        ffi_ndt::tc_ndt_registration(ctx.0, xyz(source), source.points.len(), xyz(target), target.points.len(), i7.as_ptr(), &cfg, &mut r)
    })?;
    Ok(NdtResult { transformation: iso_from7(&r.transformation), score: r.score, iterations: r.iterations, converged: r.converged != 0 })
}

/// `ndt_registration_default` (ndt_registration.rs:263-269)
pub fn ndt_registration_default(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>,
                                initial_transform: Isometry3<f32>) -> Result<NdtResult> {
    ndt_registration(ctx, source, target, initial_transform, &NdtConfig::default())
}

// ---- TSDF volumes (include/threecrate_hip_tsdf.h) ------------------------------------------------------------------------------
/// `TsdfVoxel` (threecrate-gpu/src/tsdf.rs:11-20) without its padding
#[derive(Debug, Clone, Copy)]
pub struct TsdfVoxel {
    pub tsdf_value: f32,
    pub weight: f32,
    pub color_r: u32,
    pub color_g: u32,
    pub color_b: u32,
}

/// `TsdfVolume` (tsdf.rs:24-29)
#[derive(Debug, Clone)]
pub struct TsdfVolume {
    pub voxel_size: f32,
    pub truncation_distance: f32,
    pub resolution: [u32; 3],
    pub origin: Point3<f32>,
}

/// `CameraIntrinsics` (tsdf.rs:41-50).  `depth_scale` is kept for the reference's call shape and, as in its shader, never read.
#[derive(Debug, Clone, Copy)]
pub struct CameraIntrinsics {
    pub fx: f32,
    pub fy: f32,
    pub cx: f32,
    pub cy: f32,
    pub width: u32,
    pub height: u32,
    pub depth_scale: f32,
}

/// `TsdfVolumeGpu` (tsdf.rs:32-37, :549-803): the volume lives in device memory; integrate updates it in place, extract_surface
/// reads it in place.  Deviations from the reference's shaders are listed in include/threecrate_hip_tsdf.h.
/// The library's handle keeps a pointer to its context: the borrow `'a` keeps the `HipContext` alive until the volume is dropped.
pub struct TsdfVolumeGpu<'a> {
    pub volume: TsdfVolume,
    handle: *mut ffi_tsdf::tc_tsdf_volume,
    _context: std::marker::PhantomData<&'a HipContext>,
}

impl<'a> TsdfVolumeGpu<'a> {
    /// `TsdfVolumeGpu::new(gpu, volume_params)`; the weight's cap is the reference's 100
    pub fn new(gpu: &'a HipContext, volume_params: TsdfVolume) -> Result<Self> {
        let cfg = ffi_tsdf::tc_tsdf_volume_config {
            voxel_size: volume_params.voxel_size, truncation_distance: volume_params.truncation_distance, resolution: volume_params.resolution,
            origin: [volume_params.origin.x, volume_params.origin.y, volume_params.origin.z], max_weight: 100,
        };
        let mut h: *mut ffi_tsdf::tc_tsdf_volume = std::ptr::null_mut();
        gpu.check(unsafe { ffi_tsdf::tc_tsdf_volume_create(gpu.0, &cfg, &mut h) })?;
        Ok(TsdfVolumeGpu { volume: volume_params, handle: h, _context: std::marker::PhantomData })
    }

    fn voxel_count(&self) -> usize {
        self.volume.resolution.iter().map(|&r| r as usize).product()
    }

    /// `integrate(gpu, depth_image, color_image, camera_pose, intrinsics)`: `camera_pose` is camera-to-world and inverted here
    pub fn integrate(&self, gpu: &HipContext, depth_image: &[f32], color_image: Option<&[u8]>, camera_pose: &Matrix4<f32>,
                     intrinsics: &CameraIntrinsics) -> Result<()> {
        let pixels = intrinsics.width as usize * intrinsics.height as usize;
        if depth_image.len() != pixels || color_image.map_or(false, |c| c.len() != 3 * pixels) {
            return Err(Error::InvalidData("the images do not have the size the intrinsics state".into()));
        }
        let inv = camera_pose.cast::<f64>().try_inverse().ok_or_else(|| Error::Gpu("Failed to invert camera pose matrix".into()))?;
        let mut m = [0f32; 12];
        for r in 0..3 {
            for c in 0..4 {
                m[4 * r + c] = inv[(r, c)] as f32;
            }
        }
        let k = ffi_tsdf::tc_camera_intrinsics { fx: intrinsics.fx, fy: intrinsics.fy, cx: intrinsics.cx, cy: intrinsics.cy, width: intrinsics.width,
                                                 height: intrinsics.height };
        let rgb = color_image.map_or(std::ptr::null(), |c| c.as_ptr());
        gpu.check(unsafe { ffi_tsdf::tc_tsdf_integrate(self.handle, depth_image.as_ptr(), rgb, &k, m.as_ptr(), std::ptr::null_mut()) })
    }

    /// `download_voxels(gpu)`
    pub fn download_voxels(&self, gpu: &HipContext) -> Result<Vec<TsdfVoxel>> {
        let n = self.voxel_count();
        let (mut tsdf, mut weight, mut rgb) = (vec![0f32; n], vec![0u8; n], vec![0u8; 3 * n]);
        gpu.check(unsafe { ffi_tsdf::tc_tsdf_volume_download(self.handle, tsdf.as_mut_ptr(), weight.as_mut_ptr(), rgb.as_mut_ptr()) })?;
        Ok((0..n).map(|i| TsdfVoxel { tsdf_value: tsdf[i], weight: weight[i] as f32, color_r: rgb[3 * i] as u32, color_g: rgb[3 * i + 1] as u32,
                                      color_b: rgb[3 * i + 2] as u32 }).collect())
    }

    fn upload_voxels(&self, gpu: &HipContext, voxels: &[TsdfVoxel]) -> Result<()> {
        if voxels.len() != self.voxel_count() {
            return Err(Error::InvalidData("the voxel list does not have the volume's size".into()));
        }
        let tsdf: Vec<f32> = voxels.iter().map(|v| v.tsdf_value).collect();
        let weight: Vec<u8> = voxels.iter().map(|v| v.weight.max(0.0).min(255.0) as u8).collect();
        let rgb: Vec<u8> = voxels.iter().flat_map(|v| [v.color_r.min(255) as u8, v.color_g.min(255) as u8, v.color_b.min(255) as u8]).collect();
        gpu.check(unsafe { ffi_tsdf::tc_tsdf_volume_upload(self.handle, tsdf.as_ptr(), weight.as_ptr(), rgb.as_ptr()) })
    }

    /// `extract_surface(gpu, iso_value)`: the shader's rule (flags 0); the count call, then the points
    pub fn extract_surface(&self, gpu: &HipContext, iso_value: f32) -> Result<PointCloud<ColoredPoint3f>> {
        let mut n = 0usize;
        gpu.check(unsafe { ffi_tsdf::tc_tsdf_extract_surface(self.handle, iso_value, 0, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut n) })?;
        let (mut xyz, mut rgb) = (vec![0f32; 3 * n], vec![0u8; 3 * n]);
        if n > 0 {
            gpu.check(unsafe { ffi_tsdf::tc_tsdf_extract_surface(self.handle, iso_value, 0, xyz.as_mut_ptr(), rgb.as_mut_ptr(), n, &mut n) })?;
        }
        let points = (0..n).map(|i| ColoredPoint3f { position: Point3::new(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]),
                                                     color: [rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]] }).collect();
        Ok(PointCloud::from_points(points))
    }
}

impl<'a> Drop for TsdfVolumeGpu<'a> {
    fn drop(&mut self) {
        unsafe { ffi_tsdf::tc_tsdf_volume_destroy(self.handle) }
    }
}

/// `create_tsdf_volume` (tsdf.rs:806-818)
pub fn create_tsdf_volume(voxel_size: f32, truncation_distance: f32, resolution: [u32; 3], origin: Point3<f32>) -> TsdfVolume {
    TsdfVolume { voxel_size, truncation_distance, resolution, origin }
}

/// `gpu_tsdf_integrate` (tsdf.rs:821-832): a volume in its initial state, one frame fused, its voxels -- the reference's call shape,
/// which carries the whole volume through the host; keep a `TsdfVolumeGpu` to fuse many frames
pub fn gpu_tsdf_integrate(gpu_context: &HipContext, volume: &mut TsdfVolume, depth_image: &[f32], color_image: Option<&[u8]>,
                          camera_pose: &Matrix4<f32>, intrinsics: &CameraIntrinsics) -> Result<Vec<TsdfVoxel>> {
    let v = TsdfVolumeGpu::new(gpu_context, volume.clone())?;
    v.integrate(gpu_context, depth_image, color_image, camera_pose, intrinsics)?;
    v.download_voxels(gpu_context)
}

/// `gpu_tsdf_extract_surface` (tsdf.rs:835-844)
pub fn gpu_tsdf_extract_surface(gpu_context: &HipContext, volume: &TsdfVolume, voxels: &[TsdfVoxel], iso_value: f32)
                                -> Result<PointCloud<ColoredPoint3f>> {
    let v = TsdfVolumeGpu::new(gpu_context, volume.clone())?;
    v.upload_voxels(gpu_context, voxels)?;
    v.extract_surface(gpu_context, iso_value)
}

// ---- global registration (threecrate-algorithms/src/global_registration.rs; include/threecrate_hip_global.h) ----

/// `GlobalRegistrationConfig` (global_registration.rs:27-62), the same fields and defaults
#[derive(Debug, Clone)]
pub struct GlobalRegistrationConfig {
    pub ransac_iterations: usize,
    pub distance_threshold: f32,
    pub inlier_ratio: f32,
    pub fpfh_radius: f32,
    pub fpfh_k_neighbors: usize,
    pub normal_k_neighbors: usize,
    pub refine_with_icp: bool,
    pub icp_max_iterations: usize,
    pub icp_distance_threshold: Option<f32>,
}

impl Default for GlobalRegistrationConfig {
    fn default() -> Self {
        Self { ransac_iterations: 50_000, distance_threshold: 0.05, inlier_ratio: 0.25, fpfh_radius: 0.25, fpfh_k_neighbors: 10,
               normal_k_neighbors: 10, refine_with_icp: true, icp_max_iterations: 50, icp_distance_threshold: None }
    }
}

/// `GlobalRegistrationResult` (global_registration.rs:70-79)
#[derive(Debug, Clone)]
pub struct GlobalRegistrationResult {
    pub transformation: Isometry3<f32>,
    pub inlier_count: usize,
    pub inlier_ratio: f32,
    pub icp_result: Option<ICPResult>,
}

/// `find_feature_correspondences` (global_registration.rs:94-110): the nearest target descriptor of every source descriptor, the lowest
/// index among equal distances
pub fn match_features(ctx: &HipContext, src: &[[f32; FPFH_DIM]], tgt: &[[f32; FPFH_DIM]]) -> Result<Vec<u32>> {
    let mut index = vec![0u32; src.len()];
    ctx.check(unsafe {
        ffi_global::tc_match_features(ctx.0, src.as_ptr() as *const f32, src.len(), tgt.as_ptr() as *const f32, tgt.len(), FPFH_DIM,
                                      index.as_mut_ptr(), std::ptr::null_mut())
    })?;
    Ok(index)
}

/// The RANSAC loop of global_registration.rs:252-299 over the pairs (source[corr_src[p]], target[corr_tgt[p]]), samples from the seeded
/// generator: the winner's stored matrix (R row-major, t) and the loop's record
pub fn ransac_correspondences(ctx: &HipContext, source: &[Point3f], target: &[Point3f], corr_src: &[u32], corr_tgt: &[u32], threshold: f32,
                              inlier_ratio: f32, max_iters: usize, seed: u64) -> Result<([f32; 12], ffi_global::tc_ransac_result)> {
    let mut transform = [0f32; 12];
    let mut res = ffi_global::tc_ransac_result::default();
    ctx.check(unsafe {
        ffi_global::tc_ransac_correspondences(ctx.0, source.as_ptr() as *const f32, source.len(), target.as_ptr() as *const f32, target.len(),
                                              corr_src.as_ptr(), corr_tgt.as_ptr(), corr_src.len().min(corr_tgt.len()), threshold, inlier_ratio,
                                              max_iters, seed, transform.as_mut_ptr(), &mut res, std::ptr::null_mut(), std::ptr::null_mut())
    })?;
    Ok((transform, res))
}

/// `global_registration` (global_registration.rs:185-201): normals of both clouds, then `global_registration_with_normals`
pub fn global_registration(ctx: &HipContext, source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, config: &GlobalRegistrationConfig)
                           -> Result<GlobalRegistrationResult> {
    if source.points.is_empty() {
        return Err(Error::Algorithm("Source point cloud is empty".into()));
    }
    if target.points.is_empty() {
        return Err(Error::Algorithm("Target point cloud is empty".into()));
    }
    let src_normals = estimate_normals(ctx, source, config.normal_k_neighbors)?;
    let tgt_normals = estimate_normals(ctx, target, config.normal_k_neighbors)?;
    global_registration_with_normals(ctx, &src_normals, &tgt_normals, source, target, config)
}

/// `global_registration_with_normals` (global_registration.rs:213-333), composed of the same five public steps as the Python facade:
/// FPFH of both clouds, matching, RANSAC (seed 0), and with `refine_with_icp` point-to-point ICP from RANSAC's pose
pub fn global_registration_with_normals(ctx: &HipContext, source_n: &PointCloud<NormalPoint3f>, target_n: &PointCloud<NormalPoint3f>,
                                        source: &PointCloud<Point3f>, target: &PointCloud<Point3f>, config: &GlobalRegistrationConfig)
                                        -> Result<GlobalRegistrationResult> {
    if source_n.points.is_empty() || target_n.points.is_empty() {
        return Err(Error::Algorithm("Source or target cloud is empty".into()));
    }
    let fpfh_cfg = FpfhConfig { search_radius: config.fpfh_radius, k_neighbors: config.fpfh_k_neighbors };
    let src_descs = extract_fpfh_features_with_normals(ctx, source_n, &fpfh_cfg)?;
    let tgt_descs = extract_fpfh_features_with_normals(ctx, target_n, &fpfh_cfg)?;
    let matched = match_features(ctx, &src_descs, &tgt_descs)?;
    if matched.len() < 3 {
        return Err(Error::Algorithm("Too few feature correspondences for RANSAC (need ≥ 3)".into()));
    }
    let src_pts: Vec<Point3f> = source_n.points.iter().map(|p| p.position).collect();
    let tgt_pts: Vec<Point3f> = target_n.points.iter().map(|p| p.position).collect();
    let corr_src: Vec<u32> = (0..matched.len() as u32).collect();
    let (t12, res) = ransac_correspondences(ctx, &src_pts, &tgt_pts, &corr_src, &matched, config.distance_threshold, config.inlier_ratio,
                                            config.ransac_iterations, 0)?;
    let r = nalgebra::Matrix3::new(t12[0] as f64, t12[1] as f64, t12[2] as f64, t12[3] as f64, t12[4] as f64, t12[5] as f64, t12[6] as f64,
                                   t12[7] as f64, t12[8] as f64);
    let q = nalgebra::UnitQuaternion::from_rotation_matrix(&nalgebra::Rotation3::from_matrix_unchecked(r));     // on the host, in f64
    let best = Isometry3::from_parts(Translation3::new(t12[9], t12[10], t12[11]), q.cast::<f32>());
    let icp_result = if config.refine_with_icp {
        Some(icp_point_to_point(ctx, source, target, best, config.icp_max_iterations, 1e-6, config.icp_distance_threshold)?)
    } else {
        None
    };
    let transformation = icp_result.as_ref().map(|r| r.transformation).unwrap_or(best);
    Ok(GlobalRegistrationResult { transformation, inlier_count: res.inlier_count as usize, inlier_ratio: res.inlier_ratio, icp_result })
}

/// `StreamingVoxelFilterConfig` (threecrate-algorithms/src/streaming.rs:196-201)
#[derive(Debug, Clone)]
pub struct StreamingVoxelFilterConfig {
    pub voxel_size: f32,
}

/// `StreamingVoxelFilter` (streaming.rs:216-285) on a voxel map that lives in device memory (include/threecrate_hip_voxelmap.h, which
/// pins keys, sums and centroids bit for bit).  `finalize` returns the centroids in ascending (kx, ky, kz) order, where the reference's
/// order is its HashMap's.  Keys beyond +-2^20 per axis are `Error::Unsupported`.
/// The library's handle keeps a pointer to its context: the borrow `'a` keeps the `HipContext` alive until the filter is dropped.
pub struct StreamingVoxelFilter<'a> {
    config: StreamingVoxelFilterConfig,
    gpu: &'a HipContext,
    handle: *mut ffi_voxelmap::tc_voxel_map,        // made by the first chunk: `new` accepts any voxel_size, as the reference's does
}

impl<'a> StreamingVoxelFilter<'a> {
    /// `StreamingVoxelFilter::new(config)`
    pub fn new(gpu: &'a HipContext, config: StreamingVoxelFilterConfig) -> Self {
        StreamingVoxelFilter { config, gpu, handle: std::ptr::null_mut() }
    }

    /// `voxel_count()`
    pub fn voxel_count(&self) -> usize {
        if self.handle.is_null() { 0 } else { unsafe { ffi_voxelmap::tc_voxel_map_size(self.handle) } }
    }

    /// `StreamingPipeline::process_chunk` (:250-263)
    pub fn process_chunk(&mut self, chunk: &[Point3f]) -> Result<()> {
        if !(self.config.voxel_size > 0.0) {
            return Err(Error::InvalidData("voxel_size must be positive".into()));
        }
        if self.handle.is_null() {
            let cfg = ffi_voxelmap::tc_voxel_map_config { voxel_size: self.config.voxel_size, initial_capacity: 0 };
            self.gpu.check(unsafe { ffi_voxelmap::tc_voxel_map_create(self.gpu.0, &cfg, &mut self.handle) })?;
        }
        self.gpu.check(unsafe { ffi_voxelmap::tc_voxel_map_insert(self.handle, chunk.as_ptr() as *const f32, chunk.len()) })
    }

    /// `StreamingPipeline::finalize` (:265-279): the count call, then the centroids
    pub fn finalize(self) -> Result<PointCloud<Point3f>> {
        if self.handle.is_null() {
            return Ok(PointCloud::from_points(Vec::new()));
        }
        let mut n = 0usize;
        let null = std::ptr::null_mut;
        self.gpu.check(unsafe { ffi_voxelmap::tc_voxel_map_extract(self.handle, null(), null(), null(), null(), 0, &mut n) })?;
        let mut xyz = vec![0f32; 3 * n];
        if n > 0 {
            self.gpu.check(unsafe { ffi_voxelmap::tc_voxel_map_extract(self.handle, null(), null(), null(), xyz.as_mut_ptr(), n, &mut n) })?;
        }
        Ok(PointCloud::from_points((0..n).map(|i| Point3f::new(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])).collect()))
    }
}

impl<'a> Drop for StreamingVoxelFilter<'a> {
    fn drop(&mut self) {
        unsafe { ffi_voxelmap::tc_voxel_map_destroy(self.handle) }
    }
}

/// The colorization module of the reference (threecrate-algorithms/src/colorization.rs) under its own names -- its `CameraIntrinsics`
/// (fx fy cx cy) is not the TSDF one above, hence the module -- served by include/threecrate_hip_color.h, which pins every operation bit
/// for bit and lists the deviations: points and projections that are not finite are skipped, and the pose enters as its 3 x 4 matrix.
pub mod colorization {
    use crate::{ffi_color, ffi_tsdf, HipContext};
    use nalgebra::Isometry3;
    use threecrate_core::{ColoredPoint3f, Error, Point3f, PointCloud, Result};

    /// `CameraIntrinsics` (colorization.rs:35-45)
    #[derive(Debug, Clone, Copy)]
    pub struct CameraIntrinsics {
        pub fx: f32,
        pub fy: f32,
        pub cx: f32,
        pub cy: f32,
    }

    /// `RgbImageView` (:48-76)
    #[derive(Debug, Clone, Copy)]
    pub struct RgbImageView<'a> {
        pub data: &'a [u8],
        pub width: u32,
        pub height: u32,
    }

    impl<'a> RgbImageView<'a> {
        /// `RgbImageView::new`, with its length check and message
        pub fn new(data: &'a [u8], width: u32, height: u32) -> Result<Self> {
            let expected = (width as usize) * (height as usize) * 3;
            if data.len() < expected {
                return Err(Error::InvalidData(format!("RgbImageView: buffer too small — expected {} bytes for {}×{} RGB image, got {}",
                                                      expected, width, height, data.len())));
            }
            Ok(Self { data, width, height })
        }
    }

    /// `InterpolationMode` (:133-140)
    #[derive(Debug, Clone, Copy, Default)]
    pub enum InterpolationMode {
        NearestNeighbor,
        #[default]
        Bilinear,
    }

    /// `ColorizationConfig` (:143-163)
    #[derive(Debug, Clone)]
    pub struct ColorizationConfig {
        pub default_color: [u8; 3],
        pub interpolation: InterpolationMode,
        pub min_depth: f32,
    }

    impl Default for ColorizationConfig {
        fn default() -> Self {
            Self { default_color: [128, 128, 128], interpolation: InterpolationMode::default(), min_depth: 1e-4 }
        }
    }

    /// `ColorizationResult` (:166-174)
    #[derive(Debug, Clone)]
    pub struct ColorizationResult {
        pub cloud: PointCloud<ColoredPoint3f>,
        pub colored_count: usize,
        pub uncolored_count: usize,
    }

    /// `colorize_point_cloud` (:217-249)
    pub fn colorize_point_cloud(ctx: &HipContext, cloud: &PointCloud<Point3f>, image: &RgbImageView<'_>, intrinsics: &CameraIntrinsics,
                                world_to_camera: &Isometry3<f32>, config: &ColorizationConfig) -> Result<ColorizationResult> {
        run(ctx, cloud, &[(*image, *intrinsics, *world_to_camera)], config)
    }

    /// `colorize_from_images` (:261-307): the first source that colours a point wins
    pub fn colorize_from_images(ctx: &HipContext, cloud: &PointCloud<Point3f>, sources: &[(RgbImageView<'_>, CameraIntrinsics, Isometry3<f32>)],
                                config: &ColorizationConfig) -> Result<ColorizationResult> {
        if sources.is_empty() {
            return Err(Error::InvalidData("colorize_from_images: sources slice must not be empty".into()));
        }
        run(ctx, cloud, sources, config)
    }

    fn run(ctx: &HipContext, cloud: &PointCloud<Point3f>, sources: &[(RgbImageView<'_>, CameraIntrinsics, Isometry3<f32>)],
           config: &ColorizationConfig) -> Result<ColorizationResult> {
        let table: Vec<ffi_color::tc_color_source> = sources.iter().map(|(image, k, pose)| {
            let h = pose.to_homogeneous();
            let mut m = [0f32; 12];
            for r in 0..3 {
                for c in 0..4 {
                    m[4 * r + c] = h[(r, c)];
                }
            }
            ffi_color::tc_color_source {
                rgb: image.data.as_ptr(), depth: std::ptr::null(),
                intrinsics: ffi_tsdf::tc_camera_intrinsics { fx: k.fx, fy: k.fy, cx: k.cx, cy: k.cy, width: image.width, height: image.height },
                world_to_camera: m,
            }
        }).collect();
        let mut cfg = ffi_color::tc_colorize_config { default_color: [0; 3], interpolation: 0, min_depth: 0.0, depth_tolerance: 0.0 };
        unsafe { ffi_color::tc_colorize_config_default(&mut cfg) };
        cfg.default_color = config.default_color;
        cfg.interpolation = match config.interpolation {
            InterpolationMode::NearestNeighbor => ffi_color::TC_COLOR_NEAREST,
            InterpolationMode::Bilinear => ffi_color::TC_COLOR_BILINEAR,
        };
        cfg.min_depth = config.min_depth;
        let n = cloud.points.len();
        let mut rgb = vec![0u8; 3 * n];
        let mut colored_count = 0usize;
        ctx.check(unsafe { ffi_color::tc_colorize(ctx.0, cloud.points.as_ptr() as *const f32, n, table.as_ptr(), table.len(), &cfg, rgb.as_mut_ptr(),
                                                  std::ptr::null_mut(), &mut colored_count) })?;
        let points = cloud.points.iter().enumerate()
            .map(|(i, p)| ColoredPoint3f { position: *p, color: [rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]] }).collect();
        Ok(ColorizationResult { cloud: PointCloud::from_points(points), colored_count, uncolored_count: n - colored_count })
    }
}

/// Mesh smoothing with the reference's names (threecrate-algorithms/src/mesh_smoothing.rs) over include/threecrate_hip_mesh.h.  The
/// summation order over a vertex's ring is ascending neighbour index (the reference's HashSet order is unspecified); a face index out of
/// range and a parameter that is not finite are `Error::InvalidData`.
pub mod mesh_smoothing {
    use crate::{ffi_mesh, HipContext};
    use threecrate_core::{Error, Point3f, Result, TriangleMesh};

    /// `LaplacianSmoothingConfig` (:65-81)
    #[derive(Debug, Clone)]
    pub struct LaplacianSmoothingConfig {
        pub iterations: usize,
        pub lambda: f32,
    }

    impl Default for LaplacianSmoothingConfig {
        fn default() -> Self {
            Self { iterations: 10, lambda: 0.5 }
        }
    }

    /// `TaubinSmoothingConfig` (:125-144)
    #[derive(Debug, Clone)]
    pub struct TaubinSmoothingConfig {
        pub iterations: usize,
        pub lambda: f32,
        pub mu: f32,
    }

    impl Default for TaubinSmoothingConfig {
        fn default() -> Self {
            Self { iterations: 10, lambda: 0.5, mu: -0.53 }
        }
    }

    /// `HcSmoothingConfig` (:189-210)
    #[derive(Debug, Clone)]
    pub struct HcSmoothingConfig {
        pub iterations: usize,
        pub alpha: f32,
        pub beta: f32,
    }

    impl Default for HcSmoothingConfig {
        fn default() -> Self {
            Self { iterations: 10, alpha: 0.0, beta: 0.5 }
        }
    }

    /// `smooth_laplacian` (:95-118)
    pub fn smooth_laplacian(ctx: &HipContext, mesh: &TriangleMesh, config: &LaplacianSmoothingConfig) -> Result<TriangleMesh> {
        run(ctx, mesh, ffi_mesh::TC_MESH_LAPLACIAN, config.iterations, |c| c.lambda = config.lambda)
    }

    /// `smooth_taubin` (:158-182)
    pub fn smooth_taubin(ctx: &HipContext, mesh: &TriangleMesh, config: &TaubinSmoothingConfig) -> Result<TriangleMesh> {
        run(ctx, mesh, ffi_mesh::TC_MESH_TAUBIN, config.iterations, |c| {
            c.lambda = config.lambda;
            c.mu = config.mu;
        })
    }

    /// `smooth_hc` (:225-286)
    pub fn smooth_hc(ctx: &HipContext, mesh: &TriangleMesh, config: &HcSmoothingConfig) -> Result<TriangleMesh> {
        run(ctx, mesh, ffi_mesh::TC_MESH_HC, config.iterations, |c| {
            c.alpha = config.alpha;
            c.beta = config.beta;
        })
    }

    fn run(ctx: &HipContext, mesh: &TriangleMesh, method: u32, iterations: usize, set: impl FnOnce(&mut ffi_mesh::tc_mesh_smooth_config)) -> Result<TriangleMesh> {
        let mut cfg = ffi_mesh::tc_mesh_smooth_config { method, iterations: 0, lambda: 0.0, mu: 0.0, alpha: 0.0, beta: 0.0 };
        unsafe { ffi_mesh::tc_mesh_smooth_config_default(method, &mut cfg) };
        cfg.iterations = u32::try_from(iterations).map_err(|_| Error::InvalidData("iterations does not fit 32 bits".into()))?;
        set(&mut cfg);
        let n = mesh.vertices.len();
        let mut faces = Vec::with_capacity(3 * mesh.faces.len());
        for face in &mesh.faces {
            for &v in face {
                // an index that does not fit 32 bits is out of range for every mesh the library takes
                faces.push(u32::try_from(v).unwrap_or(u32::MAX));
            }
        }
        let mut out = vec![Point3f::origin(); n];
        ctx.check(unsafe { ffi_mesh::tc_mesh_smooth(ctx.0, mesh.vertices.as_ptr() as *const f32, n, faces.as_ptr(), mesh.faces.len(), &cfg,
                                                    out.as_mut_ptr() as *mut f32) })?;
        Ok(TriangleMesh::from_vertices_and_faces(out, mesh.faces.clone()))
    }
}

/// Mesh simplification with the reference's names (threecrate-simplification/src/clustering.rs) over include/threecrate_hip_simplify.h:
/// the uniform road of `ClusteringSimplifier`.  The output vertex order is the cell order the header pins (the reference's comes out of a
/// HashMap); `ClusteringMode::Adaptive` and `RepresentativeStrategy::MinimumError` are `Error::Unsupported`; a face index out of range and
/// a coordinate that is not finite are `Error::InvalidData`.
pub mod simplification {
    use crate::{ffi_qem, ffi_simplify, HipContext};
    use threecrate_core::{Error, Point3f, Result, TriangleMesh, Vector3f};

    /// `RepresentativeStrategy` (:17-25)
    #[derive(Debug, Clone, Copy, PartialEq)]
    pub enum RepresentativeStrategy {
        Centroid,
        WeightedAverage,
        MinimumError,
    }

    /// `ClusteringMode` (:28-37)
    #[derive(Debug, Clone, Copy, PartialEq)]
    pub enum ClusteringMode {
        Uniform,
        Adaptive { max_depth: u32, error_threshold: f64 },
    }

    /// `MeshSimplifier` (lib.rs of the crate)
    pub trait MeshSimplifier {
        fn simplify(&self, ctx: &HipContext, mesh: &TriangleMesh, reduction_ratio: f32) -> Result<TriangleMesh>;
    }

    /// `ClusteringSimplifier` (:495-506)
    pub struct ClusteringSimplifier {
        pub mode: ClusteringMode,
        pub representative_strategy: RepresentativeStrategy,
        pub preserve_boundary: bool,
        pub feature_angle_threshold: f32,
    }

    impl Default for ClusteringSimplifier {
        fn default() -> Self {
            Self {
                mode: ClusteringMode::Uniform,
                representative_strategy: RepresentativeStrategy::Centroid,
                preserve_boundary: true,
                feature_angle_threshold: 45.0_f32.to_radians(),
            }
        }
    }

    impl ClusteringSimplifier {
        pub fn new() -> Self {
            Self::default()
        }

        pub fn with_params(mode: ClusteringMode, representative_strategy: RepresentativeStrategy, preserve_boundary: bool, feature_angle_threshold: f32) -> Self {
            Self { mode, representative_strategy, preserve_boundary, feature_angle_threshold }
        }
    }

    impl MeshSimplifier for ClusteringSimplifier {
        /// `simplify` (:785-829)
        fn simplify(&self, ctx: &HipContext, mesh: &TriangleMesh, reduction_ratio: f32) -> Result<TriangleMesh> {
            if self.mode != ClusteringMode::Uniform {
                return Err(Error::Unsupported("adaptive clustering depends on a sequential insertion order".into()));
            }
            let strategy = match self.representative_strategy {
                RepresentativeStrategy::Centroid => ffi_simplify::TC_SIMPLIFY_CENTROID,
                RepresentativeStrategy::WeightedAverage => ffi_simplify::TC_SIMPLIFY_WEIGHTED_AVERAGE,
                RepresentativeStrategy::MinimumError => return Err(Error::Unsupported("the minimum-error representative is not pinned".into())),
            };
            let mut cfg = ffi_simplify::tc_simplify_config { strategy: 0, preserve_boundary: 0, feature_angle_threshold: 0.0, reduction_ratio: 0.0 };
            unsafe { ffi_simplify::tc_simplify_config_default(reduction_ratio, &mut cfg) };
            cfg.strategy = strategy;
            cfg.preserve_boundary = self.preserve_boundary as u32;
            cfg.feature_angle_threshold = self.feature_angle_threshold;
            let (n, m) = (mesh.vertices.len(), mesh.faces.len());
            let mut faces = Vec::with_capacity(3 * m);
            for face in &mesh.faces {
                for &v in face {
                    // an index that does not fit 32 bits is out of range for every mesh the library takes
                    faces.push(u32::try_from(v).unwrap_or(u32::MAX));
                }
            }
            // the input's sizes bound the output's: one call
            let mut out_v = vec![Point3f::origin(); n];
            let mut out_f = vec![0u32; 3 * m];
            let mut out_n = mesh.normals.as_ref().map(|_| vec![Vector3f::zeros(); n]);
            let mut out_c = mesh.colors.as_ref().map(|_| vec![[0u8; 3]; n]);
            let (mut nv, mut nf) = (0usize, 0usize);
            ctx.check(unsafe {
                ffi_simplify::tc_simplify_clustering(
                    ctx.0, mesh.vertices.as_ptr() as *const f32, n, faces.as_ptr(), m,
                    mesh.normals.as_ref().map_or(std::ptr::null(), |v| v.as_ptr() as *const f32),
                    mesh.colors.as_ref().map_or(std::ptr::null(), |v| v.as_ptr() as *const u8), &cfg, out_v.as_mut_ptr() as *mut f32,
                    out_n.as_mut().map_or(std::ptr::null_mut(), |v| v.as_mut_ptr() as *mut f32),
                    out_c.as_mut().map_or(std::ptr::null_mut(), |v| v.as_mut_ptr() as *mut u8), n, out_f.as_mut_ptr(), m, std::ptr::null_mut(),
                    &mut nv, &mut nf)
            })?;
            out_v.truncate(nv);
            let new_faces = (0..nf).map(|f| [out_f[3 * f] as usize, out_f[3 * f + 1] as usize, out_f[3 * f + 2] as usize]).collect();
            let mut result = TriangleMesh::from_vertices_and_faces(out_v, new_faces);
            if let Some(mut normals) = out_n {
                normals.truncate(nv);
                result.set_normals(normals);
            }
            if let Some(mut colors) = out_c {
                colors.truncate(nv);
                result.set_colors(colors);
            }
            Ok(result)
        }
    }

    /// `QuadricErrorSimplifier` (threecrate-simplification/src/quadric_error.rs:66-100) over include/threecrate_hip_qem.h: edge collapse
    /// in rounds, compared with the reference for quality, not identity.  `feature_angle_threshold` is kept and ignored: the reference
    /// never reads it either.  No normals or colours come back, as from the reference's rebuild_mesh.
    pub struct QuadricErrorSimplifier {
        pub max_edge_length: Option<f32>,
        pub preserve_boundary: bool,
        pub feature_angle_threshold: f32,
    }

    impl Default for QuadricErrorSimplifier {
        fn default() -> Self {
            Self { max_edge_length: None, preserve_boundary: true, feature_angle_threshold: 45.0_f32.to_radians() }
        }
    }

    impl QuadricErrorSimplifier {
        pub fn new() -> Self {
            Self::default()
        }

        pub fn with_params(max_edge_length: Option<f32>, preserve_boundary: bool, feature_angle_threshold: f32) -> Self {
            Self { max_edge_length, preserve_boundary, feature_angle_threshold }
        }
    }

    impl MeshSimplifier for QuadricErrorSimplifier {
        /// `simplify` (:413-473)
        fn simplify(&self, ctx: &HipContext, mesh: &TriangleMesh, reduction_ratio: f32) -> Result<TriangleMesh> {
            let mut cfg = ffi_qem::tc_qem_config { reduction_ratio: 0.0, preserve_boundary: 0, max_edge_length: 0.0 };
            unsafe { ffi_qem::tc_qem_config_default(reduction_ratio, &mut cfg) };
            cfg.preserve_boundary = self.preserve_boundary as u32;
            cfg.max_edge_length = self.max_edge_length.unwrap_or(0.0);      // 0 = no limit
            let (n, m) = (mesh.vertices.len(), mesh.faces.len());
            let mut faces = Vec::with_capacity(3 * m);
            for face in &mesh.faces {
                for &v in face {
                    faces.push(u32::try_from(v).unwrap_or(u32::MAX));
                }
            }
            let mut out_v = vec![Point3f::origin(); n];
            let mut out_f = vec![0u32; 3 * m];
            let (mut nv, mut nf) = (0usize, 0usize);
            ctx.check(unsafe {
                ffi_qem::tc_simplify_quadric(
                    ctx.0, mesh.vertices.as_ptr() as *const f32, n, faces.as_ptr(), m, &cfg, out_v.as_mut_ptr() as *mut f32, n,
                    out_f.as_mut_ptr(), m, std::ptr::null_mut(), &mut nv, &mut nf, std::ptr::null_mut())
            })?;
            out_v.truncate(nv);
            let new_faces = (0..nf).map(|f| [out_f[3 * f] as usize, out_f[3 * f + 1] as usize, out_f[3 * f + 2] as usize]).collect();
            Ok(TriangleMesh::from_vertices_and_faces(out_v, new_faces))
        }
    }
}

/// Marching cubes on the device (include/threecrate_hip_mc.h; `threecrate-reconstruction/src/marching_cubes.rs`).  The per-cube
/// triangulation comes from the library's generated case table, not the reference's; numbering, winding, positions and normals follow it.
pub mod reconstruction {
    use crate::{ffi_alpha, ffi_mc, HipContext};
    use threecrate_core::{Error, Point3f, PointCloud, Result, TriangleMesh, Vector3f};

    /// `VolumetricGrid` (:12-65): `values[x][y][z]`
    #[derive(Debug, Clone)]
    pub struct VolumetricGrid {
        pub values: Vec<Vec<Vec<f32>>>,
        pub dimensions: [usize; 3],
        pub voxel_size: [f32; 3],
        pub origin: Point3f,
    }

    impl VolumetricGrid {
        pub fn new(dimensions: [usize; 3], voxel_size: [f32; 3], origin: Point3f) -> Self {
            Self { values: vec![vec![vec![0.0; dimensions[2]]; dimensions[1]]; dimensions[0]], dimensions, voxel_size, origin }
        }
    }

    /// `MarchingCubesConfig` (:141-161)
    #[derive(Debug, Clone)]
    pub struct MarchingCubesConfig {
        pub iso_level: f32,
        pub compute_normals: bool,
        pub smooth_mesh: bool,
        pub smoothing_iterations: usize,
    }

    impl Default for MarchingCubesConfig {
        fn default() -> Self {
            Self { iso_level: 0.0, compute_normals: true, smooth_mesh: false, smoothing_iterations: 3 }
        }
    }

    /// `MarchingCubes` (:463-541)
    pub struct MarchingCubes {
        config: MarchingCubesConfig,
    }

    impl MarchingCubes {
        pub fn new(config: MarchingCubesConfig) -> Self {
            Self { config }
        }

        /// `extract_isosurface`: unwelded, a vertex per crossing edge per cube, as the reference lays its mesh out
        pub fn extract_isosurface(&self, ctx: &HipContext, grid: &VolumetricGrid) -> Result<TriangleMesh> {
            if self.config.smooth_mesh {
                return Err(Error::Unsupported("the reference's smoothing sums neighbours in hash-set order".into()));
            }
            let [nx, ny, nz] = grid.dimensions;
            let mut values = Vec::with_capacity(nx * ny * nz);
            for plane in &grid.values {
                for row in plane {
                    values.extend_from_slice(row);
                }
            }
            if values.len() != nx * ny * nz || nx > u32::MAX as usize || ny > u32::MAX as usize || nz > u32::MAX as usize {
                return Err(Error::InvalidData("VolumetricGrid: values do not match dimensions".into()));
            }
            let g = ffi_mc::tc_mc_grid {
                dims: [nx as u32, ny as u32, nz as u32],
                voxel_size: grid.voxel_size,
                origin: [grid.origin.x, grid.origin.y, grid.origin.z],
                layout: ffi_mc::TC_MC_Z_FASTEST,
            };
            let mut cfg = ffi_mc::tc_mc_config { iso_level: 0.0, flags: 0 };
            unsafe { ffi_mc::tc_mc_config_default(&mut cfg) };
            cfg.iso_level = self.config.iso_level;
            cfg.flags = if self.config.compute_normals { ffi_mc::TC_MC_NORMALS } else { 0 };
            let (mut nv, mut nf) = (0usize, 0usize);
            // two calls: the counts, then the mesh
            ctx.check(unsafe {
                ffi_mc::tc_marching_cubes(ctx.0, &g, values.as_ptr(), std::ptr::null(), &cfg, std::ptr::null_mut(), std::ptr::null_mut(),
                                          std::ptr::null_mut(), 0, 0, &mut nv, &mut nf)
            })?;
            if nv == 0 {
                return Err(Error::Algorithm("No isosurface found at specified level".to_string()));
            }
            let mut out_v = vec![Point3f::origin(); nv];
            let mut out_n = if self.config.compute_normals { Some(vec![Vector3f::zeros(); nv]) } else { None };
            let mut out_f = vec![0u32; 3 * nf];
            ctx.check(unsafe {
                ffi_mc::tc_marching_cubes(ctx.0, &g, values.as_ptr(), std::ptr::null(), &cfg, out_v.as_mut_ptr() as *mut f32,
                                          out_n.as_mut().map_or(std::ptr::null_mut(), |v| v.as_mut_ptr() as *mut f32), out_f.as_mut_ptr(), nv, nf,
                                          &mut nv, &mut nf)
            })?;
            let faces = (0..nf).map(|f| [out_f[3 * f] as usize, out_f[3 * f + 1] as usize, out_f[3 * f + 2] as usize]).collect();
            let mut mesh = TriangleMesh::from_vertices_and_faces(out_v, faces);
            if let Some(normals) = out_n {
                mesh.set_normals(normals);
            }
            Ok(mesh)
        }
    }

    /// `marching_cubes(grid, iso_level)` (:857-864)
    pub fn marching_cubes(ctx: &HipContext, grid: &VolumetricGrid, iso_level: f32) -> Result<TriangleMesh> {
        MarchingCubes::new(MarchingCubesConfig { iso_level, ..Default::default() }).extract_isosurface(ctx, grid)
    }

    /// `AlphaMode` (alpha_shape.rs:20-29)
    #[derive(Debug, Clone, PartialEq)]
    pub enum AlphaMode {
        BoundaryOnly,
        Full,
        Adaptive,
    }

    /// `AlphaComplexConfig` (alpha_shape.rs:8-40), and the cap of `generate_triangles_quality` as a field: 50 000 is the reference's, 0 lifts it
    #[derive(Debug, Clone)]
    pub struct AlphaComplexConfig {
        pub alpha: f32,
        pub mode: AlphaMode,
        pub min_triangle_area: f32,
        pub fast_mode: bool,
        pub max_triangles: u32,
    }

    impl Default for AlphaComplexConfig {
        fn default() -> Self {
            Self { alpha: 1.0, mode: AlphaMode::BoundaryOnly, min_triangle_area: 1e-8, fast_mode: false, max_triangles: 50000 }
        }
    }

    /// `alpha_complex_reconstruction_with_config` (:488-494) over include/threecrate_hip_alpha.h: the quality road, boundary or full.
    /// `fast_mode` and `AlphaMode::Adaptive` are not served.  Two calls: the counts, then the faces
    pub fn alpha_complex_reconstruction_with_config(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: &AlphaComplexConfig) -> Result<TriangleMesh> {
        if config.fast_mode || config.mode == AlphaMode::Adaptive {
            return Err(Error::Unsupported("alpha shape: fast_mode and the adaptive mode are not served by the HIP backend".into()));
        }
        if cloud.points.is_empty() {
            return Err(Error::InvalidData("Point cloud is empty".to_string()));
        }
        let mut cfg = ffi_alpha::tc_alpha_config { alpha: 0.0, mode: 0, min_triangle_area: 0.0, max_triangles: 0 };
        unsafe { ffi_alpha::tc_alpha_config_default(config.alpha, &mut cfg) };
        cfg.mode = if config.mode == AlphaMode::Full { ffi_alpha::TC_ALPHA_FULL } else { ffi_alpha::TC_ALPHA_BOUNDARY_ONLY };
        cfg.min_triangle_area = config.min_triangle_area;
        cfg.max_triangles = config.max_triangles;
        let n = cloud.points.len();
        let points = cloud.points.as_ptr() as *const f32;
        let mut stats = ffi_alpha::tc_alpha_stats::default();
        ctx.check(unsafe { ffi_alpha::tc_alpha_shape(ctx.0, points, n, &cfg, std::ptr::null_mut(), 0, &mut stats) })?;
        let nf = stats.faces as usize;
        let mut out_f = vec![0u32; 3 * nf];
        ctx.check(unsafe { ffi_alpha::tc_alpha_shape(ctx.0, points, n, &cfg, out_f.as_mut_ptr(), nf, &mut stats) })?;
        let faces = (0..nf).map(|f| [out_f[3 * f] as usize, out_f[3 * f + 1] as usize, out_f[3 * f + 2] as usize]).collect();
        Ok(TriangleMesh::from_vertices_and_faces(cloud.points.clone(), faces))
    }

    /// `alpha_shape_reconstruction(cloud, alpha)` (:508-510): boundary only, the reference's cap
    pub fn alpha_shape_reconstruction(ctx: &HipContext, cloud: &PointCloud<Point3f>, alpha: f32) -> Result<TriangleMesh> {
        alpha_complex_reconstruction_with_config(ctx, cloud, &AlphaComplexConfig { alpha, ..Default::default() })
    }
}

/// Ground segmentation of a LiDAR frame on the device (include/threecrate_hip_ground.h; `threecrate-algorithms/src/ground_segmentation.rs`).
/// The header lists the deviations: the sums are f64, a point that is not finite is non-ground.
pub mod ground {
    use crate::{ffi_ground, HipContext};
    use threecrate_core::{Error, Point3f, PointCloud, Result};

    /// `PatchworkConfig` (:24-77)
    #[derive(Debug, Clone)]
    pub struct PatchworkConfig {
        pub sensor_height: f32,
        pub zone_radii: Vec<f32>,
        pub num_rings_per_zone: Vec<usize>,
        pub num_sectors_per_zone: Vec<usize>,
        pub max_range: f32,
        pub min_points_per_patch: usize,
        pub num_seed_points: usize,
        pub seed_selection_threshold: f32,
        pub dist_threshold: f32,
        pub num_iterations: usize,
        pub uprightness_threshold: f32,
        pub flatness_threshold: f32,
        pub elevation_threshold: f32,
    }

    impl Default for PatchworkConfig {
        fn default() -> Self {
            let mut c = ffi_ground::tc_ground_config::default();
            unsafe { ffi_ground::tc_ground_config_default(1.723, &mut c) };
            let nz = c.n_zones as usize;
            Self {
                sensor_height: c.sensor_height,
                zone_radii: c.zone_radii[..nz + 1].to_vec(),
                num_rings_per_zone: c.num_rings[..nz].iter().map(|&v| v as usize).collect(),
                num_sectors_per_zone: c.num_sectors[..nz].iter().map(|&v| v as usize).collect(),
                max_range: c.max_range,
                min_points_per_patch: c.min_points_per_patch as usize,
                num_seed_points: c.num_seed_points as usize,
                seed_selection_threshold: c.seed_selection_threshold,
                dist_threshold: c.dist_threshold,
                num_iterations: c.num_iterations as usize,
                uprightness_threshold: c.uprightness_threshold,
                flatness_threshold: c.flatness_threshold,
                elevation_threshold: c.elevation_threshold,
            }
        }
    }

    /// `GroundSegmentationResult` (:81-88)
    #[derive(Debug, Clone)]
    pub struct GroundSegmentationResult {
        pub ground: PointCloud<Point3f>,
        pub nonground: PointCloud<Point3f>,
        pub labels: Vec<bool>,
    }

    fn narrow(v: usize) -> u32 {
        v.min(u32::MAX as usize) as u32
    }

    /// the length checks of `validate_config` (:90-106), which a fixed-size struct cannot carry, then the struct
    fn to_ffi(config: &PatchworkConfig) -> Result<ffi_ground::tc_ground_config> {
        let nz = config.num_rings_per_zone.len();
        if nz == 0 {
            return Err(Error::InvalidData("num_rings_per_zone must be non-empty".into()));
        }
        if config.zone_radii.len() != nz + 1 {
            return Err(Error::InvalidData("zone_radii.len() must equal num_rings_per_zone.len() + 1".into()));
        }
        if config.num_sectors_per_zone.len() != nz {
            return Err(Error::InvalidData("num_sectors_per_zone.len() must equal num_rings_per_zone.len()".into()));
        }
        let mut c = ffi_ground::tc_ground_config::default();
        c.sensor_height = config.sensor_height;
        c.n_zones = narrow(nz);
        let kept = nz.min(ffi_ground::TC_GROUND_MAX_ZONES);          // more zones than the struct holds: the library answers
        c.zone_radii[..kept + 1].copy_from_slice(&config.zone_radii[..kept + 1]);
        for z in 0..kept {
            c.num_rings[z] = narrow(config.num_rings_per_zone[z]);
            c.num_sectors[z] = narrow(config.num_sectors_per_zone[z]);
        }
        c.max_range = config.max_range;
        c.min_points_per_patch = narrow(config.min_points_per_patch);
        c.num_seed_points = narrow(config.num_seed_points);
        c.seed_selection_threshold = config.seed_selection_threshold;
        c.dist_threshold = config.dist_threshold;
        c.num_iterations = narrow(config.num_iterations);
        c.uprightness_threshold = config.uprightness_threshold;
        c.flatness_threshold = config.flatness_threshold;
        c.elevation_threshold = config.elevation_threshold;
        Ok(c)
    }

    /// `patchwork_plus_plus(cloud, config)` (:336-407)
    pub fn patchwork_plus_plus(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: PatchworkConfig) -> Result<GroundSegmentationResult> {
        let cfg = to_ffi(&config)?;
        let n = cloud.points.len();
        let mut labels = vec![0u8; n.max(1)];
        let mut n_ground = 0usize;
        let points = if n == 0 { std::ptr::null() } else { cloud.points.as_ptr() as *const f32 };
        ctx.check(unsafe {
            ffi_ground::tc_segment_ground(ctx.0, points, n, &cfg, labels.as_mut_ptr(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), &mut n_ground)
        })?;
        let mut ground = PointCloud::with_capacity(n_ground);
        let mut nonground = PointCloud::with_capacity(n - n_ground);
        for (i, p) in cloud.points.iter().enumerate() {
            if labels[i] != 0 { ground.push(*p) } else { nonground.push(*p) }
        }
        Ok(GroundSegmentationResult { ground, nonground, labels: labels[..n].iter().map(|&l| l != 0).collect() })
    }

    /// `segment_ground(cloud, sensor_height)` (:410-419)
    pub fn segment_ground(ctx: &HipContext, cloud: &PointCloud<Point3f>, sensor_height: f32) -> Result<GroundSegmentationResult> {
        patchwork_plus_plus(ctx, cloud, PatchworkConfig { sensor_height, ..Default::default() })
    }
}

/// SHOT and USC descriptors with their local reference frame on the device (include/threecrate_hip_shot.h;
/// `threecrate-algorithms/src/features.rs:287-645`).  The header lists the deviations: the frame is f64, an even vote on the x axis takes a
/// canonical sign, a point that is not finite gets an all-zero row.
pub mod features {
    use crate::{ffi_shot, HipContext};
    use threecrate_core::{NormalPoint3f, PointCloud, Result};

    /// `SHOT_DIM` / `USC_DIM` (features.rs:304, :313)
    pub const SHOT_DIM: usize = ffi_shot::TC_SHOT_DIM;
    pub const USC_DIM: usize = ffi_shot::TC_USC_DIM;

    /// `ShotVariant` (features.rs:316-323)
    #[derive(Debug, Clone, Copy, PartialEq, Default)]
    pub enum ShotVariant {
        #[default]
        Standard,
        UniqueShapeContext,
    }

    /// `ShotConfig` (features.rs:326-344): same fields and defaults
    #[derive(Debug, Clone)]
    pub struct ShotConfig {
        pub search_radius: f32,
        pub k_neighbors: usize,
        pub variant: ShotVariant,
    }

    impl Default for ShotConfig {
        fn default() -> Self {
            Self { search_radius: 0.2, k_neighbors: 10, variant: ShotVariant::Standard }
        }
    }

    /// The frames and flags of a call that asks for them: row i is x, y, z of point i's frame; `TC_SHOT_*` bits per point
    pub struct ShotFrames {
        pub frames: Vec<[f32; 9]>,
        pub flags: Vec<u32>,
    }

    fn to_ffi(config: &ShotConfig) -> ffi_shot::tc_shot_config {
        let variant = match config.variant {
            ShotVariant::Standard => ffi_shot::TC_SHOT_VARIANT_SHOT,
            ShotVariant::UniqueShapeContext => ffi_shot::TC_SHOT_VARIANT_USC,
        };
        ffi_shot::tc_shot_config { search_radius: config.search_radius, k_neighbors: config.k_neighbors, variant }
    }

    /// `extract_shot_features_with_normals` (features.rs:605-645): one row of 352 (SHOT) or 128 (USC) values per point, in input order
    pub fn extract_shot_features_with_normals(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>, config: &ShotConfig) -> Result<Vec<Vec<f32>>> {
        Ok(extract_shot_features_with_frames(ctx, cloud, config, false)?.0)
    }

    /// The same with every point's local reference frame and flags (`want_frames`; otherwise both lists are empty)
    pub fn extract_shot_features_with_frames(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>, config: &ShotConfig,
                                             want_frames: bool) -> Result<(Vec<Vec<f32>>, ShotFrames)> {
        let n = cloud.points.len();
        let cfg = to_ffi(config);
        let dim = unsafe { ffi_shot::tc_shot_dim(cfg.variant) };
        let mut out = vec![0.0f32; (n * dim).max(1)];
        let mut frames = vec![[0.0f32; 9]; if want_frames { n } else { 0 }];
        let mut flags = vec![0u32; if want_frames { n } else { 0 }];
        let (lrf, fl) = if want_frames { (frames.as_mut_ptr() as *mut f32, flags.as_mut_ptr()) } else { (std::ptr::null_mut(), std::ptr::null_mut()) };
        ctx.check(unsafe {
            ffi_shot::tc_extract_shot_features_with_normals(ctx.0, cloud.points.as_ptr() as *const f32, n, &cfg, out.as_mut_ptr(), lrf, fl)
        })?;
        Ok((out[..n * dim].chunks(dim.max(1)).map(|c| c.to_vec()).collect(), ShotFrames { frames, flags }))
    }
}

/// Poisson surface reconstruction on the device (include/threecrate_hip_poisson.h; `threecrate-reconstruction/src/poisson.rs`).  The header
/// lists the deviation: the reference's entry checks are kept, its octree solver is replaced by a dense-grid solve of 2^depth nodes per axis.
pub mod reconstruction {
    use crate::{estimate_normals, ffi_poisson, HipContext};
    use threecrate_core::{NormalPoint3f, Point3f, PointCloud, Result, TriangleMesh};

    /// `PoissonConfig` (poisson.rs:8-43) where its names have a meaning on a dense grid (depth, scale); the other fields are this library's
    #[derive(Debug, Clone)]
    pub struct PoissonConfig {
        pub depth: u32,
        pub scale: f32,
        pub point_weight: f32,
        pub max_iterations: u32,
        pub tolerance: f32,
        pub min_density: f32,
    }

    impl Default for PoissonConfig {
        /// depth 6: what the reference's clamp makes of its default 8
        fn default() -> Self {
            Self { depth: 6, scale: 1.1, point_weight: 0.0, max_iterations: 200, tolerance: 1e-5, min_density: 0.0 }
        }
    }

    /// `poisson_reconstruction` (poisson.rs:53-150): a closed mesh of an oriented cloud.  Two calls: the counts, then the mesh
    pub fn poisson_reconstruction(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>, config: &PoissonConfig) -> Result<TriangleMesh> {
        let n = cloud.points.len();
        let points: Vec<f32> = cloud.points.iter().flat_map(|p| [p.position.x, p.position.y, p.position.z]).collect();
        let normals: Vec<f32> = cloud.points.iter().flat_map(|p| [p.normal.x, p.normal.y, p.normal.z]).collect();
        let cfg = ffi_poisson::tc_poisson_config {
            depth: config.depth, scale: config.scale, point_weight: config.point_weight, max_iterations: config.max_iterations,
            tolerance: config.tolerance, min_density: config.min_density,
        };
        let mut stats = ffi_poisson::tc_poisson_stats::default();
        let (mut nv, mut nf) = (0usize, 0usize);
        ctx.check(unsafe {
            ffi_poisson::tc_poisson_reconstruct(ctx.0, points.as_ptr(), normals.as_ptr(), n, &cfg, std::ptr::null_mut(), std::ptr::null_mut(), 0, 0,
                                                &mut nv, &mut nf, &mut stats)
        })?;
        let mut out_v = vec![Point3f::origin(); nv.max(1)];
        let mut out_f = vec![0u32; (3 * nf).max(1)];
        ctx.check(unsafe {
            ffi_poisson::tc_poisson_reconstruct(ctx.0, points.as_ptr(), normals.as_ptr(), n, &cfg, out_v.as_mut_ptr() as *mut f32, out_f.as_mut_ptr(),
                                                nv, nf, &mut nv, &mut nf, &mut stats)
        })?;
        out_v.truncate(nv);
        let faces = (0..nf).map(|f| [out_f[3 * f] as usize, out_f[3 * f + 1] as usize, out_f[3 * f + 2] as usize]).collect();
        Ok(TriangleMesh::from_vertices_and_faces(out_v, faces))
    }

    /// `poisson_reconstruction_default` (poisson.rs:154-156)
    pub fn poisson_reconstruction_default(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>) -> Result<TriangleMesh> {
        poisson_reconstruction(ctx, cloud, &PoissonConfig::default())
    }

    /// `poisson_reconstruction_with_normals` (poisson.rs:167-180): estimate_normals(cloud, k), then the reconstruction
    pub fn poisson_reconstruction_with_normals(ctx: &HipContext, cloud: &PointCloud<Point3f>, k: usize, config: &PoissonConfig) -> Result<TriangleMesh> {
        let with_normals = estimate_normals(ctx, cloud, k)?;
        poisson_reconstruction(ctx, &with_normals, config)
    }
}
