"""threecrate_amd -- MI355X (gfx950) native normals + ICP backend for threecrate.

The product is libthreecrate_hip.so (hand-written HIP kernels behind the C ABI of
include/threecrate_hip.h).  This package is the thin host-side mirror of the reference's
operator interface for that one path (estimate_normals / icp / icp_point_to_plane and the
threecrate-gpu facade).  It never falls back to a CPU implementation.
"""
from .api import (  # noqa: F401
    IcpScaleLevel, MultiScaleIcpConfig,
    AlgorithmError, BatchICPJob, BatchICPResult, Error, GpuContext, GpuError, ICPResult, IDENTITY, InvalidData,
    NormalEstimationConfig, Unsupported, default_context, estimate_normals, estimate_normals_radius,
    estimate_normals_with_config, gpu_batch_icp, gpu_estimate_normals, gpu_icp, gpu_icp_point_to_plane, icp,
    icp_detailed, icp_point_to_plane, icp_point_to_plane_detailed, icp_point_to_point, icp_point_to_point_default,
    isometry_to_matrix, voxel_grid_filter, gpu_voxel_grid_filter,
    OutlierResult, statistical_outlier_removal, statistical_outlier_removal_with_threshold, radius_outlier_removal,
    gpu_remove_statistical_outliers, gpu_radius_outlier_removal,
    PlaneSegmentationResult, GpuPlaneSegmentationConfig, segment_plane, segment_plane_ransac, plane_segmentation_ransac,
    gpu_segment_plane, gpu_segment_plane_ransac,
    NdtConfig, NdtResult, ndt_registration, ndt_registration_default,
    GlobalRegistrationConfig, GlobalRegistrationResult, RansacResult, global_registration, global_registration_with_normals,
    rotation_to_isometry,
    CameraIntrinsics, TsdfVolume, VoxelMap, create_tsdf_volume, gpu_tsdf_integrate, gpu_tsdf_extract_surface,
    GicpConfig, gicp, KissIcpConfig, kiss_icp, BackpressureConfig, FrameResult, FrameStream, RealtimeMetrics, read_kitti_bin, SearchIndex, Cloud,
)

__all__ = [n for n in dir() if not n.startswith("_")]
