"""ctypes binding of libthreecrate_hip.so (include/threecrate_hip.h, include/threecrate_hip_filters.h,
include/threecrate_hip_segmentation.h, include/threecrate_hip_ndt.h, include/threecrate_hip_tsdf.h) and of its companions
libthreecrate_hip_global.so (include/threecrate_hip_global.h), libthreecrate_hip_voxelmap.so (include/threecrate_hip_voxelmap.h),
libthreecrate_hip_color.so (include/threecrate_hip_color.h), libthreecrate_hip_mesh.so (include/threecrate_hip_mesh.h),
libthreecrate_hip_simplify.so (include/threecrate_hip_simplify.h), libthreecrate_hip_mc.so (include/threecrate_hip_mc.h),
libthreecrate_hip_qem.so (include/threecrate_hip_qem.h), libthreecrate_hip_alpha.so (include/threecrate_hip_alpha.h),
libthreecrate_hip_ground.so (include/threecrate_hip_ground.h), libthreecrate_hip_shot.so (include/threecrate_hip_shot.h) and
libthreecrate_hip_poisson.so (include/threecrate_hip_poisson.h).

The shared library is the product; this module only declares its C ABI.  There is no
Python / CPU fallback: if the library is missing, `load()` raises.
"""
import collections
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# TC_HIP_LIB: another build of the same library (the host-side ASan / UBSan build of tools/sanitize_cpu.sh)
LIB_PATH = os.environ.get("TC_HIP_LIB") or os.path.join(_HERE, "libthreecrate_hip.so")

TC_OK, TC_INVALID_DATA, TC_ALGORITHM, TC_GPU, TC_UNSUPPORTED = 0, 1, 2, 3, 4
TC_COMM_ID_BYTES = 128
TC_COLL_SUM_F64, TC_COLL_SUM_U32, TC_COLL_ALLGATHER_U8 = 0, 1, 2
TC_SHARD_SPATIAL, TC_SHARD_LOCAL, TC_SHARD_INDEX = 0, 1, 2
TC_COUNTER_INDEXED_POINTS, TC_COUNTER_INDEX_BUILDS = 0, 1
(TC_COUNTER_ICP_ITERATIONS, TC_COUNTER_ICP_TRIPS, TC_COUNTER_ICP_TRIPS_WITHOUT_SEARCH, TC_COUNTER_ICP_SEARCHES, TC_COUNTER_ICP_STEPS_NEEDED,
 TC_COUNTER_ICP_STEPS_TAKEN) = 2, 3, 4, 5, 6, 7
# int (*tc_host_collective_fn)(void *user, int op, void *host_buf, size_t count)
HOST_COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t)
SUMS_P2PLANE, SUMS_P2P, SUMS_STRIDE = 29, 17, 32
TC_TSDF_OBSERVED_EDGES = 1


class NormalConfig(C.Structure):
    _fields_ = [("k_neighbors", C.c_uint64), ("radius", C.c_float), ("has_radius", C.c_int32),
                ("consistent_orientation", C.c_int32), ("has_viewpoint", C.c_int32),
                ("viewpoint", C.c_float * 3)]


class IcpResultC(C.Structure):
    _fields_ = [("transformation", C.c_float * 7), ("mse", C.c_float), ("iterations", C.c_uint64),
                ("converged", C.c_int32), ("n_correspondences", C.c_uint64),
                ("corr_target", C.c_void_p)]


class BatchJobC(C.Structure):
    _fields_ = [("source", C.c_void_p), ("n_source", C.c_size_t), ("target", C.c_void_p),
                ("n_target", C.c_size_t), ("max_iterations", C.c_size_t),
                ("convergence_threshold", C.c_float), ("max_correspondence_distance", C.c_float)]


class BatchResultC(C.Structure):
    _fields_ = [("transformation", C.c_float * 7), ("final_error", C.c_float),
                ("iterations", C.c_uint64), ("status", C.c_int32)]


class ScaleLevelC(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("max_iterations", C.c_size_t), ("max_correspondence_distance", C.c_float)]


class MultiScaleConfigC(C.Structure):
    _fields_ = [("levels", C.POINTER(ScaleLevelC)), ("n_levels", C.c_size_t), ("final_refinement_iterations", C.c_size_t),
                ("final_max_correspondence_distance", C.c_float), ("convergence_threshold", C.c_float)]


class GicpConfigC(C.Structure):
    _fields_ = [("max_iterations", C.c_size_t), ("max_correspondence_distance", C.c_float), ("convergence_threshold", C.c_float),
                ("k_correspondences", C.c_size_t)]


class KissIcpConfigC(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("max_range", C.c_float), ("min_range", C.c_float), ("max_iterations", C.c_size_t)]


class FrameStreamConfigC(C.Structure):
    _fields_ = [("max_points", C.c_size_t), ("max_queue_depth", C.c_size_t), ("voxel_size", C.c_float),
                ("k_neighbors", C.c_size_t), ("max_iterations", C.c_size_t),
                ("max_correspondence_distance", C.c_float), ("convergence_threshold", C.c_float)]


class FrameResultC(C.Structure):
    _fields_ = [("transformation", C.c_float * 7), ("mse", C.c_float), ("iterations", C.c_uint64),
                ("converged", C.c_int32), ("status", C.c_int32), ("n_points_in", C.c_uint64), ("n_points", C.c_uint64)]


class FrameStreamMetricsC(C.Structure):
    _fields_ = [("items_queued", C.c_uint64), ("items_processed", C.c_uint64), ("items_dropped", C.c_uint64),
                ("max_depth_seen", C.c_uint64)]


class NdtConfigC(C.Structure):
    _fields_ = [("resolution", C.c_float), ("step_size", C.c_float), ("max_iterations", C.c_size_t), ("epsilon", C.c_float),
                ("min_points_per_voxel", C.c_size_t)]


class NdtResultC(C.Structure):
    _fields_ = [("transformation", C.c_float * 7), ("score", C.c_float), ("iterations", C.c_size_t), ("converged", C.c_int),
                ("n_voxels", C.c_size_t), ("n_hits", C.c_size_t)]


class TsdfVolumeConfigC(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("truncation_distance", C.c_float), ("resolution", C.c_uint32 * 3), ("origin", C.c_float * 3),
                ("max_weight", C.c_uint32)]


class CameraIntrinsicsC(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32)]


class RansacResultC(C.Structure):
    _fields_ = [("inlier_count", C.c_uint64), ("iterations_run", C.c_uint64), ("best_iteration", C.c_uint32), ("early_exit", C.c_int32),
                ("inlier_ratio", C.c_float)]


class VoxelMapConfigC(C.Structure):
    _fields_ = [("voxel_size", C.c_float), ("initial_capacity", C.c_size_t)]


class ColorSourceC(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("depth", C.c_void_p), ("intrinsics", CameraIntrinsicsC), ("world_to_camera", C.c_float * 12)]


class ColorizeConfigC(C.Structure):
    _fields_ = [("default_color", C.c_uint8 * 3), ("interpolation", C.c_uint8), ("min_depth", C.c_float), ("depth_tolerance", C.c_float)]


class MeshSmoothConfigC(C.Structure):
    _fields_ = [("method", C.c_uint32), ("iterations", C.c_uint32), ("lambda", C.c_float), ("mu", C.c_float), ("alpha", C.c_float), ("beta", C.c_float)]


class SimplifyConfigC(C.Structure):
    _fields_ = [("strategy", C.c_uint32), ("preserve_boundary", C.c_uint32), ("feature_angle_threshold", C.c_float), ("reduction_ratio", C.c_float)]


class QemConfigC(C.Structure):
    _fields_ = [("reduction_ratio", C.c_float), ("preserve_boundary", C.c_uint32), ("max_edge_length", C.c_float)]


class AlphaConfigC(C.Structure):
    _fields_ = [("alpha", C.c_float), ("mode", C.c_uint32), ("min_triangle_area", C.c_float), ("max_triangles", C.c_uint32)]


class AlphaStatsC(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("boundary_candidates", C.c_uint64), ("faces", C.c_uint64), ("capped", C.c_uint32)]


TC_GROUND_MAX_ZONES = 8


class GroundConfigC(C.Structure):
    _fields_ = [("sensor_height", C.c_float), ("n_zones", C.c_uint32), ("zone_radii", C.c_float * (TC_GROUND_MAX_ZONES + 1)),
                ("num_rings", C.c_uint32 * TC_GROUND_MAX_ZONES), ("num_sectors", C.c_uint32 * TC_GROUND_MAX_ZONES), ("max_range", C.c_float),
                ("min_points_per_patch", C.c_uint32), ("num_seed_points", C.c_uint32), ("seed_selection_threshold", C.c_float),
                ("dist_threshold", C.c_float), ("num_iterations", C.c_uint32), ("uprightness_threshold", C.c_float),
                ("flatness_threshold", C.c_float), ("elevation_threshold", C.c_float)]


class GroundPatchC(C.Structure):
    _fields_ = [("count", C.c_uint32), ("n_inliers", C.c_uint32), ("status", C.c_uint32), ("normal", C.c_float * 3), ("d", C.c_float),
                ("mean_z", C.c_float), ("flatness", C.c_float)]


class ShotConfigC(C.Structure):
    _fields_ = [("search_radius", C.c_float), ("k_neighbors", C.c_size_t), ("variant", C.c_int)]


class PoissonConfigC(C.Structure):
    _fields_ = [("depth", C.c_uint32), ("scale", C.c_float), ("point_weight", C.c_float), ("max_iterations", C.c_uint32), ("tolerance", C.c_float),
                ("min_density", C.c_float)]


class PoissonStatsC(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("rel_residual", C.c_float), ("iso_value", C.c_float), ("occupied_nodes", C.c_uint32)]


class McGridC(C.Structure):
    _fields_ = [("dims", C.c_uint32 * 3), ("voxel_size", C.c_float * 3), ("origin", C.c_float * 3), ("layout", C.c_uint32)]


class McConfigC(C.Structure):
    _fields_ = [("iso_level", C.c_float), ("flags", C.c_uint32)]


class KernelStatC(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("min_ms", C.c_double), ("max_ms", C.c_double)]


Surface = collections.namedtuple("Surface", "header rust rows structs")


def _surfaces():
    """One entry per header of include/, in the order the headers arrived: its file name, its Rust declarations file
    (bindings/rust/threecrate-hip/src), its signature rows and its structs (C name -> ctypes mirror).  A row names every export that
    has its signature, (names...): (restype, argtypes): a host entry point and its *_device twin take the same list.  argtypes None:
    the symbol takes no arguments and gets none set.  tests/test_abi_surfaces.py holds every entry to its header, its Rust file and
    the library; tests/test_abi_conformance.py holds the structs to the compiled layouts."""
    vp, f32p, sz, f, i, u64 = C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_uint64
    out, szp, fp, u32p = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    resp, ncfg = C.POINTER(IcpResultC), C.POINTER(NormalConfig)
    pair = [vp, f32p, sz, f32p, sz, f32p]                   # context, source, n, target, n, init
    main = Surface("threecrate_hip.h", "ffi.rs", {
        ("tc_abi_version", "tc_device_count"): (i, None),
        ("tc_context_create",): (i, [i, out]),
        ("tc_context_create_on_stream",): (i, [i, vp, out]),
        ("tc_context_wait_stream", "tc_stream_wait_context"): (i, [vp, vp]),
        ("tc_context_trim", "tc_synchronize"): (i, [vp]),
        ("tc_context_destroy", "tc_cloud_destroy", "tc_comm_destroy", "tc_icp_shard_destroy", "tc_search_index_destroy",
         "tc_frame_stream_destroy", "tc_profile_reset"): (None, [vp]),
        ("tc_last_error_message",): (C.c_char_p, [vp]),
        ("tc_normal_config_default",): (None, [ncfg]),
        ("tc_estimate_normals", "tc_estimate_normals_device"): (i, [vp, f32p, sz, ncfg, f32p]),
        ("tc_estimate_normals_slice_device",): (i, [vp, f32p, sz, ncfg, sz, sz, f32p]),
        ("tc_normals_unsort_device",): (i, [vp, f32p, sz, f32p]),
        ("tc_icp_detailed", "tc_icp_detailed_device", "tc_icp_point_to_point"): (i, pair + [sz, f, f, resp]),
        ("tc_icp",): (i, pair + [sz, f32p]),
        ("tc_icp_point_to_plane_detailed", "tc_icp_point_to_plane_detailed_device"):
            (i, [vp, f32p, sz, f32p, sz, f32p, sz, sz, f32p, sz, f, f, resp]),
        ("tc_batch_icp",): (i, [out, sz, C.POINTER(BatchJobC), sz, C.POINTER(BatchResultC)]),
        ("tc_icp_shard_create",): (i, [vp, i, f32p, sz, f32p, sz, f32p, sz, f32p, f, f, out]),
        ("tc_icp_shard_sums", "tc_cloud_points_device", "tc_cloud_normals_device"): (C.c_void_p, [vp]),
        ("tc_icp_shard_reduce", "tc_icp_shard_apply", "tc_comm_unique_id"): (i, [vp]),
        ("tc_icp_shard_get_sums", "tc_icp_shard_set_sums"): (i, [vp, vp]),
        ("tc_icp_shard_done",): (i, [vp, C.POINTER(C.c_int)]),
        ("tc_icp_shard_finish",): (i, [vp, sz, resp]),
        ("tc_cloud_upload", "tc_cloud_upload_device"): (i, [vp, f32p, sz, out]),
        ("tc_cloud_size", "tc_search_index_size"): (sz, [vp]),
        ("tc_cloud_estimate_normals", "tc_cloud_estimate_normals_device"): (i, [vp, ncfg, f32p]),
        ("tc_cloud_set_normals_device",): (i, [vp, f32p, sz, sz]),
        ("tc_cloud_icp_point_to_plane", "tc_cloud_icp_detailed"): (i, [vp, vp, f32p, sz, f, f, resp]),
        ("tc_cloud_sharded_icp",): (i, [vp, i, i, f32p, sz, vp, f32p, sz, f, f, resp]),
        ("tc_comm_create",): (i, [vp, i, i, vp, out]),
        ("tc_comm_adopt",): (i, [vp, vp, i, i, out]),
        ("tc_comm_create_host",): (i, [vp, i, i, HOST_COLLECTIVE_FN, vp, out]),
        ("tc_comm_create_local",): (i, [vp, out]),
        ("tc_comm_rank", "tc_comm_size"): (i, [vp]),
        ("tc_sharded_icp_point_to_plane_device",): (i, [vp, vp, i, f32p, sz, f32p, sz, f32p, sz, sz, f32p, sz, f, f, resp]),
        ("tc_sharded_icp_detailed_device",): (i, [vp, vp, i, f32p, sz, f32p, sz, f32p, sz, f, f, resp]),
        ("tc_sharded_estimate_normals_device",): (i, [vp, vp, f32p, sz, ncfg, f32p]),
        ("tc_sharded_estimate_normals_local_device",): (i, [vp, vp, f32p, sz, ncfg, f32p, vp, szp, szp]),
        ("tc_debug_counter",): (C.c_ulonglong, [vp, i]),
        ("tc_multiscale_icp_point_to_point",): (i, pair + [C.POINTER(MultiScaleConfigC), resp]),
        ("tc_gicp", "tc_gicp_device"): (i, pair + [C.POINTER(GicpConfigC), resp]),
        ("tc_kiss_icp", "tc_kiss_icp_device"): (i, pair + [C.POINTER(KissIcpConfigC), resp, szp]),
        ("tc_knn", "tc_knn_device"): (i, [vp, f32p, sz, f32p, sz, sz, vp, vp, vp]),
        ("tc_radius_search", "tc_radius_search_device"): (i, [vp, f32p, sz, f32p, sz, f, sz, vp, vp, vp]),
        ("tc_search_index_create", "tc_search_index_create_device"): (i, [vp, f32p, sz, sz, out]),
        ("tc_search_index_query", "tc_search_index_query_device"): (i, [vp, f32p, sz, sz, f, vp, vp, vp]),
        ("tc_search_index_radius_count",): (i, [vp, f32p, sz, f, vp]),
        ("tc_search_index_radius_fill",): (i, [vp, f32p, sz, f, vp, sz, vp, vp]),
        ("tc_voxel_grid_filter", "tc_voxel_grid_filter_device"): (i, [vp, f32p, sz, f, f32p, szp]),
        ("tc_extract_euclidean_clusters", "tc_extract_euclidean_clusters_device"): (i, [vp, f32p, sz, f, sz, sz, vp, vp, vp, szp]),
        ("tc_extract_fpfh_features_with_normals", "tc_extract_fpfh_features_with_normals_device", "tc_extract_fpfh_features",
         "tc_extract_fpfh_features_device"): (i, [vp, f32p, sz, f, sz, f32p]),
        ("tc_frame_stream_create",): (i, [vp, C.POINTER(FrameStreamConfigC), out]),
        ("tc_frame_stream_send",): (i, [vp, f32p, sz, sz]),
        ("tc_frame_stream_try_send",): (i, [vp, f32p, sz, sz, C.POINTER(C.c_int)]),
        ("tc_frame_stream_finish",): (i, [vp, C.POINTER(FrameResultC), sz, szp, C.POINTER(FrameStreamMetricsC)]),
        ("tc_read_kitti_bin",): (i, [C.c_char_p, f32p, sz, szp]),
        ("tc_profile_enable",): (None, [vp, i]),
        ("tc_profile_read",): (sz, [vp, C.POINTER(KernelStatC), sz]),
    }, {"tc_normal_config": NormalConfig, "tc_icp_result": IcpResultC, "tc_batch_icp_job": BatchJobC, "tc_batch_icp_result": BatchResultC,
        "tc_kernel_stat": KernelStatC, "tc_icp_scale_level": ScaleLevelC, "tc_multiscale_icp_config": MultiScaleConfigC,
        "tc_gicp_config": GicpConfigC, "tc_kiss_icp_config": KissIcpConfigC, "tc_frame_stream_config": FrameStreamConfigC,
        "tc_frame_result": FrameResultC, "tc_frame_stream_metrics": FrameStreamMetricsC})
    filters = Surface("threecrate_hip_filters.h", "ffi_filters.rs", {
        # context, xyz, n, k_neighbors, std_dev_multiplier, out_xyz, kept_index, mean_distance, n_out, threshold_used
        ("tc_statistical_outlier_removal", "tc_statistical_outlier_removal_device"): (i, [vp, f32p, sz, sz, f, f32p, vp, f32p, szp, fp]),
        ("tc_statistical_outlier_removal_with_threshold", "tc_statistical_outlier_removal_with_threshold_device"):
            (i, [vp, f32p, sz, sz, f, f32p, vp, f32p, szp]),
        # context, xyz, n, radius, min_neighbors, out_xyz, kept_index, n_out
        ("tc_radius_outlier_removal", "tc_radius_outlier_removal_device"): (i, [vp, f32p, sz, f, sz, f32p, vp, szp]),
    }, {})
    segmentation = Surface("threecrate_hip_segmentation.h", "ffi_segmentation.rs", {
        # context, xyz, n, threshold, max_iters, seed, coefficients[4], inlier_index, n_inliers, best_iteration
        ("tc_segment_plane", "tc_segment_plane_device"): (i, [vp, f32p, sz, f, sz, u64, fp, vp, szp, u32p]),
        # context, xyz, n, threshold, samples, n_samples, coefficients[4], inlier_index, n_inliers, best_iteration
        ("tc_segment_plane_samples", "tc_segment_plane_samples_device"): (i, [vp, f32p, sz, f, vp, sz, fp, vp, szp, u32p]),
    }, {})
    ndt = Surface("threecrate_hip_ndt.h", "ffi_ndt.rs", {
        # context, source, n, target, n, init (7 floats or NULL), config, result
        ("tc_ndt_registration", "tc_ndt_registration_device"): (i, [vp, f32p, sz, f32p, sz, f32p, C.POINTER(NdtConfigC), C.POINTER(NdtResultC)]),
        # context, target, n, resolution, min_points_per_voxel, keys, counts, mean, inv_cov, capacity, n_voxels
        ("tc_ndt_voxels", "tc_ndt_voxels_device"): (i, [vp, f32p, sz, f, sz, vp, vp, f32p, f32p, sz, szp]),
    }, {"tc_ndt_config": NdtConfigC, "tc_ndt_result": NdtResultC})
    return [main, filters, segmentation, ndt]


def _extensions():
    """Surfaces that arrived after tests/test_abi_surfaces.py pinned SURFACES to four headers and 104 names: the same kind of entry,
    loaded the same way, each held to the same checks by a test file of its own (tests/test_abi_tsdf.py).  An entry joins SURFACES
    once EXPORT_COUNTS of that file may be edited."""
    vp, sz, i, f, u32, szp = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.c_uint32, C.POINTER(C.c_size_t)
    tsdf = Surface("threecrate_hip_tsdf.h", "ffi_tsdf.rs", {
        ("tc_tsdf_volume_create",): (i, [vp, C.POINTER(TsdfVolumeConfigC), C.POINTER(C.c_void_p)]),
        ("tc_tsdf_volume_destroy",): (None, [vp]),
        ("tc_tsdf_volume_reset",): (i, [vp]),
        # volume, depth, rgb (or NULL), intrinsics, world_to_camera[12], n_updated (or NULL)
        ("tc_tsdf_integrate", "tc_tsdf_integrate_device"): (i, [vp, vp, vp, C.POINTER(CameraIntrinsicsC), C.POINTER(C.c_float), szp]),
        # volume, tsdf, weight, rgb
        ("tc_tsdf_volume_download", "tc_tsdf_volume_download_device", "tc_tsdf_volume_upload", "tc_tsdf_volume_upload_device"): (i, [vp, vp, vp, vp]),
        # volume, iso_value, flags, xyz, rgb, capacity, n_points
        ("tc_tsdf_extract_surface", "tc_tsdf_extract_surface_device"): (i, [vp, f, u32, vp, vp, sz, szp]),
    }, {"tc_tsdf_volume_config": TsdfVolumeConfigC, "tc_camera_intrinsics": CameraIntrinsicsC})
    return [tsdf]


Companion = collections.namedtuple("Companion", Surface._fields + ("library",))


def _companions():
    """Surfaces whose symbols live in a shared library of their own beside the product library and linked against it: the same kind
    of entry plus the library's file name, loaded by load_companion(header), held to the same checks by a test file of its own
    (tests/test_abi_global.py).  load() does not touch them and the product library's set of names stays what it is."""
    vp, sz, f, i, u64, fp = C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_uint64, C.POINTER(C.c_float)
    resp = C.POINTER(RansacResultC)
    head = [vp, vp, sz, vp, sz, vp, vp, sz, f, f]             # context, source, n, target, n, corr_src, corr_tgt, m, threshold, inlier_ratio
    tail = [fp, resp, vp, vp]                                 # transform[12], result, cand_transform, cand_count
    glob = Companion("threecrate_hip_global.h", "ffi_global.rs", {
        # context, src_desc, ns, tgt_desc, nt, dim, match_index, match_dist
        ("tc_match_features", "tc_match_features_device"): (i, [vp, vp, sz, vp, sz, sz, vp, vp]),
        # ..., max_iters, seed, ...
        ("tc_ransac_correspondences", "tc_ransac_correspondences_device"): (i, head + [sz, u64] + tail),
        # ..., samples, n_samples, ...
        ("tc_ransac_correspondences_samples", "tc_ransac_correspondences_samples_device"): (i, head + [vp, sz] + tail),
    }, {"tc_ransac_result": RansacResultC}, "libthreecrate_hip_global.so")
    return [glob]


def _later_companions():
    """Companions that arrived after tests/test_abi_global.py pinned COMPANIONS to exactly the global-registration header: the same kind
    of entry, loaded by the same load_companion(header), each held to the same checks by a test file of its own
    (tests/test_abi_voxelmap.py).  The EXTENSIONS precedent: an entry joins COMPANIONS once that file may be edited."""
    vp, sz, i, u64, szp = C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.POINTER(C.c_size_t)
    voxelmap = Companion("threecrate_hip_voxelmap.h", "ffi_voxelmap.rs", {
        ("tc_voxel_map_create",): (i, [vp, C.POINTER(VoxelMapConfigC), C.POINTER(C.c_void_p)]),
        ("tc_voxel_map_destroy",): (None, [vp]),
        ("tc_voxel_map_reset",): (i, [vp]),
        ("tc_voxel_map_size",): (sz, [vp]),
        ("tc_voxel_map_points",): (u64, [vp]),
        # map, xyz, n
        ("tc_voxel_map_insert", "tc_voxel_map_insert_device"): (i, [vp, vp, sz]),
        # map, keys, counts, sums, centroids, capacity, n_voxels
        ("tc_voxel_map_extract", "tc_voxel_map_extract_device"): (i, [vp, vp, vp, vp, vp, sz, szp]),
    }, {"tc_voxel_map_config": VoxelMapConfigC}, "libthreecrate_hip_voxelmap.so")
    return [voxelmap]


def _further_companions():
    """The open-ended list of further companions: every companion that arrives after tests/test_abi_voxelmap.py pinned LATER_COMPANIONS to
    exactly the voxel-map header goes HERE, the same kind of entry, loaded by the same load_companion(header).  The test file of an entry
    (tests/test_abi_color.py) asserts that its header is a member of this list, not what the list equals: the next companion needs no
    fourth table."""
    vp, sz, i, szp = C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_size_t)
    color = Companion("threecrate_hip_color.h", "ffi_color.rs", {
        ("tc_colorize_config_default",): (None, [C.POINTER(ColorizeConfigC)]),
        # context, xyz, n, sources, n_sources, config, rgb, source_index, colored_count
        ("tc_colorize", "tc_colorize_device"): (i, [vp, vp, sz, C.POINTER(ColorSourceC), sz, C.POINTER(ColorizeConfigC), vp, vp, szp]),
    }, {"tc_color_source": ColorSourceC, "tc_colorize_config": ColorizeConfigC}, "libthreecrate_hip_color.so")
    mesh = Companion("threecrate_hip_mesh.h", "ffi_mesh.rs", {
        ("tc_mesh_smooth_config_default",): (None, [C.c_uint32, C.POINTER(MeshSmoothConfigC)]),
        # context, vertices, n_vertices, faces, n_faces, config, out_vertices
        ("tc_mesh_smooth", "tc_mesh_smooth_device"): (i, [vp, vp, sz, vp, sz, C.POINTER(MeshSmoothConfigC), vp]),
        # context, n_vertices, faces, n_faces, offsets, neighbors, capacity, n_entries
        ("tc_mesh_vertex_adjacency", "tc_mesh_vertex_adjacency_device"): (i, [vp, sz, vp, sz, vp, vp, sz, szp]),
    }, {"tc_mesh_smooth_config": MeshSmoothConfigC}, "libthreecrate_hip_mesh.so")
    simplify = Companion("threecrate_hip_simplify.h", "ffi_simplify.rs", {
        ("tc_simplify_config_default",): (None, [C.c_float, C.POINTER(SimplifyConfigC)]),
        # context, vertices, n_vertices, faces, n_faces, normals, colors, config, out_vertices, out_normals, out_colors, cap_vertices,
        # out_faces, cap_faces, out_vertex_map, n_out_vertices, n_out_faces
        ("tc_simplify_clustering", "tc_simplify_clustering_device"):
            (i, [vp, vp, sz, vp, sz, vp, vp, C.POINTER(SimplifyConfigC), vp, vp, vp, sz, vp, sz, vp, szp, szp]),
    }, {"tc_simplify_config": SimplifyConfigC}, "libthreecrate_hip_simplify.so")
    mc = Companion("threecrate_hip_mc.h", "ffi_mc.rs", {
        ("tc_mc_config_default",): (None, [C.POINTER(McConfigC)]),
        # context, grid, values, valid, config, vertices, normals, faces, vertex_capacity, face_capacity, n_vertices, n_faces
        ("tc_marching_cubes", "tc_marching_cubes_device"): (i, [vp, C.POINTER(McGridC), vp, vp, C.POINTER(McConfigC), vp, vp, vp, sz, sz, szp, szp]),
    }, {"tc_mc_grid": McGridC, "tc_mc_config": McConfigC}, "libthreecrate_hip_mc.so")
    qem = Companion("threecrate_hip_qem.h", "ffi_qem.rs", {
        ("tc_qem_config_default",): (None, [C.c_float, C.POINTER(QemConfigC)]),
        # context, vertices, n_vertices, faces, n_faces, config, out_vertices, cap_vertices, out_faces, cap_faces, out_vertex_map,
        # n_out_vertices, n_out_faces, n_rounds
        ("tc_simplify_quadric", "tc_simplify_quadric_device"):
            (i, [vp, vp, sz, vp, sz, C.POINTER(QemConfigC), vp, sz, vp, sz, vp, szp, szp, C.POINTER(C.c_uint32)]),
    }, {"tc_qem_config": QemConfigC}, "libthreecrate_hip_qem.so")
    alpha = Companion("threecrate_hip_alpha.h", "ffi_alpha.rs", {
        ("tc_alpha_config_default",): (None, [C.c_float, C.POINTER(AlphaConfigC)]),
        # context, points, n, config, out_faces, cap_faces, stats
        ("tc_alpha_shape", "tc_alpha_shape_device"): (i, [vp, vp, sz, C.POINTER(AlphaConfigC), vp, sz, C.POINTER(AlphaStatsC)]),
    }, {"tc_alpha_config": AlphaConfigC, "tc_alpha_stats": AlphaStatsC}, "libthreecrate_hip_alpha.so")
    ground = Companion("threecrate_hip_ground.h", "ffi_ground.rs", {
        ("tc_ground_config_default",): (None, [C.c_float, C.POINTER(GroundConfigC)]),
        ("tc_ground_patch_count",): (sz, [C.POINTER(GroundConfigC)]),
        # context, points, n, config, out_labels, out_ground_index, out_nonground_index, out_patches, n_ground
        ("tc_segment_ground", "tc_segment_ground_device"): (i, [vp, vp, sz, C.POINTER(GroundConfigC), vp, vp, vp, vp, szp]),
    }, {"tc_ground_config": GroundConfigC, "tc_ground_patch": GroundPatchC}, "libthreecrate_hip_ground.so")
    return [color, mesh, simplify, mc, qem, alpha, ground]


def _more_companions():
    """Companions that arrived after tests/test_abi_ground.py counted the libraries of the three tables above (eight beside its own): the
    same kind of entry, loaded by the same load_companion(header), each held to the same checks by a test file of its own
    (tests/test_abi_shot.py), which asserts MEMBERSHIP and counts nothing."""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    shot = Companion("threecrate_hip_shot.h", "ffi_shot.rs", {
        ("tc_shot_config_default",): (None, [C.POINTER(ShotConfigC)]),
        ("tc_shot_dim",): (sz, [i]),
        # context, normal_points, n, config, out, lrf, flags
        ("tc_extract_shot_features_with_normals", "tc_extract_shot_features_with_normals_device"): (i, [vp, vp, sz, C.POINTER(ShotConfigC), vp, vp, vp]),
    }, {"tc_shot_config": ShotConfigC}, "libthreecrate_hip_shot.so")
    poisson = Companion("threecrate_hip_poisson.h", "ffi_poisson.rs", {
        ("tc_poisson_config_default",): (None, [C.POINTER(PoissonConfigC)]),
        # context, points, normals, n, config, grid, chi, density, stats
        ("tc_poisson_field", "tc_poisson_field_device"): (i, [vp, vp, vp, sz, C.POINTER(PoissonConfigC), C.POINTER(McGridC), vp, vp, C.POINTER(PoissonStatsC)]),
        # context, points, normals, n, config, vertices, faces, vertex_capacity, face_capacity, n_vertices, n_faces, stats
        ("tc_poisson_reconstruct", "tc_poisson_reconstruct_device"): (i, [vp, vp, vp, sz, C.POINTER(PoissonConfigC), vp, vp, sz, sz, C.POINTER(sz), C.POINTER(sz),
                                                                          C.POINTER(PoissonStatsC)]),
    }, {"tc_poisson_config": PoissonConfigC, "tc_poisson_stats": PoissonStatsC}, "libthreecrate_hip_poisson.so")
    return [shot, poisson]


def signatures(surface):
    """name -> (restype, argtypes) of every export of one surface, in the order of its rows"""
    return {name: sig for names, sig in surface.rows.items() for name in names}


SURFACES = _surfaces()
# the names of each header, for the callers that want one surface (the symbols all live in the same library)
EXPORTS, FILTER_EXPORTS, SEGMENTATION_EXPORTS, NDT_EXPORTS = (list(signatures(s)) for s in SURFACES)
EXTENSIONS = _extensions()
(TSDF_EXPORTS,) = (list(signatures(s)) for s in EXTENSIONS)
COMPANIONS = _companions()
(GLOBAL_EXPORTS,) = (list(signatures(s)) for s in COMPANIONS)
LATER_COMPANIONS = _later_companions()
(VOXELMAP_EXPORTS,) = (list(signatures(s)) for s in LATER_COMPANIONS)
FURTHER_COMPANIONS = _further_companions()
COLOR_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_color.h")))
TC_COLOR_NEAREST, TC_COLOR_BILINEAR, TC_COLOR_MAX_SOURCES = 0, 1, 64
MESH_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_mesh.h")))
TC_MESH_LAPLACIAN, TC_MESH_TAUBIN, TC_MESH_HC = 0, 1, 2
SIMPLIFY_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_simplify.h")))
TC_SIMPLIFY_CENTROID, TC_SIMPLIFY_WEIGHTED_AVERAGE = 0, 1
MC_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_mc.h")))
TC_MC_Z_FASTEST, TC_MC_X_FASTEST, TC_MC_NORMALS, TC_MC_WELD = 0, 1, 1, 2
QEM_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_qem.h")))
ALPHA_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_alpha.h")))
TC_ALPHA_BOUNDARY_ONLY, TC_ALPHA_FULL, TC_ALPHA_REFERENCE_CAP = 0, 1, 50000
GROUND_EXPORTS = list(signatures(next(s for s in FURTHER_COMPANIONS if s.header == "threecrate_hip_ground.h")))
TC_GROUND_MAX_PATCHES = 65536
TC_GROUND_STATUS = ("EMPTY", "TOO_FEW_POINTS", "TOO_FEW_SEEDS", "TOO_FEW_INLIERS", "NO_ITERATION", "NOT_UPRIGHT", "ELEVATION", "NOT_FLAT", "GROUND")
(TC_GROUND_PATCH_EMPTY, TC_GROUND_PATCH_TOO_FEW_POINTS, TC_GROUND_PATCH_TOO_FEW_SEEDS, TC_GROUND_PATCH_TOO_FEW_INLIERS, TC_GROUND_PATCH_NO_ITERATION,
 TC_GROUND_PATCH_NOT_UPRIGHT, TC_GROUND_PATCH_ELEVATION, TC_GROUND_PATCH_NOT_FLAT, TC_GROUND_PATCH_GROUND) = range(9)
MORE_COMPANIONS = _more_companions()
SHOT_EXPORTS = list(signatures(next(s for s in MORE_COMPANIONS if s.header == "threecrate_hip_shot.h")))
POISSON_EXPORTS = list(signatures(next(s for s in MORE_COMPANIONS if s.header == "threecrate_hip_poisson.h")))
TC_POISSON_MIN_POINTS, TC_POISSON_MIN_DEPTH, TC_POISSON_MAX_DEPTH = 10, 2, 8
TC_SHOT_DIM, TC_USC_DIM, TC_SHOT_VARIANT_SHOT, TC_SHOT_VARIANT_USC = 352, 128, 0, 1
TC_SHOT_ROAD_BALL, TC_SHOT_ROAD_FALLBACK, TC_SHOT_ROAD_INERT, TC_SHOT_ROAD_MASK, TC_SHOT_X_TIE, TC_SHOT_ZERO_COV, TC_SHOT_EMPTY = 0, 1, 2, 3, 4, 8, 16
TC_FPFH_DIM, TC_RANSAC_MAX_ITERS = 33, 1 << 20
TC_VOXEL_MAP_KEY_LIMIT, TC_VOXEL_MAP_MIN_CAPACITY, TC_VOXEL_MAP_DEFAULT_CAPACITY, TC_VOXEL_MAP_MAX_CAPACITY = 1 << 20, 1 << 8, 1 << 16, 1 << 28

_lib = None
_companion_libs = {}


def _preload_hip_runtime():
    """If PyTorch-ROCm is installed it bundles its own libamdhip64.so (SONAME libamdhip64.so.7).
    Two HIP runtimes in one process cannot both open the GPU, so bind to torch's copy first:
    our NEEDED libamdhip64.so.7 then resolves to it and torch tensors / streams can be handed
    across the C ABI.  Without torch the system ROCm runtime (/opt/rocm/lib) is used."""
    if os.environ.get("TC_NO_TORCH_PRELOAD"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load the HIP library; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  threecrate_amd has no CPU fallback.")
    _preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    for surface in SURFACES + EXTENSIONS:
        for name, (restype, argtypes) in signatures(surface).items():
            fn = getattr(L, name)
            fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
    _lib = L
    return L


def load_companion(header, variant=None):
    """The companion library of `header` (an entry of COMPANIONS, LATER_COMPANIONS, FURTHER_COMPANIONS or MORE_COMPANIONS): the product library first, then the companion, which binds it by
    name from its own directory; signatures from the table.  A companion always binds the PRODUCT library: with TC_HIP_LIB pointing at
    another build the two would be two copies of the host layer in one process, so this raises instead."""
    if header in _companion_libs:
        return _companion_libs[header]
    (surface,) = [s for s in COMPANIONS + LATER_COMPANIONS + FURTHER_COMPANIONS + MORE_COMPANIONS if s.header == header]
    product = os.path.join(_HERE, "libthreecrate_hip.so")
    if os.path.realpath(LIB_PATH) != os.path.realpath(product):
        raise ImportError(f"{surface.library} is linked against {product}; it cannot be used with TC_HIP_LIB={LIB_PATH}")
    # variant: an A/B build of the companion under variants/ (csrc/Makefile: mesh-ab), for the process's first load of this header only
    path = os.path.join(_HERE, "variants", variant) if variant else os.path.join(_HERE, surface.library)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  threecrate_amd has no CPU fallback.")
    load()
    L = C.CDLL(path)
    for name, (restype, argtypes) in signatures(surface).items():
        fn = getattr(L, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _companion_libs[header] = L
    return L
