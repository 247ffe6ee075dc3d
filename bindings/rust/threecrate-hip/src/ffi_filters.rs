//! Raw declarations of include/threecrate_hip_filters.h: the extension surface of libthreecrate_hip.so (same library, same
//! status and context types as ffi.rs).  tests/test_abi_surfaces.py checks names, parameter counts and types against the header.
use crate::ffi::tc_context;
use std::os::raw::c_int;

extern "C" {
    pub fn tc_statistical_outlier_removal(ctx: *mut tc_context, xyz: *const f32, n: usize, k_neighbors: usize, std_dev_multiplier: f32,
                                          out_xyz: *mut f32, kept_index: *mut u32, mean_distance: *mut f32, n_out: *mut usize,
                                          threshold_used: *mut f32) -> c_int;
    pub fn tc_statistical_outlier_removal_device(ctx: *mut tc_context, d_xyz: *const f32, n: usize, k_neighbors: usize, std_dev_multiplier: f32,
                                                 d_out_xyz: *mut f32, d_kept_index: *mut u32, d_mean_distance: *mut f32, n_out: *mut usize,
                                                 threshold_used: *mut f32) -> c_int;
    pub fn tc_statistical_outlier_removal_with_threshold(ctx: *mut tc_context, xyz: *const f32, n: usize, k_neighbors: usize, threshold: f32,
                                                         out_xyz: *mut f32, kept_index: *mut u32, mean_distance: *mut f32,
                                                         n_out: *mut usize) -> c_int;
    pub fn tc_statistical_outlier_removal_with_threshold_device(ctx: *mut tc_context, d_xyz: *const f32, n: usize, k_neighbors: usize,
                                                                threshold: f32, d_out_xyz: *mut f32, d_kept_index: *mut u32,
                                                                d_mean_distance: *mut f32, n_out: *mut usize) -> c_int;
    pub fn tc_radius_outlier_removal(ctx: *mut tc_context, xyz: *const f32, n: usize, radius: f32, min_neighbors: usize, out_xyz: *mut f32,
                                     kept_index: *mut u32, n_out: *mut usize) -> c_int;
    pub fn tc_radius_outlier_removal_device(ctx: *mut tc_context, d_xyz: *const f32, n: usize, radius: f32, min_neighbors: usize,
                                            d_out_xyz: *mut f32, d_kept_index: *mut u32, n_out: *mut usize) -> c_int;
}
