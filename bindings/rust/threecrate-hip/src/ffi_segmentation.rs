//! Raw declarations of include/threecrate_hip_segmentation.h: RANSAC plane segmentation, the second extension surface of
//! libthreecrate_hip.so (same library, same status and context types as ffi.rs).  tests/test_abi_surfaces.py checks names,
//! parameter counts and types against the header.
use crate::ffi::tc_context;
use std::os::raw::c_int;

extern "C" {
    pub fn tc_segment_plane(ctx: *mut tc_context, xyz: *const f32, n: usize, threshold: f32, max_iters: usize, seed: u64,
                            coefficients: *mut f32, inlier_index: *mut u32, n_inliers: *mut usize, best_iteration: *mut u32) -> c_int;
    pub fn tc_segment_plane_device(ctx: *mut tc_context, d_xyz: *const f32, n: usize, threshold: f32, max_iters: usize, seed: u64,
                                   coefficients: *mut f32, d_inlier_index: *mut u32, n_inliers: *mut usize,
                                   best_iteration: *mut u32) -> c_int;
    pub fn tc_segment_plane_samples(ctx: *mut tc_context, xyz: *const f32, n: usize, threshold: f32, samples: *const u32,
                                    n_samples: usize, coefficients: *mut f32, inlier_index: *mut u32, n_inliers: *mut usize,
                                    best_iteration: *mut u32) -> c_int;
    pub fn tc_segment_plane_samples_device(ctx: *mut tc_context, d_xyz: *const f32, n: usize, threshold: f32, d_samples: *const u32,
                                           n_samples: usize, coefficients: *mut f32, d_inlier_index: *mut u32, n_inliers: *mut usize,
                                           best_iteration: *mut u32) -> c_int;
}
