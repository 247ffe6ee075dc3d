//! Raw declarations of include/threecrate_hip_global.h: descriptor matching and RANSAC over correspondences, the two device steps of
//! global registration.  The symbols live in the companion library libthreecrate_hip_global.so (build.rs links it beside
//! libthreecrate_hip.so), with the status and context types of ffi.rs.  tests/test_abi_global.py checks names, parameter counts, types
//! and the struct's layout against the header.
use crate::ffi::tc_context;
use std::os::raw::c_int;

pub const TC_RANSAC_MAX_ITERS: usize = 1 << 20;

#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_ransac_result {
    pub inlier_count: u64,
    pub iterations_run: u64,
    pub best_iteration: u32,
    pub early_exit: i32,
    pub inlier_ratio: f32,
}

extern "C" {
    pub fn tc_match_features(ctx: *mut tc_context, src_desc: *const f32, ns: usize, tgt_desc: *const f32, nt: usize, dim: usize,
                             match_index: *mut u32, match_dist: *mut f32) -> c_int;
    pub fn tc_match_features_device(ctx: *mut tc_context, d_src_desc: *const f32, ns: usize, d_tgt_desc: *const f32, nt: usize, dim: usize,
                                    d_match_index: *mut u32, d_match_dist: *mut f32) -> c_int;
    pub fn tc_ransac_correspondences(ctx: *mut tc_context, src_xyz: *const f32, ns: usize, tgt_xyz: *const f32, nt: usize,
                                     corr_src: *const u32, corr_tgt: *const u32, m: usize, threshold: f32, inlier_ratio: f32,
                                     max_iters: usize, seed: u64, transform: *mut f32, result: *mut tc_ransac_result,
                                     cand_transform: *mut f32, cand_count: *mut u32) -> c_int;
    pub fn tc_ransac_correspondences_device(ctx: *mut tc_context, d_src_xyz: *const f32, ns: usize, d_tgt_xyz: *const f32, nt: usize,
                                            d_corr_src: *const u32, d_corr_tgt: *const u32, m: usize, threshold: f32, inlier_ratio: f32,
                                            max_iters: usize, seed: u64, transform: *mut f32, result: *mut tc_ransac_result,
                                            d_cand_transform: *mut f32, d_cand_count: *mut u32) -> c_int;
    pub fn tc_ransac_correspondences_samples(ctx: *mut tc_context, src_xyz: *const f32, ns: usize, tgt_xyz: *const f32, nt: usize,
                                             corr_src: *const u32, corr_tgt: *const u32, m: usize, threshold: f32, inlier_ratio: f32,
                                             samples: *const u32, n_samples: usize, transform: *mut f32, result: *mut tc_ransac_result,
                                             cand_transform: *mut f32, cand_count: *mut u32) -> c_int;
    pub fn tc_ransac_correspondences_samples_device(ctx: *mut tc_context, d_src_xyz: *const f32, ns: usize, d_tgt_xyz: *const f32, nt: usize,
                                                    d_corr_src: *const u32, d_corr_tgt: *const u32, m: usize, threshold: f32,
                                                    inlier_ratio: f32, d_samples: *const u32, n_samples: usize, transform: *mut f32,
                                                    result: *mut tc_ransac_result, d_cand_transform: *mut f32, d_cand_count: *mut u32) -> c_int;
}
