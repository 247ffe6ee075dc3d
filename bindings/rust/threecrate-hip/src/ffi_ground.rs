//! Raw declarations of include/threecrate_hip_ground.h: ground segmentation of a LiDAR frame, Patchwork++ patches.
//! The symbols live in the ninth companion library, libthreecrate_hip_ground.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_ground.py checks names, parameter counts and types
//! against the header and the structs against the compiled layouts.
use crate::ffi::tc_context;
use std::os::raw::c_int;

pub const TC_GROUND_MAX_ZONES: usize = 8;
pub const TC_GROUND_PATCH_EMPTY: u32 = 0;
pub const TC_GROUND_PATCH_TOO_FEW_POINTS: u32 = 1;
pub const TC_GROUND_PATCH_TOO_FEW_SEEDS: u32 = 2;
pub const TC_GROUND_PATCH_TOO_FEW_INLIERS: u32 = 3;
pub const TC_GROUND_PATCH_NO_ITERATION: u32 = 4;
pub const TC_GROUND_PATCH_NOT_UPRIGHT: u32 = 5;
pub const TC_GROUND_PATCH_ELEVATION: u32 = 6;
pub const TC_GROUND_PATCH_NOT_FLAT: u32 = 7;
pub const TC_GROUND_PATCH_GROUND: u32 = 8;

/// `tc_ground_config`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_ground_config {
    pub sensor_height: f32,
    pub n_zones: u32,
    pub zone_radii: [f32; 9],
    pub num_rings: [u32; 8],
    pub num_sectors: [u32; 8],
    pub max_range: f32,
    pub min_points_per_patch: u32,
    pub num_seed_points: u32,
    pub seed_selection_threshold: f32,
    pub dist_threshold: f32,
    pub num_iterations: u32,
    pub uprightness_threshold: f32,
    pub flatness_threshold: f32,
    pub elevation_threshold: f32,
}

/// `tc_ground_patch`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_ground_patch {
    pub count: u32,
    pub n_inliers: u32,
    pub status: u32,
    pub normal: [f32; 3],
    pub d: f32,
    pub mean_z: f32,
    pub flatness: f32,
}

extern "C" {
    pub fn tc_ground_config_default(sensor_height: f32, cfg: *mut tc_ground_config);
    pub fn tc_ground_patch_count(cfg: *const tc_ground_config) -> usize;
    pub fn tc_segment_ground(ctx: *mut tc_context, points: *const f32, n: usize, cfg: *const tc_ground_config, out_labels: *mut u8,
                             out_ground_index: *mut u32, out_nonground_index: *mut u32, out_patches: *mut tc_ground_patch, n_ground: *mut usize) -> c_int;
    pub fn tc_segment_ground_device(ctx: *mut tc_context, points: *const f32, n: usize, cfg: *const tc_ground_config, out_labels: *mut u8,
                                    out_ground_index: *mut u32, out_nonground_index: *mut u32, out_patches: *mut tc_ground_patch,
                                    n_ground: *mut usize) -> c_int;
}
