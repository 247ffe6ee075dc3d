//! Raw declarations of include/threecrate_hip_shot.h: SHOT and USC descriptors with their local reference frame.
//! The symbols live in the tenth companion library, libthreecrate_hip_shot.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_shot.py checks names, parameter counts and types
//! against the header and the struct against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

pub const TC_SHOT_DIM: usize = 352;
pub const TC_USC_DIM: usize = 128;
pub const TC_SHOT_VARIANT_SHOT: c_int = 0;
pub const TC_SHOT_VARIANT_USC: c_int = 1;
pub const TC_SHOT_ROAD_BALL: u32 = 0;
pub const TC_SHOT_ROAD_FALLBACK: u32 = 1;
pub const TC_SHOT_ROAD_INERT: u32 = 2;
pub const TC_SHOT_ROAD_MASK: u32 = 3;
pub const TC_SHOT_X_TIE: u32 = 4;
pub const TC_SHOT_ZERO_COV: u32 = 8;
pub const TC_SHOT_EMPTY: u32 = 16;

/// `tc_shot_config`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_shot_config {
    pub search_radius: f32,
    pub k_neighbors: usize,
    pub variant: c_int,
}

extern "C" {
    pub fn tc_shot_config_default(cfg: *mut tc_shot_config);
    pub fn tc_shot_dim(variant: c_int) -> usize;
    pub fn tc_extract_shot_features_with_normals(ctx: *mut tc_context, normal_points: *const f32, n: usize, cfg: *const tc_shot_config, out: *mut f32,
                                                 lrf: *mut f32, flags: *mut u32) -> c_int;
    pub fn tc_extract_shot_features_with_normals_device(ctx: *mut tc_context, normal_points: *const f32, n: usize, cfg: *const tc_shot_config,
                                                        out: *mut f32, lrf: *mut f32, flags: *mut u32) -> c_int;
}
