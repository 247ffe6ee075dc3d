//! Raw declarations of include/threecrate_hip_color.h: colour a point cloud from registered camera images.
//! The symbols live in the third companion library, libthreecrate_hip_color.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs; tc_camera_intrinsics is ffi_tsdf.rs's); build.rs links both.  tests/test_abi_color.py checks
//! names, parameter counts and types against the header and the structs against the compiled layout.
use crate::ffi::tc_context;
use crate::ffi_tsdf::tc_camera_intrinsics;
use std::os::raw::c_int;

/// `tc_color_source`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_color_source {
    pub rgb: *const u8,
    pub depth: *const f32,
    pub intrinsics: tc_camera_intrinsics,
    pub world_to_camera: [f32; 12],
}

/// `tc_colorize_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_colorize_config {
    pub default_color: [u8; 3],
    pub interpolation: u8,
    pub min_depth: f32,
    pub depth_tolerance: f32,
}

pub const TC_COLOR_NEAREST: u8 = 0;
pub const TC_COLOR_BILINEAR: u8 = 1;
pub const TC_COLOR_MAX_SOURCES: usize = 64;

extern "C" {
    pub fn tc_colorize_config_default(cfg: *mut tc_colorize_config);
    pub fn tc_colorize(ctx: *mut tc_context, xyz: *const f32, n: usize, sources: *const tc_color_source, n_sources: usize,
                       cfg: *const tc_colorize_config, rgb: *mut u8, source_index: *mut i32, colored_count: *mut usize) -> c_int;
    pub fn tc_colorize_device(ctx: *mut tc_context, xyz: *const f32, n: usize, sources: *const tc_color_source, n_sources: usize,
                              cfg: *const tc_colorize_config, rgb: *mut u8, source_index: *mut i32, colored_count: *mut usize) -> c_int;
}
