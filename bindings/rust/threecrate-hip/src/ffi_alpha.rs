//! Raw declarations of include/threecrate_hip_alpha.h: alpha-shape surface reconstruction, a point cloud to triangles.
//! The symbols live in the eighth companion library, libthreecrate_hip_alpha.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_alpha.py checks names, parameter counts and types
//! against the header and the structs against the compiled layouts.
use crate::ffi::tc_context;
use std::os::raw::c_int;

pub const TC_ALPHA_BOUNDARY_ONLY: u32 = 0;
pub const TC_ALPHA_FULL: u32 = 1;

/// `tc_alpha_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_alpha_config {
    pub alpha: f32,
    pub mode: u32,
    pub min_triangle_area: f32,
    pub max_triangles: u32,
}

/// `tc_alpha_stats`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_alpha_stats {
    pub candidates: u64,
    pub boundary_candidates: u64,
    pub faces: u64,
    pub capped: u32,
}

extern "C" {
    pub fn tc_alpha_config_default(alpha: f32, cfg: *mut tc_alpha_config);
    pub fn tc_alpha_shape(ctx: *mut tc_context, points: *const f32, n: usize, cfg: *const tc_alpha_config, out_faces: *mut u32, cap_faces: usize,
                          stats: *mut tc_alpha_stats) -> c_int;
    pub fn tc_alpha_shape_device(ctx: *mut tc_context, points: *const f32, n: usize, cfg: *const tc_alpha_config, out_faces: *mut u32,
                                 cap_faces: usize, stats: *mut tc_alpha_stats) -> c_int;
}
