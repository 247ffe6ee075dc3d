//! Raw declarations of include/threecrate_hip_simplify.h: vertex-clustering simplification of a triangle mesh.
//! The symbols live in the fifth companion library, libthreecrate_hip_simplify.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_simplify.py checks names, parameter counts and types
//! against the header and the struct against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_simplify_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_simplify_config {
    pub strategy: u32,
    pub preserve_boundary: u32,
    pub feature_angle_threshold: f32,
    pub reduction_ratio: f32,
}

pub const TC_SIMPLIFY_CENTROID: u32 = 0;
pub const TC_SIMPLIFY_WEIGHTED_AVERAGE: u32 = 1;

extern "C" {
    pub fn tc_simplify_config_default(reduction_ratio: f32, cfg: *mut tc_simplify_config);
    pub fn tc_simplify_clustering(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                                  normals: *const f32, colors: *const u8, cfg: *const tc_simplify_config, out_vertices: *mut f32,
                                  out_normals: *mut f32, out_colors: *mut u8, cap_vertices: usize, out_faces: *mut u32, cap_faces: usize,
                                  out_vertex_map: *mut u32, n_out_vertices: *mut usize, n_out_faces: *mut usize) -> c_int;
    pub fn tc_simplify_clustering_device(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                                         normals: *const f32, colors: *const u8, cfg: *const tc_simplify_config, out_vertices: *mut f32,
                                         out_normals: *mut f32, out_colors: *mut u8, cap_vertices: usize, out_faces: *mut u32,
                                         cap_faces: usize, out_vertex_map: *mut u32, n_out_vertices: *mut usize, n_out_faces: *mut usize) -> c_int;
}
