//! Raw declarations of include/threecrate_hip_qem.h: quadric-error simplification of a triangle mesh, in rounds.
//! The symbols live in the seventh companion library, libthreecrate_hip_qem.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_qem.py checks names, parameter counts and types
//! against the header and the struct against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_qem_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_qem_config {
    pub reduction_ratio: f32,
    pub preserve_boundary: u32,
    pub max_edge_length: f32,
}

extern "C" {
    pub fn tc_qem_config_default(reduction_ratio: f32, cfg: *mut tc_qem_config);
    pub fn tc_simplify_quadric(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                               cfg: *const tc_qem_config, out_vertices: *mut f32, cap_vertices: usize, out_faces: *mut u32, cap_faces: usize,
                               out_vertex_map: *mut u32, n_out_vertices: *mut usize, n_out_faces: *mut usize, n_rounds: *mut u32) -> c_int;
    pub fn tc_simplify_quadric_device(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                                      cfg: *const tc_qem_config, out_vertices: *mut f32, cap_vertices: usize, out_faces: *mut u32,
                                      cap_faces: usize, out_vertex_map: *mut u32, n_out_vertices: *mut usize, n_out_faces: *mut usize,
                                      n_rounds: *mut u32) -> c_int;
}
