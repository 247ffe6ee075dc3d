//! Raw declarations of include/threecrate_hip_mesh.h: Laplacian, Taubin and HC smoothing of a triangle mesh and its one-ring adjacency.
//! The symbols live in the fourth companion library, libthreecrate_hip_mesh.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_mesh.py checks names, parameter counts and types
//! against the header and the struct against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_mesh_smooth_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_mesh_smooth_config {
    pub method: u32,
    pub iterations: u32,
    pub lambda: f32,
    pub mu: f32,
    pub alpha: f32,
    pub beta: f32,
}

pub const TC_MESH_LAPLACIAN: u32 = 0;
pub const TC_MESH_TAUBIN: u32 = 1;
pub const TC_MESH_HC: u32 = 2;

extern "C" {
    pub fn tc_mesh_smooth_config_default(method: u32, cfg: *mut tc_mesh_smooth_config);
    pub fn tc_mesh_smooth(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                          cfg: *const tc_mesh_smooth_config, out_vertices: *mut f32) -> c_int;
    pub fn tc_mesh_smooth_device(ctx: *mut tc_context, vertices: *const f32, n_vertices: usize, faces: *const u32, n_faces: usize,
                                 cfg: *const tc_mesh_smooth_config, out_vertices: *mut f32) -> c_int;
    pub fn tc_mesh_vertex_adjacency(ctx: *mut tc_context, n_vertices: usize, faces: *const u32, n_faces: usize, offsets: *mut u32,
                                    neighbors: *mut u32, capacity: usize, n_entries: *mut usize) -> c_int;
    pub fn tc_mesh_vertex_adjacency_device(ctx: *mut tc_context, n_vertices: usize, faces: *const u32, n_faces: usize, offsets: *mut u32,
                                           neighbors: *mut u32, capacity: usize, n_entries: *mut usize) -> c_int;
}
