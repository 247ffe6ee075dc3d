//! Raw declarations of include/threecrate_hip_poisson.h: Poisson surface reconstruction on a dense grid.
//! The symbols live in the eleventh companion library, libthreecrate_hip_poisson.so, which is linked against libthreecrate_hip.so and
//! libthreecrate_hip_mc.so (same status and context types as ffi.rs, the grid of ffi_mc.rs); build.rs links them.
//! tests/test_abi_poisson.py checks names, parameter counts and types against the header and the structs against the compiled layout.
use crate::ffi::tc_context;
use crate::ffi_mc::tc_mc_grid;
use std::os::raw::c_int;

pub const TC_POISSON_MIN_POINTS: usize = 10;
pub const TC_POISSON_MIN_DEPTH: u32 = 2;
pub const TC_POISSON_MAX_DEPTH: u32 = 8;

/// `tc_poisson_config`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_poisson_config {
    pub depth: u32,
    pub scale: f32,
    pub point_weight: f32,
    pub max_iterations: u32,
    pub tolerance: f32,
    pub min_density: f32,
}

/// `tc_poisson_stats`
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct tc_poisson_stats {
    pub iterations: u32,
    pub rel_residual: f32,
    pub iso_value: f32,
    pub occupied_nodes: u32,
}

extern "C" {
    pub fn tc_poisson_config_default(cfg: *mut tc_poisson_config);
    pub fn tc_poisson_field(ctx: *mut tc_context, points: *const f32, normals: *const f32, n: usize, cfg: *const tc_poisson_config, grid: *mut tc_mc_grid,
                            chi: *mut f32, density: *mut f32, stats: *mut tc_poisson_stats) -> c_int;
    pub fn tc_poisson_field_device(ctx: *mut tc_context, points: *const f32, normals: *const f32, n: usize, cfg: *const tc_poisson_config,
                                   grid: *mut tc_mc_grid, chi: *mut f32, density: *mut f32, stats: *mut tc_poisson_stats) -> c_int;
    pub fn tc_poisson_reconstruct(ctx: *mut tc_context, points: *const f32, normals: *const f32, n: usize, cfg: *const tc_poisson_config,
                                  vertices: *mut f32, faces: *mut u32, vertex_capacity: usize, face_capacity: usize, n_vertices: *mut usize,
                                  n_faces: *mut usize, stats: *mut tc_poisson_stats) -> c_int;
    pub fn tc_poisson_reconstruct_device(ctx: *mut tc_context, points: *const f32, normals: *const f32, n: usize, cfg: *const tc_poisson_config,
                                         vertices: *mut f32, faces: *mut u32, vertex_capacity: usize, face_capacity: usize, n_vertices: *mut usize,
                                         n_faces: *mut usize, stats: *mut tc_poisson_stats) -> c_int;
}
