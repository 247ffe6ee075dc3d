//! Raw declarations of include/threecrate_hip_mc.h: marching cubes, a scalar grid or a TSDF volume's arrays to a triangle mesh.
//! The symbols live in the sixth companion library, libthreecrate_hip_mc.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_mc.py checks names, parameter counts and types
//! against the header and the structs against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_mc_grid`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_mc_grid {
    pub dims: [u32; 3],
    pub voxel_size: [f32; 3],
    pub origin: [f32; 3],
    pub layout: u32,
}

/// `tc_mc_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_mc_config {
    pub iso_level: f32,
    pub flags: u32,
}

pub const TC_MC_Z_FASTEST: u32 = 0;
pub const TC_MC_X_FASTEST: u32 = 1;
pub const TC_MC_NORMALS: u32 = 1;
pub const TC_MC_WELD: u32 = 2;

extern "C" {
    pub fn tc_mc_config_default(cfg: *mut tc_mc_config);
    pub fn tc_marching_cubes(ctx: *mut tc_context, grid: *const tc_mc_grid, values: *const f32, valid: *const u8, cfg: *const tc_mc_config,
                             vertices: *mut f32, normals: *mut f32, faces: *mut u32, vertex_capacity: usize, face_capacity: usize,
                             n_vertices: *mut usize, n_faces: *mut usize) -> c_int;
    pub fn tc_marching_cubes_device(ctx: *mut tc_context, grid: *const tc_mc_grid, values: *const f32, valid: *const u8, cfg: *const tc_mc_config,
                                    vertices: *mut f32, normals: *mut f32, faces: *mut u32, vertex_capacity: usize, face_capacity: usize,
                                    n_vertices: *mut usize, n_faces: *mut usize) -> c_int;
}
