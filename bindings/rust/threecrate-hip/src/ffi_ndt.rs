//! Raw declarations of include/threecrate_hip_ndt.h: NDT registration and its voxel map, the third extension surface of
//! libthreecrate_hip.so (same library, same status and context types as ffi.rs).  tests/test_abi_surfaces.py checks names,
//! parameter counts and types against the header, tests/test_abi_conformance.py the structs against the compiled layouts.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_ndt_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_ndt_config {
    pub resolution: f32,
    pub step_size: f32,
    pub max_iterations: usize,
    pub epsilon: f32,
    pub min_points_per_voxel: usize,
}

/// `tc_ndt_result`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_ndt_result {
    pub transformation: [f32; 7],
    pub score: f32,
    pub iterations: usize,
    pub converged: c_int,
    pub n_voxels: usize,
    pub n_hits: usize,
}

extern "C" {
    pub fn tc_ndt_registration(ctx: *mut tc_context, source: *const f32, ns: usize, target: *const f32, nt: usize, init: *const f32,
                               cfg: *const tc_ndt_config, result: *mut tc_ndt_result) -> c_int;
    pub fn tc_ndt_registration_device(ctx: *mut tc_context, d_source: *const f32, ns: usize, d_target: *const f32, nt: usize,
                                      init: *const f32, cfg: *const tc_ndt_config, result: *mut tc_ndt_result) -> c_int;
    pub fn tc_ndt_voxels(ctx: *mut tc_context, target: *const f32, nt: usize, resolution: f32, min_points_per_voxel: usize,
                         keys: *mut i32, counts: *mut u32, mean: *mut f32, inv_cov: *mut f32, capacity: usize,
                         n_voxels: *mut usize) -> c_int;
    pub fn tc_ndt_voxels_device(ctx: *mut tc_context, d_target: *const f32, nt: usize, resolution: f32, min_points_per_voxel: usize,
                                d_keys: *mut i32, d_counts: *mut u32, d_mean: *mut f32, d_inv_cov: *mut f32, capacity: usize,
                                n_voxels: *mut usize) -> c_int;
}
