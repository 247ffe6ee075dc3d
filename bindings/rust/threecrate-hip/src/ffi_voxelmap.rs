//! Raw declarations of include/threecrate_hip_voxelmap.h: a voxel map that lives on the device across the chunks of a point stream.
//! The symbols live in the second companion library, libthreecrate_hip_voxelmap.so, which is linked against libthreecrate_hip.so
//! (same status and context types as ffi.rs); build.rs links both.  tests/test_abi_voxelmap.py checks names, parameter counts and
//! types against the header and the struct against the compiled layout.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_voxel_map`: opaque
#[repr(C)]
pub struct tc_voxel_map {
    _private: [u8; 0],
}

/// `tc_voxel_map_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_voxel_map_config {
    pub voxel_size: f32,
    pub initial_capacity: usize,
}

pub const TC_VOXEL_MAP_KEY_LIMIT: i32 = 1 << 20;
pub const TC_VOXEL_MAP_MIN_CAPACITY: usize = 1 << 8;
pub const TC_VOXEL_MAP_DEFAULT_CAPACITY: usize = 1 << 16;
pub const TC_VOXEL_MAP_MAX_CAPACITY: usize = 1 << 28;

extern "C" {
    pub fn tc_voxel_map_create(ctx: *mut tc_context, config: *const tc_voxel_map_config, out: *mut *mut tc_voxel_map) -> c_int;
    pub fn tc_voxel_map_destroy(map: *mut tc_voxel_map);
    pub fn tc_voxel_map_reset(map: *mut tc_voxel_map) -> c_int;
    pub fn tc_voxel_map_size(map: *mut tc_voxel_map) -> usize;
    pub fn tc_voxel_map_points(map: *mut tc_voxel_map) -> u64;
    pub fn tc_voxel_map_insert(map: *mut tc_voxel_map, xyz: *const f32, n: usize) -> c_int;
    pub fn tc_voxel_map_insert_device(map: *mut tc_voxel_map, d_xyz: *const f32, n: usize) -> c_int;
    pub fn tc_voxel_map_extract(map: *mut tc_voxel_map, keys: *mut i32, counts: *mut u32, sums: *mut f64, centroids: *mut f32, capacity: usize,
                                n_voxels: *mut usize) -> c_int;
    pub fn tc_voxel_map_extract_device(map: *mut tc_voxel_map, d_keys: *mut i32, d_counts: *mut u32, d_sums: *mut f64, d_centroids: *mut f32,
                                       capacity: usize, n_voxels: *mut usize) -> c_int;
}
