//! Raw declarations of include/threecrate_hip_tsdf.h: TSDF depth fusion and surface extraction on a device-resident volume, the fourth
//! extension surface of libthreecrate_hip.so (same library, same status and context types as ffi.rs).  tests/test_abi_tsdf.py checks
//! names, parameter counts and types against the header and the structs against the compiled layouts.
use crate::ffi::tc_context;
use std::os::raw::c_int;

/// `tc_tsdf_volume`: opaque
#[repr(C)]
pub struct tc_tsdf_volume {
    _private: [u8; 0],
}

/// `tc_tsdf_volume_config`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_tsdf_volume_config {
    pub voxel_size: f32,
    pub truncation_distance: f32,
    pub resolution: [u32; 3],
    pub origin: [f32; 3],
    pub max_weight: u32,
}

/// `tc_camera_intrinsics`
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct tc_camera_intrinsics {
    pub fx: f32,
    pub fy: f32,
    pub cx: f32,
    pub cy: f32,
    pub width: u32,
    pub height: u32,
}

pub const TC_TSDF_OBSERVED_EDGES: u32 = 1;

extern "C" {
    pub fn tc_tsdf_volume_create(ctx: *mut tc_context, cfg: *const tc_tsdf_volume_config, out: *mut *mut tc_tsdf_volume) -> c_int;
    pub fn tc_tsdf_volume_destroy(vol: *mut tc_tsdf_volume);
    pub fn tc_tsdf_volume_reset(vol: *mut tc_tsdf_volume) -> c_int;
    pub fn tc_tsdf_integrate(vol: *mut tc_tsdf_volume, depth: *const f32, rgb: *const u8, intrinsics: *const tc_camera_intrinsics,
                             world_to_camera: *const f32, n_updated: *mut usize) -> c_int;
    pub fn tc_tsdf_integrate_device(vol: *mut tc_tsdf_volume, d_depth: *const f32, d_rgb: *const u8, intrinsics: *const tc_camera_intrinsics,
                                    world_to_camera: *const f32, n_updated: *mut usize) -> c_int;
    pub fn tc_tsdf_volume_download(vol: *mut tc_tsdf_volume, tsdf: *mut f32, weight: *mut u8, rgb: *mut u8) -> c_int;
    pub fn tc_tsdf_volume_download_device(vol: *mut tc_tsdf_volume, d_tsdf: *mut f32, d_weight: *mut u8, d_rgb: *mut u8) -> c_int;
    pub fn tc_tsdf_volume_upload(vol: *mut tc_tsdf_volume, tsdf: *const f32, weight: *const u8, rgb: *const u8) -> c_int;
    pub fn tc_tsdf_volume_upload_device(vol: *mut tc_tsdf_volume, d_tsdf: *const f32, d_weight: *const u8, d_rgb: *const u8) -> c_int;
    pub fn tc_tsdf_extract_surface(vol: *mut tc_tsdf_volume, iso_value: f32, flags: u32, xyz: *mut f32, rgb: *mut u8, capacity: usize,
                                   n_points: *mut usize) -> c_int;
    pub fn tc_tsdf_extract_surface_device(vol: *mut tc_tsdf_volume, iso_value: f32, flags: u32, d_xyz: *mut f32, d_rgb: *mut u8,
                                          capacity: usize, n_points: *mut usize) -> c_int;
}
