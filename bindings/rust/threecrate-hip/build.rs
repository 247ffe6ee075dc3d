// Link against libthreecrate_hip.so and its companion libthreecrate_hip_global.so (ffi_global.rs), which lives in the same directory.  THREECRATE_HIP_LIB_DIR points at the directory that holds it
// (built with `make -C threecrate_amd/csrc`); ROCm's libamdhip64 is found through the .so's own NEEDED entry.
fn main() {
    if let Ok(dir) = std::env::var("THREECRATE_HIP_LIB_DIR") {
        println!("cargo:rustc-link-search=native={dir}");
        println!("cargo:rustc-link-arg=-Wl,-rpath,{dir}");
    }
    println!("cargo:rustc-link-lib=dylib=threecrate_hip");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_global");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_voxelmap");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_color");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_mesh");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_simplify");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_qem");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_alpha");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_ground");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_shot");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_poisson");
    println!("cargo:rustc-link-lib=dylib=threecrate_hip_mc");
    println!("cargo:rerun-if-env-changed=THREECRATE_HIP_LIB_DIR");
}
