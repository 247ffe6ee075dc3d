"""A COMPILED consumer of every header of include/ (VERDICT r2 next #8): tests/abi/abi_conformance.c is built with gcc -std=c11
and again as C++ (-Wall -Wextra -Werror), linked against libthreecrate_hip.so.

  CPU:  the struct layouts (sizeof / offsetof) and constants the compiler derives from the header must equal the hand-written
        ctypes mirror (threecrate_amd/_lib.py) and the #[repr(C)] structs of the Rust shim (bindings/rust, uncompiled: no Rust
        toolchain in this image -- its layouts are computed here with the C layout rules).
  GPU:  the program runs the reference's call shapes through the HOST entry points (tc_estimate_normals,
        tc_icp_point_to_plane_detailed, tc_icp_detailed, tc_icp) on the 10 k-point golden case and its raw output is compared
        with the golden fixtures (tests/golden/) and with the ctypes path, bit for bit.
"""
import ctypes as C
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from threecrate_amd import _lib, synth
from tests.abi_text import RUST_DIR, header_decls, rust_decls, rust_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "abi", "abi_conformance.c")
LIBDIR = os.path.join(ROOT, "threecrate_amd")

MIRROR = {name: cls for surface in _lib.SURFACES for name, cls in surface.structs.items()}


def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


def _layout(exe):
    out = subprocess.check_output([exe, "layout"], text=True)
    return {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi"))
    return {lang: _build(tmp, lang) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_on_the_header(exes):
    assert _layout(exes["c"]) == _layout(exes["cpp"])


def test_compiled_layouts_equal_the_ctypes_mirror(exes):
    lay = _layout(exes["c"])
    seen = set()
    for name, cls in MIRROR.items():
        assert lay[f"sizeof.{name}"] == C.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert lay[f"offsetof.{name}.{fname}"] == getattr(cls, fname).offset, (name, fname)
            assert lay[f"fieldsize.{name}.{fname}"] == getattr(cls, fname).size, (name, fname)
            seen.add(f"offsetof.{name}.{fname}")
    # every field the headers declare is mirrored (no field missing on the Python side)
    assert {k for k in lay if k.startswith("offsetof.")} == seen
    assert lay["sizeof.tc_ndt_config"] == C.sizeof(_lib.NdtConfigC) == 32 and lay["sizeof.tc_ndt_result"] == C.sizeof(_lib.NdtResultC) == 64
    for cname, val in (("TC_OK", _lib.TC_OK), ("TC_INVALID_DATA", _lib.TC_INVALID_DATA), ("TC_ALGORITHM", _lib.TC_ALGORITHM),
                       ("TC_GPU", _lib.TC_GPU), ("TC_UNSUPPORTED", _lib.TC_UNSUPPORTED), ("TC_COMM_ID_BYTES", _lib.TC_COMM_ID_BYTES),
                       ("TC_ICP_SUMS_P2PLANE", _lib.SUMS_P2PLANE), ("TC_ICP_SUMS_P2P", _lib.SUMS_P2P), ("TC_ICP_SUMS_STRIDE", _lib.SUMS_STRIDE),
                       ("TC_COLL_SUM_F64", _lib.TC_COLL_SUM_F64), ("TC_COLL_SUM_U32", _lib.TC_COLL_SUM_U32),
                       ("TC_COLL_ALLGATHER_U8", _lib.TC_COLL_ALLGATHER_U8), ("TC_SHARD_SPATIAL", _lib.TC_SHARD_SPATIAL),
                       ("TC_SHARD_LOCAL", _lib.TC_SHARD_LOCAL), ("TC_SHARD_INDEX", _lib.TC_SHARD_INDEX),
                       ("TC_COUNTER_INDEXED_POINTS", _lib.TC_COUNTER_INDEXED_POINTS), ("TC_COUNTER_INDEX_BUILDS", _lib.TC_COUNTER_INDEX_BUILDS),
                       ("TC_COUNTER_ICP_ITERATIONS", _lib.TC_COUNTER_ICP_ITERATIONS), ("TC_COUNTER_ICP_TRIPS", _lib.TC_COUNTER_ICP_TRIPS),
                       ("TC_COUNTER_ICP_TRIPS_WITHOUT_SEARCH", _lib.TC_COUNTER_ICP_TRIPS_WITHOUT_SEARCH),
                       ("TC_COUNTER_ICP_SEARCHES", _lib.TC_COUNTER_ICP_SEARCHES), ("TC_COUNTER_ICP_STEPS_NEEDED", _lib.TC_COUNTER_ICP_STEPS_NEEDED),
                       ("TC_COUNTER_ICP_STEPS_TAKEN", _lib.TC_COUNTER_ICP_STEPS_TAKEN)):
        assert lay[f"const.{cname}"] == val, cname
    # constants without a Python mirror: the values their headers document
    assert (lay["const.TC_SEGMENT_PLANE_MAX_ITERS"], lay["const.TC_CLUSTER_NONE"], lay["const.TC_FPFH_DIM"]) == (1 << 20, 0xFFFFFFFF, 33)
    assert lay["call.tc_abi_version"] == lay["const.TC_ABI_VERSION"] == _lib.load().tc_abi_version()


def _rust_structs():
    """#[repr(C)] structs of the Rust shim -> {name: [(field, size, align)]} with the C layout rules for the types it uses"""
    text = "\n".join(rust_text(surface.rust) for surface in _lib.SURFACES)
    prim = {"u64": (8, 8), "usize": (8, 8), "i32": (4, 4), "f32": (4, 4), "u32": (4, 4), "f64": (8, 8), "u8": (1, 1), "c_char": (1, 1),
            "c_int": (4, 4)}
    out = {}
    for m in re.finditer(r"#\[repr\(C\)\](?:\s*#\[derive\([^)]*\)\])?\s*pub struct (\w+)\s*\{([^}]*)\}", text):
        fields = []
        for fm in re.finditer(r"pub (\w+)\s*:\s*([^,]+?)\s*(?:,|$)", m.group(2).strip()):
            ty = fm.group(2).strip()
            am = re.fullmatch(r"\[(\w+);\s*(\d+)\]", ty)
            if am: size, align = prim[am.group(1)][0] * int(am.group(2)), prim[am.group(1)][1]
            elif ty.startswith("*"): size, align = 8, 8
            else: size, align = prim[ty]
            fields.append((fm.group(1), size, align))
        if fields: out[m.group(1)] = fields
    return out


def test_rust_shim_structs_have_the_compiled_layout(exes):
    lay = _layout(exes["c"])
    rs = _rust_structs()
    assert set(rs) == set(MIRROR)
    for name, fields in rs.items():
        off, amax = 0, 1
        for fname, size, align in fields:
            off = (off + align - 1) // align * align
            assert (lay[f"offsetof.{name}.{fname}"], lay[f"fieldsize.{name}.{fname}"]) == (off, size), (name, fname)
            off += size
            amax = max(amax, align)
        assert lay[f"sizeof.{name}"] == (off + amax - 1) // amax * amax, name
        assert len(fields) == sum(1 for k in lay if k.startswith(f"offsetof.{name}.")), name


def test_rust_shim_covers_the_header_and_the_reference_names():
    """Text level (no rustc in this image): ffi.rs declares EVERY tc_* export of the header (tests/test_abi_surfaces.py compares them
    parameter by parameter, type by type), and lib.rs has a `pub fn` for every function name of threecrate-algorithms / the
    threecrate-gpu facade that this path replaces (the shim used to stop short of gpu_icp_point_to_plane,
    gpu_batch_icp, multiscale_icp_point_to_point ...)."""
    lib = open(os.path.join(RUST_DIR, "lib.rs")).read()
    assert sorted(rust_decls("ffi.rs")) == sorted(header_decls("threecrate_hip.h")) == sorted(_lib.EXPORTS)
    # the reference's names on this path: threecrate-algorithms normals.rs:238-380, registration.rs:232-789, gicp.rs:100, kiss_icp.rs:183,
    # filtering.rs:38; threecrate-gpu lib.rs re-exports (normals.rs:443, icp.rs:977-1036, filtering.rs:908, nearest_neighbor.rs:332-367)
    wanted = ["estimate_normals", "estimate_normals_with_config", "estimate_normals_radius", "icp", "icp_detailed", "icp_point_to_point",
              "icp_point_to_point_default", "icp_point_to_plane", "icp_point_to_plane_detailed", "multiscale_icp_point_to_point", "gicp",
              "kiss_icp", "voxel_grid_filter", "gpu_estimate_normals", "gpu_icp", "gpu_icp_point_to_plane", "gpu_batch_icp",
              "gpu_voxel_grid_filter", "gpu_find_k_nearest", "gpu_find_k_nearest_batch", "gpu_find_radius_neighbors"]
    missing = [n for n in wanted if not re.search(r"^pub fn " + n + r"\(", lib, re.M)]
    assert not missing, missing
    for s in ("BatchICPJob", "BatchICPResult", "GpuPointToPlaneICPResult"):
        assert re.search(r"^pub struct " + s + r"\b", lib, re.M), s
    assert "k.min(self.len()).min(2048)" not in lib          # (the silent clamp: the ABI's limit is 2047 and an error)


def _read_result(buf, pos, ns):
    t = np.frombuffer(buf, np.float32, 7, pos); pos += 28
    mse = struct.unpack_from("<f", buf, pos)[0]; pos += 4
    it, conv, ncorr = struct.unpack_from("<3Q", buf, pos); pos += 24
    corr = np.frombuffer(buf, np.uint32, ns, pos); pos += 4 * ns
    return (t, mse, it, bool(conv), ncorr, corr), pos


@pytest.mark.gpu
def test_compiled_consumer_reproduces_the_golden_case(exes, tmp_path, ctx):
    """the 10 k-point golden case (tests/golden/make_golden.py) through the C program's host-buffer calls"""
    from tests.golden.make_golden import corr_digest
    n, k, iters = 10000, 16, 20
    src, tgt, T = synth.registration_pair(n, seed=1)
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<4Q", n, n, k, iters)); f.write(tgt.tobytes()); f.write(src.tobytes())
    for lang in ("c", "cpp"):
        subprocess.check_call([exes[lang], "run", inp, outp])
        buf = open(outp, "rb").read()
        np6 = np.frombuffer(buf, np.float32, n * 6, 0).reshape(n, 6); pos = n * 24
        pl, pos = _read_result(buf, pos, n)
        pp, pos = _read_result(buf, pos, n)
        t_icp = np.frombuffer(buf, np.float32, 7, pos); pos += 28
        codes = struct.unpack_from("<3i", buf, pos); pos += 12
        assert pos == len(buf)
        assert codes == (_lib.TC_INVALID_DATA, _lib.TC_OK, _lib.TC_INVALID_DATA)
        # normals: the golden fixture (oracle) within the budget, the ctypes path bit for bit
        G = os.path.join(ROOT, "tests", "golden")
        ref = np.load(os.path.join(G, "normals_u10k_k16.npy"))
        cs = np.abs((np6[:, 3:].astype(np.float64) * ref.astype(np.float64)).sum(1))
        assert np.array_equal(np6[:, :3], tgt) and cs.min() >= 1 - 1e-4
        assert np.array_equal(np6, ctx.estimate_normals(tgt, k))
        # registrations: golden transform / mse / correspondences
        gold = json.load(open(os.path.join(G, "icp_u10k.json")))
        from oracle import oracle as O
        mat = lambda t: O.isometry_to_matrix(np.asarray(t, np.float32)).astype(np.float64)
        gp = gold["icp_p2p_u10k_20it"]
        assert pp[2] == gp["iterations"] == iters and pp[3] == gp["converged"] and pp[4] == gp["n_correspondences"]
        assert np.linalg.norm(mat(pp[0]) - mat(gp["transformation"])) <= 1e-5 and abs(pp[1] - gp["mse"]) <= 1e-9 + 1e-3 * abs(gp["mse"])
        pairs = np.stack([np.arange(n, dtype=np.int64), pp[5].astype(np.int64)], 1)[pp[5] != 0xFFFFFFFF]
        assert corr_digest(pairs) == gp["correspondences_sha256"]
        # point-to-plane with the program's own normals == the same call through ctypes, bit for bit
        r = ctx.icp_point_to_plane_detailed(src, tgt, np6[:, 3:], None, iters, None, 0.0)
        assert np.array_equal(pl[0], r.transformation) and pl[1] == r.mse and pl[2] == r.iterations == iters
        assert np.array_equal(pl[5].astype(np.int64)[r.correspondences[:, 0]], r.correspondences[:, 1])
        gl = gold["icp_p2pl_u10k_20it"]
        assert np.linalg.norm(mat(pl[0]) - mat(gl["transformation"])) <= 1e-5 and pl[4] == gl["n_correspondences"]
        # icp(): threshold 1e-6, errors swallowed -> a transform near the truth
        assert np.linalg.norm(mat(t_icp) - synth.isometry_matrix(T)) <= 1e-4
