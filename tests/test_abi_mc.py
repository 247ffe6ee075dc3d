"""The marching-cubes surface (include/threecrate_hip_mc.h, _lib.FURTHER_COMPANIONS, bindings/rust ffi_mc.rs) held to every check that
tests/test_abi_simplify.py holds the simplification surface to, through the same readers (tests/abi_text.py).  Its symbols live in a
sixth companion library, libthreecrate_hip_mc.so: the product library's 115 names and the older companions' six, nine, three, five and
three stay what they are.  The rules that need a live context (the count call, the capacities, every invalid argument) are in
tests/test_gpu_mc.py.  The table is the open-ended list of further companions: this file asserts MEMBERSHIP.  No compute calls: this
runs without a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from threecrate_amd import _lib
from tests import abi_text as T
from tests.test_abi_conformance import _layout
from tests.test_abi_surfaces import ABI_VERSION, TRIVIAL

HEADER, RUST, N_EXPORTS = "threecrate_hip_mc.h", "ffi_mc.rs", 3
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_mc.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.FURTHER_COMPANIONS if s.header == HEADER]
    return s


def test_the_table_is_a_further_companion_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_mc.so" and HEADER in [s.header for s in _lib.FURTHER_COMPANIONS]
    assert [s.header for s in _lib.COMPANIONS] == ["threecrate_hip_global.h"] and len(_lib.GLOBAL_EXPORTS) == 6
    assert [s.header for s in _lib.LATER_COMPANIONS] == ["threecrate_hip_voxelmap.h"] and len(_lib.VOXELMAP_EXPORTS) == 9
    assert HEADER not in [s.header for s in _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS]
    assert _lib.MC_EXPORTS == list(_lib.signatures(surface)) and len(_lib.MC_EXPORTS) == N_EXPORTS
    assert "threecrate_hip_simplify.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.SIMPLIFY_EXPORTS) == 3
    assert "threecrate_hip_color.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.COLOR_EXPORTS) == 3
    assert "threecrate_hip_mesh.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.MESH_EXPORTS) == 5
    assert len(_lib.SURFACES) == 4 and sum(len(_lib.signatures(s)) for s in _lib.SURFACES + _lib.EXTENSIONS) == 115
    assert _lib.load().tc_abi_version() == ABI_VERSION == 2
    assert "open-ended" in _lib._further_companions.__doc__ and "test_abi_voxelmap.py" in _lib._further_companions.__doc__


def test_header_table_and_rust_declare_the_same_functions(surface):
    h, r, t = T.header_decls(HEADER), T.rust_decls(RUST), _lib.signatures(surface)
    assert len(h) == len(t) == N_EXPORTS
    assert sorted(h) == sorted(t), sorted(set(h) ^ set(t))
    assert sorted(r) == sorted(h), sorted(set(h) ^ set(r))
    counts = {name: n for name, (n, _) in h.items()}
    assert {name: n for name, (n, _) in r.items()} == counts
    assert {name: len(argtypes or ()) for name, (_, argtypes) in t.items()} == counts
    restype = {"": None, "c_int": C.c_int}
    for name, (_, (_, ret)) in h.items():
        assert t[name][0] is restype[ret], (name, ret)
    twins = [name for name in h if name + "_device" in h]
    assert twins == ["tc_marching_cubes"]
    for name in twins:
        assert h[name + "_device"] == h[name], name


def test_header_and_rust_agree_on_every_type():
    h, r = T.header_decls(HEADER), T.rust_decls(RUST)
    bad = {k: (h[k][1], r[k][1]) for k in h if k not in r or h[k][1] != r[k][1]}
    assert not bad, bad


def test_the_tables_scalar_types_are_the_headers(surface):
    """a pointer is an address in the table; a scalar has the header's width and kind"""
    scalar = {"usize": C.c_size_t, "f32": C.c_float}
    for name, (_, (params, _)) in T.header_decls(HEADER).items():
        argtypes = _lib.signatures(surface)[name][1]
        for p, a in zip(params, argtypes):
            if p.startswith("*"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is scalar[p], (name, p, a)


def test_structs_are_the_headers_field_by_field(surface):
    mirror = {name: [f[0] for f in cls._fields_] for name, cls in surface.structs.items()}
    assert mirror == T.header_structs(HEADER)
    assert sorted(mirror) == ["tc_mc_config", "tc_mc_grid"]
    assert mirror["tc_mc_grid"] == ["dims", "voxel_size", "origin", "layout"] and mirror["tc_mc_config"] == ["iso_level", "flags"]


def test_the_surface_stays_apart_from_every_other_in_both_directions(surface):
    names = set(_lib.signatures(surface))
    own = T.header_text(HEADER)
    others = _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS + [s for s in _lib.FURTHER_COMPANIONS if s.header != HEADER]
    for other in others:
        theirs = set(_lib.signatures(other))
        assert not names & theirs, other.header
        assert not [n for n in names if re.search(r"\b" + n + r"\b", T.header_text(other.header))], other.header
        assert not [n for n in theirs if re.search(r"\b" + n + r"\b", own)], other.header
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    assert re.search(r"^pub mod ffi_mc;", lib_rs, re.M)
    used = set(re.findall(r"\bffi_mc::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    for other in ("ffi.rs", "ffi_filters.rs", "ffi_segmentation.rs", "ffi_ndt.rs", "ffi_tsdf.rs", "ffi_global.rs", "ffi_voxelmap.rs", "ffi_color.rs", "ffi_mesh.rs", "ffi_simplify.rs"):
        assert not names & set(T.rust_decls(other)), other
    build_rs = open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()
    assert "dylib=threecrate_hip_mc" in build_rs


def test_companion_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load_companion(HEADER)
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert _lib.load_companion(HEADER) is L
    assert _lib.load_companion("threecrate_hip_global.h") is not L and _lib.load_companion("threecrate_hip_voxelmap.h") is not L
    assert _lib.load_companion("threecrate_hip_color.h") is not L and _lib.load_companion("threecrate_hip_mesh.h") is not L
    assert _lib.load_companion("threecrate_hip_simplify.h") is not L


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if re.search(r" T tc_\w+$", line))


def test_the_seven_libraries_export_exactly_their_names(surface):
    declared = sorted(_lib.signatures(surface))
    assert _exported(os.path.join(LIBDIR, surface.library)) == declared and len(declared) == N_EXPORTS
    for lib in (_lib.LIB_PATH, os.path.join(LIBDIR, "variants", "libthreecrate_hip_dev.so"), os.path.join(LIBDIR, "libthreecrate_hip_global.so"),
                os.path.join(LIBDIR, "libthreecrate_hip_voxelmap.so"), os.path.join(LIBDIR, "libthreecrate_hip_color.so"), os.path.join(LIBDIR, "libthreecrate_hip_mesh.so"), os.path.join(LIBDIR, "libthreecrate_hip_simplify.so")):
        assert not set(_exported(lib)) & set(declared), lib
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_color.so")) == sorted(_lib.COLOR_EXPORTS) and len(_lib.COLOR_EXPORTS) == 3
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_mesh.so")) == sorted(_lib.MESH_EXPORTS) and len(_lib.MESH_EXPORTS) == 5
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_simplify.so")) == sorted(_lib.SIMPLIFY_EXPORTS) and len(_lib.SIMPLIFY_EXPORTS) == 3
    assert (len(_lib.GLOBAL_EXPORTS), len(_lib.VOXELMAP_EXPORTS)) == (6, 9)
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_global.so")) == sorted(_lib.GLOBAL_EXPORTS)
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_voxelmap.so")) == sorted(_lib.VOXELMAP_EXPORTS)
    product = sorted(n for s in _lib.SURFACES + _lib.EXTENSIONS for n in _lib.signatures(s))
    assert _exported(_lib.LIB_PATH) == product and len(product) == 115


def test_the_companion_is_linked_like_the_voxel_map(surface):
    """against the product library by name, found through $ORIGIN"""
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(LIBDIR, surface.library)], text=True)
    assert re.search(r"NEEDED.*\[libthreecrate_hip\.so\]", dyn) and re.search(r"(RUNPATH|RPATH).*\[\$ORIGIN", dyn), dyn
    mk = open(os.path.join(LIBDIR, "csrc", "Makefile")).read()
    assert re.search(r"^clean:.*mc\.o.*\$\(MC_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(MC_OUT\)", mk, re.M) and "mc.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m, f"definition of {name} not found"
        assert m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "mc.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_mc_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_mc", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_mc"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"]
    assert lay["count.exports"] == N_EXPORTS
    assert lay["const.TC_MC_Z_FASTEST"] == _lib.TC_MC_Z_FASTEST == 0 and lay["const.TC_MC_X_FASTEST"] == _lib.TC_MC_X_FASTEST == 1
    assert lay["const.TC_MC_NORMALS"] == _lib.TC_MC_NORMALS == 1 and lay["const.TC_MC_WELD"] == _lib.TC_MC_WELD == 2
    for call in ("mc_null", "mc_device_null"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0              # nothing is written without a context
    assert (lay["default.iso_is_zero"], lay["default.flags"]) == (1, _lib.TC_MC_NORMALS)       # MarchingCubesConfig::default()


def test_compiled_layouts_equal_the_ctypes_mirror(surface, layouts):
    lay, seen = layouts["c"], set()
    for name, cls in surface.structs.items():
        assert lay[f"sizeof.{name}"] == C.sizeof(cls) and lay[f"alignof.{name}"] == C.alignment(cls), name
        for fname, _ in cls._fields_:
            assert lay[f"offsetof.{name}.{fname}"] == getattr(cls, fname).offset, (name, fname)
            assert lay[f"fieldsize.{name}.{fname}"] == getattr(cls, fname).size, (name, fname)
            seen.add(f"offsetof.{name}.{fname}")
    assert {k for k in lay if k.startswith("offsetof.")} == seen
    assert (lay["sizeof.tc_mc_grid"], lay["alignof.tc_mc_grid"]) == (40, 4) and (lay["sizeof.tc_mc_config"], lay["alignof.tc_mc_config"]) == (8, 4)


def test_rust_structs_have_the_compiled_layout(surface, layouts):
    """the C layout rules applied to the #[repr(C)] structs of ffi_mc.rs (no Rust toolchain compiles the shim)"""
    lay = layouts["c"]
    prim = {"f32": (4, 4), "u32": (4, 4), "[u32; 3]": (12, 4), "[f32; 3]": (12, 4)}
    rs = {}
    for m in re.finditer(r"#\[repr\(C\)\](?:\s*#\[derive\([^)]*\)\])?\s*pub struct (\w+)\s*\{([^}]*)\}", T.rust_text(RUST)):
        fields = [(fm.group(1),) + prim[fm.group(2).strip()] for fm in re.finditer(r"pub (\w+)\s*:\s*([^,]+?)\s*(?:,|$)", m.group(2).strip())]
        rs[m.group(1)] = fields
    assert set(rs) == set(surface.structs)
    for name, fields in rs.items():
        off, amax = 0, 1
        for fname, size, align in fields:
            off = (off + align - 1) // align * align
            assert (lay[f"offsetof.{name}.{fname}"], lay[f"fieldsize.{name}.{fname}"]) == (off, size), (name, fname)
            off += size
            amax = max(amax, align)
        assert lay[f"sizeof.{name}"] == (off + amax - 1) // amax * amax and lay[f"alignof.{name}"] == amax, name
        assert [f[0] for f in fields] == [f[0] for f in surface.structs[name]._fields_]
    for const, value in (("TC_MC_Z_FASTEST: u32", "0"), ("TC_MC_X_FASTEST: u32", "1"), ("TC_MC_NORMALS: u32", "1"), ("TC_MC_WELD: u32", "2")):
        assert re.search(r"pub const " + re.escape(const) + " = " + re.escape(value) + ";", T.rust_text(RUST)), const
