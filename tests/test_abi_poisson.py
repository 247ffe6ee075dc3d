"""The Poisson surface (include/threecrate_hip_poisson.h, _lib.MORE_COMPANIONS, bindings/rust ffi_poisson.rs) held to the checks that
tests/test_abi_shot.py holds the SHOT surface to, through the same readers (tests/abi_text.py).  Its symbols live in an eleventh companion
library, libthreecrate_hip_poisson.so, which needs the product library and the marching-cubes companion; every older library keeps its
names.  This file asserts MEMBERSHIP in the open-ended table and counts nothing but its own names.  No test here needs a GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from threecrate_amd import _lib
from tests import abi_text as T
from tests.test_abi_conformance import _layout
from tests.test_abi_surfaces import ABI_VERSION, TRIVIAL

HEADER, RUST, N_EXPORTS = "threecrate_hip_poisson.h", "ffi_poisson.rs", 5
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_poisson.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")
OLDER = _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS + _lib.FURTHER_COMPANIONS + [s for s in _lib.MORE_COMPANIONS if s.header != HEADER]
CONSTS = dict(TC_POISSON_MIN_POINTS=10, TC_POISSON_MIN_DEPTH=2, TC_POISSON_MAX_DEPTH=8)
STRUCTS = {"tc_poisson_config": ["depth", "scale", "point_weight", "max_iterations", "tolerance", "min_density"],
           "tc_poisson_stats": ["iterations", "rel_residual", "iso_value", "occupied_nodes"]}


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.MORE_COMPANIONS if s.header == HEADER]
    return s


def test_the_surface_joined_the_open_table_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_poisson.so" and "threecrate_hip_shot.h" in [s.header for s in _lib.MORE_COMPANIONS]
    assert len(_lib.FURTHER_COMPANIONS) == 7 and len(_lib.SHOT_EXPORTS) == 4
    assert _lib.POISSON_EXPORTS == list(_lib.signatures(surface)) and len(_lib.POISSON_EXPORTS) == N_EXPORTS
    assert len(_lib.SURFACES) == 4 and sum(len(_lib.signatures(s)) for s in _lib.SURFACES + _lib.EXTENSIONS) == 115
    assert _lib.load().tc_abi_version() == ABI_VERSION == 2


def test_header_table_and_rust_declare_the_same_functions(surface):
    h, r, t = T.header_decls(HEADER), T.rust_decls(RUST), _lib.signatures(surface)
    assert len(h) == len(t) == N_EXPORTS
    assert sorted(h) == sorted(t) == sorted(r)
    counts = {name: n for name, (n, _) in h.items()}
    assert {name: n for name, (n, _) in r.items()} == counts
    assert {name: len(argtypes or ()) for name, (_, argtypes) in t.items()} == counts
    restype = {"": None, "c_int": C.c_int, "usize": C.c_size_t}
    for name, (_, (_, ret)) in h.items():
        assert t[name][0] is restype[ret], (name, ret)
    twins = sorted(name for name in h if name + "_device" in h)
    assert twins == ["tc_poisson_field", "tc_poisson_reconstruct"]
    for name in twins:
        assert h[name + "_device"] == h[name]


def test_header_and_rust_agree_on_every_type():
    h, r = T.header_decls(HEADER), T.rust_decls(RUST)
    bad = {k: (h[k][1], r[k][1]) for k in h if k not in r or h[k][1] != r[k][1]}
    assert not bad, bad


def test_the_tables_scalar_types_are_the_headers(surface):
    scalar = {"usize": C.c_size_t, "f32": C.c_float, "c_int": C.c_int}
    for name, (_, (params, _)) in T.header_decls(HEADER).items():
        for p, a in zip(params, _lib.signatures(surface)[name][1]):
            if p.startswith("*"):
                assert a is C.c_void_p or issubclass(a, C._Pointer), (name, p, a)
            else:
                assert a is scalar[p], (name, p, a)


def test_structs_and_constants_are_the_headers(surface):
    mirror = {name: [f[0] for f in cls._fields_] for name, cls in surface.structs.items()}
    assert mirror == T.header_structs(HEADER) == STRUCTS
    text, rust = T.header_text(HEADER), T.rust_text(RUST)
    assert {k: int(v) for k, v in re.findall(r"#define (TC_POISSON_\w+)\s+(\d+)u?\b", text)} == CONSTS
    assert {k: int(v) for k, v in re.findall(r"pub const (TC_\w+): \w+ = (\d+);", rust)} == CONSTS
    assert {k: getattr(_lib, k) for k in CONSTS} == CONSTS


def test_the_surface_stays_apart_from_every_other_in_both_directions(surface):
    names = set(_lib.signatures(surface))
    own = T.header_text(HEADER)
    for other in OLDER:
        theirs = set(_lib.signatures(other))
        assert not names & theirs, other.header
        assert not [n for n in names if re.search(r"\b" + n + r"\b", T.header_text(other.header))], other.header
        # this header names the one export of another surface that it calls
        assert [n for n in theirs if re.search(r"\b" + n + r"\b", own)] in ([], ["tc_marching_cubes", "tc_marching_cubes_device"]), other.header
        assert not names & set(T.rust_decls(other.rust)), other.rust
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    assert re.search(r"^pub mod ffi_poisson;", lib_rs, re.M) and re.search(r"^pub mod reconstruction \{", lib_rs, re.M)
    used = set(re.findall(r"\bffi_poisson::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    for fn in ("poisson_reconstruction", "poisson_reconstruction_default", "poisson_reconstruction_with_normals"):
        assert re.search(r"pub fn " + fn + r"\(ctx: &HipContext, cloud: &PointCloud<", lib_rs), fn
    assert "dylib=threecrate_hip_poisson" in open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()


def test_companion_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load_companion(HEADER)
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert _lib.load_companion(HEADER) is L and _lib.load_companion("threecrate_hip_shot.h") is not L


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if re.search(r" T tc_\w+$", line))


def test_the_libraries_export_exactly_their_names(surface):
    declared = sorted(_lib.signatures(surface))
    assert _exported(os.path.join(LIBDIR, surface.library)) == declared and len(declared) == N_EXPORTS
    companions = [s.library for s in OLDER if getattr(s, "library", None)]
    for lib in [_lib.LIB_PATH, os.path.join(LIBDIR, "variants", "libthreecrate_hip_dev.so")] + [os.path.join(LIBDIR, c) for c in sorted(set(companions))]:
        assert not set(_exported(lib)) & set(declared), lib
    product = sorted(n for s in _lib.SURFACES + _lib.EXTENSIONS for n in _lib.signatures(s))
    assert _exported(_lib.LIB_PATH) == product and len(product) == 115


def test_the_companion_is_linked_against_the_product_and_marching_cubes(surface):
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(LIBDIR, surface.library)], text=True)
    assert re.search(r"NEEDED.*\[libthreecrate_hip\.so\]", dyn) and re.search(r"NEEDED.*\[libthreecrate_hip_mc\.so\]", dyn)
    assert re.search(r"(RUNPATH|RPATH).*\[\$ORIGIN", dyn), dyn
    mk = open(os.path.join(LIBDIR, "csrc", "Makefile")).read()
    assert re.search(r"^clean:.*poisson\.o.*\$\(POISSON_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(POISSON_OUT\)", mk, re.M) and "poisson.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^poisson\.o:.*run_fold\.h", mk, re.M)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m and m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "poisson.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_poisson_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_poisson", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", f"-Wl,-rpath-link,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_poisson"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"] and lay["count.exports"] == N_EXPORTS
    for call in ("field_null_0", "field_null_1", "reconstruct_null_0", "reconstruct_null_1"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0
    assert (lay["default.depth"], lay["default.max_iterations"], lay["default.floats_ok"]) == (6, 200, 1)
    assert {k: lay["const." + k] for k in CONSTS} == CONSTS


def test_compiled_layout_equals_the_ctypes_mirror_and_the_rust_structs(surface, layouts):
    lay = layouts["c"]
    prim = {"f32": (4, 4), "u32": (4, 4)}
    offsets = set()
    for sname, cls, size in (("tc_poisson_config", _lib.PoissonConfigC, 24), ("tc_poisson_stats", _lib.PoissonStatsC, 16)):
        assert (lay[f"sizeof.{sname}"], lay[f"alignof.{sname}"]) == (C.sizeof(cls), C.alignment(cls)) == (size, 4)
        for fname, _ in cls._fields_:
            assert (lay[f"offsetof.{sname}.{fname}"], lay[f"fieldsize.{sname}.{fname}"]) == (getattr(cls, fname).offset, getattr(cls, fname).size), fname
            offsets.add(f"offsetof.{sname}.{fname}")
        # the C layout rules applied to the #[repr(C)] struct of ffi_poisson.rs (no Rust toolchain compiles the shim)
        m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct " + sname + r"\s*\{([^}]*)\}", T.rust_text(RUST))
        off, amax, names = 0, 1, []
        for fm in re.finditer(r"pub (\w+)\s*:\s*(\w+)\s*,", m.group(1)):
            fsize, align = prim[fm.group(2)]
            off = (off + align - 1) // align * align
            assert (lay[f"offsetof.{sname}.{fm.group(1)}"], lay[f"fieldsize.{sname}.{fm.group(1)}"]) == (off, fsize)
            off, amax = off + fsize, max(amax, align)
            names.append(fm.group(1))
        assert names == [f for f, _ in cls._fields_] and (off + amax - 1) // amax * amax == size
    assert {k for k in lay if k.startswith("offsetof.")} == offsets
