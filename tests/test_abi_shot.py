"""The SHOT / USC surface (include/threecrate_hip_shot.h, _lib.MORE_COMPANIONS, bindings/rust ffi_shot.rs) held to every check that
tests/test_abi_ground.py holds the ground surface to, through the same readers (tests/abi_text.py).  Its symbols live in a tenth companion
library, libthreecrate_hip_shot.so: the product library's 115 names and the older companions' names stay what they are.  The table is a
list of its own (tests/test_abi_ground.py counts the libraries of the older three): this file asserts MEMBERSHIP and counts nothing but its
own names.  Everything but the last tests runs without a GPU; the last ones walk the header's order of checks through the C ABI on a live
context, through both roads, with lrf and flags NULL in every combination."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from threecrate_amd import _lib
from tests import abi_text as T
from tests.test_abi_conformance import _layout
from tests.test_abi_surfaces import ABI_VERSION, TRIVIAL

HEADER, RUST, N_EXPORTS = "threecrate_hip_shot.h", "ffi_shot.rs", 4
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_shot.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")
OLDER = _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS + _lib.FURTHER_COMPANIONS
FLAGS = dict(TC_SHOT_ROAD_BALL=0, TC_SHOT_ROAD_FALLBACK=1, TC_SHOT_ROAD_INERT=2, TC_SHOT_ROAD_MASK=3, TC_SHOT_X_TIE=4, TC_SHOT_ZERO_COV=8, TC_SHOT_EMPTY=16)


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.MORE_COMPANIONS if s.header == HEADER]
    return s


def test_the_table_is_a_list_of_its_own_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_shot.so" and HEADER not in [s.header for s in OLDER]
    assert [s.header for s in _lib.COMPANIONS] == ["threecrate_hip_global.h"] and len(_lib.GLOBAL_EXPORTS) == 6
    assert [s.header for s in _lib.LATER_COMPANIONS] == ["threecrate_hip_voxelmap.h"] and len(_lib.VOXELMAP_EXPORTS) == 9
    assert len(_lib.FURTHER_COMPANIONS) == 7 and len(_lib.GROUND_EXPORTS) == 4
    assert _lib.SHOT_EXPORTS == list(_lib.signatures(surface)) and len(_lib.SHOT_EXPORTS) == N_EXPORTS
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
    twins = [name for name in h if name + "_device" in h]
    assert twins == ["tc_extract_shot_features_with_normals"]
    assert h[twins[0] + "_device"] == h[twins[0]]


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


def test_struct_and_constants_are_the_headers(surface):
    mirror = {name: [f[0] for f in cls._fields_] for name, cls in surface.structs.items()}
    assert mirror == T.header_structs(HEADER) == {"tc_shot_config": ["search_radius", "k_neighbors", "variant"]}
    text, rust = T.header_text(HEADER), T.rust_text(RUST)
    consts = dict(FLAGS, TC_SHOT_DIM=352, TC_USC_DIM=128, TC_SHOT_VARIANT_SHOT=0, TC_SHOT_VARIANT_USC=1)
    assert {k: int(v) for k, v in re.findall(r"#define (TC_(?:SHOT|USC)_\w+)\s+(\d+)u?\b", text)} == consts
    assert {k: int(v) for k, v in re.findall(r"pub const (TC_\w+): \w+ = (\d+);", rust)} == consts
    assert {k: getattr(_lib, k) for k in consts} == consts


def test_the_surface_stays_apart_from_every_other_in_both_directions(surface):
    names = set(_lib.signatures(surface))
    own = T.header_text(HEADER)
    for other in OLDER:
        theirs = set(_lib.signatures(other))
        assert not names & theirs, other.header
        assert not [n for n in names if re.search(r"\b" + n + r"\b", T.header_text(other.header))], other.header
        assert not [n for n in theirs if re.search(r"\b" + n + r"\b", own)], other.header
        assert not names & set(T.rust_decls(other.rust)), other.rust
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    assert re.search(r"^pub mod ffi_shot;", lib_rs, re.M) and re.search(r"^pub mod features \{", lib_rs, re.M)
    used = set(re.findall(r"\bffi_shot::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    assert re.search(r"pub fn extract_shot_features_with_normals\(ctx: &HipContext, cloud: &PointCloud<NormalPoint3f>, config: &ShotConfig\) -> Result<Vec<Vec<f32>>>", lib_rs)
    assert "dylib=threecrate_hip_shot" in open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()


def test_companion_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load_companion(HEADER)
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert _lib.load_companion(HEADER) is L and _lib.load_companion("threecrate_hip_ground.h") is not L


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if re.search(r" T tc_\w+$", line))


def test_the_libraries_export_exactly_their_names(surface):
    declared = sorted(_lib.signatures(surface))
    assert _exported(os.path.join(LIBDIR, surface.library)) == declared and len(declared) == N_EXPORTS
    companions = [s.library for s in _lib.COMPANIONS + _lib.LATER_COMPANIONS + _lib.FURTHER_COMPANIONS]
    for lib in [_lib.LIB_PATH, os.path.join(LIBDIR, "variants", "libthreecrate_hip_dev.so")] + [os.path.join(LIBDIR, c) for c in companions]:
        assert not set(_exported(lib)) & set(declared), lib
    product = sorted(n for s in _lib.SURFACES + _lib.EXTENSIONS for n in _lib.signatures(s))
    assert _exported(_lib.LIB_PATH) == product and len(product) == 115


def test_the_companion_is_linked_like_the_others(surface):
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(LIBDIR, surface.library)], text=True)
    assert re.search(r"NEEDED.*\[libthreecrate_hip\.so\]", dyn) and re.search(r"(RUNPATH|RPATH).*\[\$ORIGIN", dyn), dyn
    mk = open(os.path.join(LIBDIR, "csrc", "Makefile")).read()
    assert re.search(r"^clean:.*shot\.o.*\$\(SHOT_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(SHOT_OUT\)", mk, re.M) and "shot.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^shot\.o:.*sym3_eigen\.h", mk, re.M)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m and m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "shot.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_shot_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_shot", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_shot"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"] and lay["count.exports"] == N_EXPORTS
    for call in ("extract_null", "extract_device_null"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0
    assert (lay["default.radius_ok"], lay["default.k"], lay["default.variant"]) == (1, 10, 0)
    assert (lay["dim.shot"], lay["dim.usc"], lay["dim.other"], lay["dim.negative"]) == (352, 128, 0, 0)
    assert {k: lay["const." + k] for k in FLAGS} == FLAGS and (lay["const.TC_SHOT_DIM"], lay["const.TC_USC_DIM"]) == (352, 128)


def test_compiled_layout_equals_the_ctypes_mirror_and_the_rust_struct(surface, layouts):
    lay, cls = layouts["c"], _lib.ShotConfigC
    assert (lay["sizeof.tc_shot_config"], lay["alignof.tc_shot_config"]) == (C.sizeof(cls), C.alignment(cls)) == (24, 8)
    for fname, _ in cls._fields_:
        assert (lay[f"offsetof.tc_shot_config.{fname}"], lay[f"fieldsize.tc_shot_config.{fname}"]) == (getattr(cls, fname).offset, getattr(cls, fname).size), fname
    assert {k for k in lay if k.startswith("offsetof.")} == {f"offsetof.tc_shot_config.{f}" for f, _ in cls._fields_}
    # the C layout rules applied to the #[repr(C)] struct of ffi_shot.rs (no Rust toolchain compiles the shim)
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct tc_shot_config\s*\{([^}]*)\}", T.rust_text(RUST))
    prim = {"f32": (4, 4), "usize": (8, 8), "c_int": (4, 4)}
    off, amax, names = 0, 1, []
    for fm in re.finditer(r"pub (\w+)\s*:\s*(\w+)\s*,", m.group(1)):
        size, align = prim[fm.group(2)]
        off = (off + align - 1) // align * align
        assert (lay[f"offsetof.tc_shot_config.{fm.group(1)}"], lay[f"fieldsize.tc_shot_config.{fm.group(1)}"]) == (off, size)
        off, amax = off + size, max(amax, align)
        names.append(fm.group(1))
    assert names == [f for f, _ in cls._fields_] and (off + amax - 1) // amax * amax == 24


# ---- the order of the checks and the optional outputs, through the C ABI on a live context ----
@pytest.mark.gpu
@pytest.mark.parametrize("road", ["host", "device"])
def test_the_order_of_checks_with_a_live_context(road):
    import torch
    import threecrate_amd as tc
    from tests import shot_cases as CASES
    from tests import shot_checker as SC

    L = _lib.load_companion(HEADER)
    fn = L.tc_extract_shot_features_with_normals if road == "host" else L.tc_extract_shot_features_with_normals_device
    I, U, OK = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED, _lib.TC_OK
    ctx = tc.GpuContext(0)
    try:
        message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
        dev = road == "device"
        c = CASES.case("blocks_65")
        np6, n = c["np6"], len(c["np6"])
        p = torch.from_numpy(np.array(np6)).to("cuda:0") if dev else np6
        new = lambda shape, dtype: torch.full(shape, 7, dtype=torch.float32 if dtype is np.float32 else torch.int32, device="cuda:0") if dev else np.full(shape, 7, dtype)
        ptr = lambda a: a.data_ptr() if dev else a.ctypes.data
        host = lambda a: a.cpu().numpy() if dev else a
        out, lrf, flags = new((n, 352), np.float32), new((n, 9), np.float32), new((n,), np.uint32)
        untouched = lambda: bool((host(out) == 7).all() and (host(lrf) == 7).all() and (host(flags) == 7).all())

        def call(cfg, n=n, p_ptr=True, o_ptr=True, l_ptr=True, f_ptr=True, o=None):
            if dev:
                torch.cuda.synchronize()
            return fn(ctx._h, ptr(p) if p_ptr else None, n, None if cfg is None else C.byref(cfg), ptr(out if o is None else o) if o_ptr else None,
                      ptr(lrf) if l_ptr else None, ptr(flags) if f_ptr else None)

        config = lambda radius=c["radius"], k=c["k"], variant=0: _lib.ShotConfigC(radius, k, variant)
        # 1: the NULLs before everything (a wrong variant, a wrong radius, too many points and too large a k behind them)
        assert call(None, n=2 ** 40) == I and "config is NULL" in message()
        assert call(config(-1.0, 4096, 7), n=2 ** 40, p_ptr=False) == I and "normal_points is NULL" in message()
        assert call(config(-1.0, 4096, 7), n=2 ** 40, o_ptr=False) == I and "out is NULL" in message()
        assert call(config(-1.0, 4096, 7), n=0, o_ptr=False) == I and "out is NULL" in message()
        # 2: the variant before the radius
        for v in (2, -1):
            assert call(config(-1.0, 4096, v), n=2 ** 40) == I and "variant" in message()
        # 3: the radius before the sizes
        for r in (0.0, -1.0, float("nan"), float("inf")):
            assert call(config(r, 4096), n=2 ** 40) == I and message() == "search_radius must be positive"
        # 4: the empty cloud before the limits, with or without points
        assert call(config(k=4096), n=0) == OK and call(config(k=4096), n=0, p_ptr=False) == OK
        # 5: the limits, each at its bound
        assert call(config(), n=2 ** 32 - 15) == U and "n is above" in message()
        assert call(config(k=2048)) == U and "k_neighbors > 2047" in message()
        assert untouched()                                      # a failed call wrote nothing
        # and full calls on the same context afterwards: lrf and flags NULL in every combination, both variants
        for variant, name in enumerate(CASES.VARIANTS):
            want = CASES.expected("blocks_65", name)
            for mask in range(4):
                o = new((n, SC.dim(name)), np.float32)
                lrf, flags = new((n, 9), np.float32), new((n,), np.uint32)
                assert call(config(variant=variant), l_ptr=bool(mask & 1), f_ptr=bool(mask & 2), o=o) == OK, (name, mask)
                got_l = host(lrf) if mask & 1 else want["lrf"]
                got_f = host(flags).view(np.uint32) if mask & 2 else want["flags"]
                assert (mask & 1) or (host(lrf) == 7).all()
                assert (mask & 2) or (host(flags) == 7).all()
                assert not SC.compare(host(o), got_l, got_f, want), (name, mask)
    finally:
        ctx.close()
