"""The alpha-shape reconstruction surface (include/threecrate_hip_alpha.h, _lib.FURTHER_COMPANIONS, bindings/rust ffi_alpha.rs) held to every
check that tests/test_abi_alpha.py holds the quadric simplification surface to, through the same readers (tests/abi_text.py).  Its symbols live in
an eighth companion library, libthreecrate_hip_alpha.so: the product library's 115 names and the older companions' names stay what they are.
The table is the open-ended list of further companions: this file asserts MEMBERSHIP.  Everything but the last test runs without a GPU;
the last one walks the header's order of checks through the C ABI on a live context."""
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

HEADER, RUST, N_EXPORTS = "threecrate_hip_alpha.h", "ffi_alpha.rs", 3
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_alpha.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.FURTHER_COMPANIONS if s.header == HEADER]
    return s


def test_the_table_is_a_further_companion_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_alpha.so" and HEADER in [s.header for s in _lib.FURTHER_COMPANIONS]
    assert [s.header for s in _lib.COMPANIONS] == ["threecrate_hip_global.h"] and len(_lib.GLOBAL_EXPORTS) == 6
    assert [s.header for s in _lib.LATER_COMPANIONS] == ["threecrate_hip_voxelmap.h"] and len(_lib.VOXELMAP_EXPORTS) == 9
    assert HEADER not in [s.header for s in _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS]
    assert _lib.ALPHA_EXPORTS == list(_lib.signatures(surface)) and len(_lib.ALPHA_EXPORTS) == N_EXPORTS
    assert "threecrate_hip_color.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.COLOR_EXPORTS) == 3
    assert "threecrate_hip_mesh.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.MESH_EXPORTS) == 5
    assert "threecrate_hip_qem.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.QEM_EXPORTS) == 3
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
    assert twins == ["tc_alpha_shape"]
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
    assert sorted(mirror) == ["tc_alpha_config", "tc_alpha_stats"]
    assert mirror["tc_alpha_config"] == ["alpha", "mode", "min_triangle_area", "max_triangles"]             # no fast_mode
    assert mirror["tc_alpha_stats"] == ["candidates", "boundary_candidates", "faces", "capped"]


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
    assert re.search(r"^pub mod ffi_alpha;", lib_rs, re.M)
    used = set(re.findall(r"\bffi_alpha::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    for other in ("ffi.rs", "ffi_filters.rs", "ffi_segmentation.rs", "ffi_ndt.rs", "ffi_tsdf.rs", "ffi_global.rs", "ffi_voxelmap.rs", "ffi_color.rs", "ffi_mesh.rs", "ffi_simplify.rs", "ffi_mc.rs", "ffi_qem.rs"):
        assert not names & set(T.rust_decls(other)), other
    build_rs = open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()
    assert "dylib=threecrate_hip_alpha" in build_rs


def test_companion_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load_companion(HEADER)
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert _lib.load_companion(HEADER) is L
    assert _lib.load_companion("threecrate_hip_global.h") is not L and _lib.load_companion("threecrate_hip_voxelmap.h") is not L
    assert _lib.load_companion("threecrate_hip_simplify.h") is not L and _lib.load_companion("threecrate_hip_mc.h") is not L


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if re.search(r" T tc_\w+$", line))


def test_the_libraries_export_exactly_their_names(surface):
    declared = sorted(_lib.signatures(surface))
    assert _exported(os.path.join(LIBDIR, surface.library)) == declared and len(declared) == N_EXPORTS
    for lib in (_lib.LIB_PATH, os.path.join(LIBDIR, "variants", "libthreecrate_hip_dev.so"), os.path.join(LIBDIR, "libthreecrate_hip_global.so"),
                os.path.join(LIBDIR, "libthreecrate_hip_voxelmap.so"), os.path.join(LIBDIR, "libthreecrate_hip_color.so"), os.path.join(LIBDIR, "libthreecrate_hip_mesh.so"),
                os.path.join(LIBDIR, "libthreecrate_hip_simplify.so"), os.path.join(LIBDIR, "libthreecrate_hip_mc.so"), os.path.join(LIBDIR, "libthreecrate_hip_qem.so")):
        assert not set(_exported(lib)) & set(declared), lib
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_simplify.so")) == sorted(_lib.SIMPLIFY_EXPORTS) and len(_lib.SIMPLIFY_EXPORTS) == 3
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_mc.so")) == sorted(_lib.MC_EXPORTS) and len(_lib.MC_EXPORTS) == 3
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_color.so")) == sorted(_lib.COLOR_EXPORTS) and len(_lib.COLOR_EXPORTS) == 3
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_mesh.so")) == sorted(_lib.MESH_EXPORTS) and len(_lib.MESH_EXPORTS) == 5
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
    assert re.search(r"^clean:.*alpha\.o.*\$\(ALPHA_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(ALPHA_OUT\)", mk, re.M) and "alpha.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m, f"definition of {name} not found"
        assert m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "alpha.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_alpha_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_alpha", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_alpha"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"]
    assert lay["count.exports"] == N_EXPORTS
    for call in ("shape_null", "shape_device_null"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0              # nothing is written without a context
    assert (lay["default.mode"], lay["default.alpha_ok"], lay["default.area_ok"], lay["default.max_triangles"]) == (_lib.TC_ALPHA_BOUNDARY_ONLY, 1, 1, 50000)
    assert (lay["const.TC_ALPHA_BOUNDARY_ONLY"], lay["const.TC_ALPHA_FULL"]) == (_lib.TC_ALPHA_BOUNDARY_ONLY, _lib.TC_ALPHA_FULL) == (0, 1)


def test_compiled_layouts_equal_the_ctypes_mirror(surface, layouts):
    lay, seen = layouts["c"], set()
    for name, cls in surface.structs.items():
        assert lay[f"sizeof.{name}"] == C.sizeof(cls) and lay[f"alignof.{name}"] == C.alignment(cls), name
        for fname, _ in cls._fields_:
            assert lay[f"offsetof.{name}.{fname}"] == getattr(cls, fname).offset, (name, fname)
            assert lay[f"fieldsize.{name}.{fname}"] == getattr(cls, fname).size, (name, fname)
            seen.add(f"offsetof.{name}.{fname}")
    assert {k for k in lay if k.startswith("offsetof.")} == seen
    assert (lay["sizeof.tc_alpha_config"], lay["alignof.tc_alpha_config"]) == (16, 4)
    assert (lay["sizeof.tc_alpha_stats"], lay["alignof.tc_alpha_stats"]) == (32, 8)


def test_rust_structs_have_the_compiled_layout(surface, layouts):
    """the C layout rules applied to the #[repr(C)] struct of ffi_alpha.rs (no Rust toolchain compiles the shim)"""
    lay = layouts["c"]
    prim = {"f32": (4, 4), "u32": (4, 4), "u64": (8, 8)}
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


# ---- the order of the checks, through the C ABI on a live context ----
@pytest.mark.gpu
@pytest.mark.parametrize("road", ["host", "device"])
def test_the_order_of_checks_with_a_live_context(road):
    import torch
    import threecrate_amd as tc
    from tests import alpha_cases as AC

    L = _lib.load_companion(HEADER)
    fn = L.tc_alpha_shape if road == "host" else L.tc_alpha_shape_device
    I, U, A, OK = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED, _lib.TC_ALGORITHM, _lib.TC_OK
    ctx = tc.GpuContext(0)
    try:
        message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
        to = lambda a: a if road == "host" else torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")
        ptr = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
        host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        points, alpha, _ = AC.CASES["sphere300_0.35"]
        want = AC.expected("sphere300_0.35", "boundary")
        n, nf_want = len(points), want["n_faces"]
        dp = to(points)
        out = to(np.full((nf_want + 5, 3), 7, np.uint32))
        untouched = lambda: (host(out).view(np.uint32) == 7).all()
        st = _lib.AlphaStatsC(7, 7, 7, 7)
        stats = lambda: (st.candidates, st.boundary_candidates, st.faces, st.capped)

        def call(cfg, n=n, p_ptr=True, s_ptr=True, pts=dp, cap=nf_want + 5, faces=True):
            torch.cuda.synchronize()
            return fn(ctx._h, ptr(pts) if p_ptr else None, n, None if cfg is None else C.byref(cfg), ptr(out) if faces else None, cap,
                      C.byref(st) if s_ptr else None)

        config = lambda a=alpha, mode=0, area=1e-8, cap=50000: _lib.AlphaConfigC(a, mode, area, cap)
        bad = config(float("nan"), 2, -1.0)
        # 1 (the NULLs) before everything
        for kw in ({"p_ptr": False}, {"s_ptr": False}):
            assert call(bad, n=0, **kw) == I and "NULL" in message()
        assert call(None, n=0) == I and "config is NULL" in message()
        # 2 (the empty cloud, then fewer than three points) before 3, 4, 5
        assert call(bad, n=0) == I and message() == "Point cloud is empty"
        assert call(bad, n=2) == I and message() == "Need at least 3 points for triangulation"
        # 3 before 4 and 5
        assert call(bad, n=2 ** 40) == I and "mode" in message()
        # 4 before 5: alpha, before min_triangle_area
        for a in (float("nan"), float("inf"), 0.0, -1.0):
            assert call(config(a, 1, -1.0), n=2 ** 40) == I and "alpha is" in message()
        assert call(config(alpha, 1, -1.0), n=2 ** 40) == I and "min_triangle_area" in message()
        assert call(config(alpha, 1, float("nan")), n=2 ** 40) == I and "min_triangle_area" in message()
        # 5 (the limit, at its exact bound) before 6
        nan_p = points.copy()
        nan_p[n - 1, 2] = np.nan
        dnan = to(nan_p)
        assert call(config(), n=2 ** 32 - 16, pts=dnan) == U and "n is" in message()
        # 6: a coordinate that is not finite
        assert call(config(), pts=dnan) == I and "a coordinate is not finite" in message()
        # the two TC_ALGORITHM results write nothing, the stats included
        assert call(config(1e-3)) == A and message() == "No candidate triangles generated"
        assert call(config(alpha, 0, 1e30)) == A and message() == "No candidate triangles generated"
        tet = to(AC.CASES["tetrahedron"][0])
        assert call(config(1.5), n=4, pts=tet) == A and message() == "No triangles survived alpha filtering"
        assert stats() == (7, 7, 7, 7) and untouched()                                  # a failed call wrote nothing
        # 8: a capacity one too small: the counts and nothing else
        counts = (want["candidates"], want["boundary_candidates"], nf_want, want["capped"])
        for cap in (nf_want - 1, 0):
            st.candidates = st.faces = 7
            assert call(config(), cap=cap) == I and "cap_faces" in message()
            assert stats() == counts and untouched()
        # the counts-only call: no output array, no capacity
        st.candidates = st.faces = 7
        assert call(config(), cap=0, faces=False) == OK and stats() == counts and untouched()
        # and the exact capacity passes: nothing is written behind the count
        assert call(config(), cap=nf_want) == OK and stats() == counts
        got = host(out).view(np.uint32)
        assert got[:nf_want].tobytes() == want["faces"].tobytes() and (got[nf_want:] == 7).all()
    finally:
        ctx.close()
