"""The quadric-error simplification surface (include/threecrate_hip_qem.h, _lib.FURTHER_COMPANIONS, bindings/rust ffi_qem.rs) held to every
check that tests/test_abi_simplify.py holds the clustering surface to, through the same readers (tests/abi_text.py).  Its symbols live in a
seventh companion library, libthreecrate_hip_qem.so: the product library's 115 names and the older companions' names stay what they are.
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

HEADER, RUST, N_EXPORTS = "threecrate_hip_qem.h", "ffi_qem.rs", 3
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_qem.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.FURTHER_COMPANIONS if s.header == HEADER]
    return s


def test_the_table_is_a_further_companion_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_qem.so" and HEADER in [s.header for s in _lib.FURTHER_COMPANIONS]
    assert [s.header for s in _lib.COMPANIONS] == ["threecrate_hip_global.h"] and len(_lib.GLOBAL_EXPORTS) == 6
    assert [s.header for s in _lib.LATER_COMPANIONS] == ["threecrate_hip_voxelmap.h"] and len(_lib.VOXELMAP_EXPORTS) == 9
    assert HEADER not in [s.header for s in _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS]
    assert _lib.QEM_EXPORTS == list(_lib.signatures(surface)) and len(_lib.QEM_EXPORTS) == N_EXPORTS
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
    assert twins == ["tc_simplify_quadric"]
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
    assert sorted(mirror) == ["tc_qem_config"]
    assert mirror["tc_qem_config"] == ["reduction_ratio", "preserve_boundary", "max_edge_length"]            # no feature_angle_threshold


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
    assert re.search(r"^pub mod ffi_qem;", lib_rs, re.M)
    used = set(re.findall(r"\bffi_qem::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    for other in ("ffi.rs", "ffi_filters.rs", "ffi_segmentation.rs", "ffi_ndt.rs", "ffi_tsdf.rs", "ffi_global.rs", "ffi_voxelmap.rs", "ffi_color.rs", "ffi_mesh.rs", "ffi_simplify.rs", "ffi_mc.rs"):
        assert not names & set(T.rust_decls(other)), other
    build_rs = open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()
    assert "dylib=threecrate_hip_qem" in build_rs


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
                os.path.join(LIBDIR, "libthreecrate_hip_simplify.so"), os.path.join(LIBDIR, "libthreecrate_hip_mc.so")):
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
    assert re.search(r"^clean:.*qem\.o.*\$\(QEM_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(QEM_OUT\)", mk, re.M) and "qem.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m, f"definition of {name} not found"
        assert m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "qem.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_qem_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_qem", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_qem"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"]
    assert lay["count.exports"] == N_EXPORTS
    for call in ("simplify_null", "simplify_device_null"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0              # nothing is written without a context
    assert (lay["default.preserve_boundary"], lay["default.ratio_ok"], lay["default.no_limit"]) == (1, 1, 1)


def test_compiled_layouts_equal_the_ctypes_mirror(surface, layouts):
    lay, seen = layouts["c"], set()
    for name, cls in surface.structs.items():
        assert lay[f"sizeof.{name}"] == C.sizeof(cls) and lay[f"alignof.{name}"] == C.alignment(cls), name
        for fname, _ in cls._fields_:
            assert lay[f"offsetof.{name}.{fname}"] == getattr(cls, fname).offset, (name, fname)
            assert lay[f"fieldsize.{name}.{fname}"] == getattr(cls, fname).size, (name, fname)
            seen.add(f"offsetof.{name}.{fname}")
    assert {k for k in lay if k.startswith("offsetof.")} == seen
    assert (lay["sizeof.tc_qem_config"], lay["alignof.tc_qem_config"]) == (12, 4)


def test_rust_structs_have_the_compiled_layout(surface, layouts):
    """the C layout rules applied to the #[repr(C)] struct of ffi_qem.rs (no Rust toolchain compiles the shim)"""
    lay = layouts["c"]
    prim = {"f32": (4, 4), "u32": (4, 4)}
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
    from tests import qem_cases as SC
    from tests import qem_checker as K

    L = _lib.load_companion(HEADER)
    fn = L.tc_simplify_quadric if road == "host" else L.tc_simplify_quadric_device
    I, U, OK = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED, _lib.TC_OK
    ctx = tc.GpuContext(0)
    try:
        message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
        to = lambda a: a if road == "host" else torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to("cuda:0")
        ptr = lambda a: None if a is None else (a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data)
        host = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        v, f = SC.CASES["icosphere_3"]["vertices"], SC.CASES["icosphere_3"]["faces"]
        n, m = len(v), len(f)
        dv, df = to(v), to(f)
        dev = {"v": to(np.full((n, 3), 7, np.float32)), "f": to(np.full((m, 3), 7, np.uint32)), "m": to(np.full(n, 7, np.uint32))}
        untouched = lambda: all((host(a).view(np.uint32) == np.full(1, 7, host(a).dtype).view(np.uint32)[0]).all() for a in dev.values())
        nv, nf, rounds = C.c_size_t(7), C.c_size_t(7), C.c_uint32(7)

        def call(cfg, n=n, m=m, v_ptr=True, f_ptr=True, counts=(True, True), vertices=dv, faces=df, caps=None, outputs=("v", "f", "m")):
            torch.cuda.synchronize()
            cap_v, cap_f = caps if caps is not None else (n, m)
            return fn(ctx._h, ptr(vertices) if v_ptr else None, n, ptr(faces) if f_ptr else None, m, None if cfg is None else C.byref(cfg),
                      ptr(dev["v"]) if "v" in outputs else None, cap_v, ptr(dev["f"]) if "f" in outputs else None, cap_f,
                      ptr(dev["m"]) if "m" in outputs else None, C.byref(nv) if counts[0] else None, C.byref(nf) if counts[1] else None, C.byref(rounds))

        config = lambda ratio=0.5, pb=1, max_len=0.0: _lib.QemConfigC(ratio, pb, max_len)
        bad = config(float("nan"), 2, -1.0)
        # 1 (the NULLs) before everything
        for kw in ({"v_ptr": False}, {"f_ptr": False}, {"counts": (False, True)}, {"counts": (True, False)}):
            assert call(bad, n=0, m=0, **kw) == I and "NULL" in message()
        assert call(None, n=0, m=0) == I and "config is NULL" in message()
        # 2 (the empty mesh) before 3, 4, 5
        assert call(bad, n=0, m=2 ** 40) == I and message() == "Mesh is empty"
        assert call(bad, n=2 ** 40, m=0) == I and message() == "Mesh is empty"
        # 3 before 4 and 5
        assert call(bad, n=2 ** 40) == I and "preserve_boundary" in message()
        # 4 before 5: the ratio, before max_edge_length
        assert call(config(1.5, 1, -1.0), n=2 ** 40) == I and message() == "Reduction ratio must be between 0.0 and 1.0"
        assert call(config(0.5, 1, -1.0), m=2 ** 40) == I and "max_edge_length" in message()
        assert call(config(0.5, 1, float("nan")), m=2 ** 40) == I and "max_edge_length" in message()
        # 5 (the limits, at their exact bounds) before 6
        bad_faces = f.copy()
        bad_faces[5, 1] = n
        dbad = to(bad_faces)
        assert call(config(), n=2 ** 32 - 16, faces=dbad) == U and "n_vertices" in message()
        assert call(config(), m=1431655760, faces=dbad) == U and "n_faces" in message()
        # 6: a bad index, a NaN coordinate; with ratio 0 as well
        nan_v = v.copy()
        nan_v[n - 1, 2] = np.nan
        dnan = to(nan_v)
        for cfg in (config(), config(0.0)):
            assert call(cfg, faces=dbad) == I and "a face index is >= n_vertices" in message()
            assert call(cfg, vertices=dnan) == I and "a vertex coordinate is not finite" in message()
        assert (nv.value, nf.value, rounds.value) == (7, 7, 7) and untouched()          # a failed call wrote nothing
        # 7: capacities one too small: the counts and nothing else
        want = K.simplify(v, f, K.config(0.5))
        nv_want, nf_want = len(want["vertices"]), len(want["faces"])
        for caps, word in (((nv_want - 1, nf_want), "cap_vertices"), ((nv_want, nf_want - 1), "cap_faces"), ((0, 0), "cap_vertices")):
            nv.value = nf.value = 7
            assert call(config(), caps=caps) == I and word in message()
            assert (nv.value, nf.value) == (nv_want, nf_want) and untouched()
        assert call(config(), caps=(0, 0), outputs=("m",)) == I and untouched()       # the vertex map alone is an output like the others
        assert call(config(0.0), caps=(n - 1, m)) == I and (nv.value, nf.value) == (n, m) and untouched()
        # the counts-only call: no output array, no capacity
        nv.value = nf.value = 7
        assert call(config(), caps=(0, 0), outputs=()) == OK and (nv.value, nf.value, rounds.value) == (nv_want, nf_want, want["rounds"])
        assert call(config(0.0), caps=(0, 0), outputs=()) == OK and (nv.value, nf.value, rounds.value) == (n, m, 0)
        # and exact capacities pass: nothing is written behind the counts
        assert call(config(), caps=(nv_want, nf_want)) == OK
        assert host(dev["v"])[:nv_want].tobytes() == want["vertices"].tobytes() and (host(dev["v"])[nv_want:] == 7).all()
        assert host(dev["f"]).view(np.uint32)[:nf_want].tobytes() == want["faces"].tobytes() and (host(dev["f"]).view(np.uint32)[nf_want:] == 7).all()
        assert host(dev["m"]).view(np.uint32).tobytes() == want["map"].tobytes()
    finally:
        ctx.close()
