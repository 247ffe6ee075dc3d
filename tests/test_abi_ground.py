"""The ground segmentation surface (include/threecrate_hip_ground.h, _lib.FURTHER_COMPANIONS, bindings/rust ffi_ground.rs) held to every
check that tests/test_abi_alpha.py holds the alpha-shape surface to, through the same readers (tests/abi_text.py).  Its symbols live in
a ninth companion library, libthreecrate_hip_ground.so: the product library's 115 names and the older companions' names stay what they are.
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

HEADER, RUST, N_EXPORTS = "threecrate_hip_ground.h", "ffi_ground.rs", 4
SRC = os.path.join(T.ROOT, "tests", "abi", "abi_ground.c")
LIBDIR = os.path.join(T.ROOT, "threecrate_amd")


@pytest.fixture(scope="module")
def surface():
    (s,) = [s for s in _lib.FURTHER_COMPANIONS if s.header == HEADER]
    return s


def test_the_table_is_a_further_companion_and_the_other_tables_are_untouched(surface):
    assert surface.library == "libthreecrate_hip_ground.so" and HEADER in [s.header for s in _lib.FURTHER_COMPANIONS]
    assert [s.header for s in _lib.COMPANIONS] == ["threecrate_hip_global.h"] and len(_lib.GLOBAL_EXPORTS) == 6
    assert [s.header for s in _lib.LATER_COMPANIONS] == ["threecrate_hip_voxelmap.h"] and len(_lib.VOXELMAP_EXPORTS) == 9
    assert HEADER not in [s.header for s in _lib.SURFACES + _lib.EXTENSIONS + _lib.COMPANIONS + _lib.LATER_COMPANIONS]
    assert _lib.GROUND_EXPORTS == list(_lib.signatures(surface)) and len(_lib.GROUND_EXPORTS) == N_EXPORTS
    assert "threecrate_hip_alpha.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.ALPHA_EXPORTS) == 3
    assert "threecrate_hip_qem.h" in [s.header for s in _lib.FURTHER_COMPANIONS] and len(_lib.QEM_EXPORTS) == 3
    assert len(_lib.SURFACES) == 4 and sum(len(_lib.signatures(s)) for s in _lib.SURFACES + _lib.EXTENSIONS) == 115
    assert _lib.load().tc_abi_version() == ABI_VERSION == 2
    assert "open-ended" in _lib._further_companions.__doc__


def test_header_table_and_rust_declare_the_same_functions(surface):
    h, r, t = T.header_decls(HEADER), T.rust_decls(RUST), _lib.signatures(surface)
    assert len(h) == len(t) == N_EXPORTS
    assert sorted(h) == sorted(t), sorted(set(h) ^ set(t))
    assert sorted(r) == sorted(h), sorted(set(h) ^ set(r))
    counts = {name: n for name, (n, _) in h.items()}
    assert {name: n for name, (n, _) in r.items()} == counts
    assert {name: len(argtypes or ()) for name, (_, argtypes) in t.items()} == counts
    restype = {"": None, "c_int": C.c_int, "usize": C.c_size_t}
    for name, (_, (_, ret)) in h.items():
        assert t[name][0] is restype[ret], (name, ret)
    twins = [name for name in h if name + "_device" in h]
    assert twins == ["tc_segment_ground"]
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
    assert sorted(mirror) == ["tc_ground_config", "tc_ground_patch"]
    assert mirror["tc_ground_config"] == ["sensor_height", "n_zones", "zone_radii", "num_rings", "num_sectors", "max_range", "min_points_per_patch",
                                          "num_seed_points", "seed_selection_threshold", "dist_threshold", "num_iterations", "uprightness_threshold",
                                          "flatness_threshold", "elevation_threshold"]
    assert mirror["tc_ground_patch"] == ["count", "n_inliers", "status", "normal", "d", "mean_z", "flatness"]
    # the status codes: the header's, the table's, the Rust file's
    codes = dict(re.findall(r"#define (TC_GROUND_PATCH_\w+)\s+(\d+)u", T.header_text(HEADER)))
    assert [k[len("TC_GROUND_PATCH_"):] for k in sorted(codes, key=lambda k: int(codes[k]))] == list(_lib.TC_GROUND_STATUS)
    assert {k: int(v) for k, v in codes.items()} == {"TC_GROUND_PATCH_" + s: i for i, s in enumerate(_lib.TC_GROUND_STATUS)}
    assert {k: int(v) for k, v in re.findall(r"pub const (TC_GROUND_PATCH_\w+): u32 = (\d+);", T.rust_text(RUST))} == {k: int(v) for k, v in codes.items()}
    assert re.search(r"#define TC_GROUND_MAX_ZONES 8\b", T.header_text(HEADER)) and _lib.TC_GROUND_MAX_ZONES == 8


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
    assert re.search(r"^pub mod ffi_ground;", lib_rs, re.M)
    used = set(re.findall(r"\bffi_ground::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used and used <= set(T.rust_decls(RUST)), used - set(T.rust_decls(RUST))
    assert re.search(r"pub fn patchwork_plus_plus\(ctx: &HipContext, cloud: &PointCloud<Point3f>, config: PatchworkConfig\) -> Result<GroundSegmentationResult>", lib_rs)
    assert re.search(r"pub fn segment_ground\(ctx: &HipContext, cloud: &PointCloud<Point3f>, sensor_height: f32\) -> Result<GroundSegmentationResult>", lib_rs)
    for other in ("ffi.rs", "ffi_filters.rs", "ffi_segmentation.rs", "ffi_ndt.rs", "ffi_tsdf.rs", "ffi_global.rs", "ffi_voxelmap.rs", "ffi_color.rs", "ffi_mesh.rs",
                  "ffi_simplify.rs", "ffi_mc.rs", "ffi_qem.rs", "ffi_alpha.rs"):
        assert not names & set(T.rust_decls(other)), other
    build_rs = open(os.path.join(T.RUST_DIR, "..", "build.rs")).read()
    assert "dylib=threecrate_hip_ground" in build_rs


def test_companion_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load_companion(HEADER)
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
    assert _lib.load_companion(HEADER) is L
    assert _lib.load_companion("threecrate_hip_alpha.h") is not L and _lib.load_companion("threecrate_hip_voxelmap.h") is not L


def _exported(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    return sorted(line.split()[-1] for line in out.splitlines() if re.search(r" T tc_\w+$", line))


def test_the_libraries_export_exactly_their_names(surface):
    declared = sorted(_lib.signatures(surface))
    assert _exported(os.path.join(LIBDIR, surface.library)) == declared and len(declared) == N_EXPORTS
    companions = [s.library for s in _lib.COMPANIONS + _lib.LATER_COMPANIONS + _lib.FURTHER_COMPANIONS if s.header != HEADER]
    assert len(companions) == 8
    for lib in [_lib.LIB_PATH, os.path.join(LIBDIR, "variants", "libthreecrate_hip_dev.so")] + [os.path.join(LIBDIR, c) for c in companions]:
        assert not set(_exported(lib)) & set(declared), lib
    assert _exported(os.path.join(LIBDIR, "libthreecrate_hip_alpha.so")) == sorted(_lib.ALPHA_EXPORTS) and len(_lib.ALPHA_EXPORTS) == 3
    product = sorted(n for s in _lib.SURFACES + _lib.EXTENSIONS for n in _lib.signatures(s))
    assert _exported(_lib.LIB_PATH) == product and len(product) == 115


def test_the_companion_is_linked_like_the_voxel_map(surface):
    """against the product library by name, found through $ORIGIN"""
    dyn = subprocess.check_output(["readelf", "-d", os.path.join(LIBDIR, surface.library)], text=True)
    assert re.search(r"NEEDED.*\[libthreecrate_hip\.so\]", dyn) and re.search(r"(RUNPATH|RPATH).*\[\$ORIGIN", dyn), dyn
    mk = open(os.path.join(LIBDIR, "csrc", "Makefile")).read()
    assert re.search(r"^clean:.*ground\.o.*\$\(GROUND_OUT\)", mk, re.M | re.S)
    assert re.search(r"^all:.*\$\(GROUND_OUT\)", mk, re.M) and "ground.hip" not in re.search(r"^SRCS = (.*)$", mk, re.M).group(1)
    assert re.search(r"^ground\.o:.*sym3_eigen\.h", mk, re.M)


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m, f"definition of {name} not found"
        assert m.group(1) and name not in TRIVIAL, name
    text = open(os.path.join(T.ROOT, "threecrate_amd", "csrc", "ground.hip")).read()
    assert text.count(") try {") == N_EXPORTS == len(re.findall(r"^\} TC_CATCH_(?:STATUS|VOID|VALUE)", text, re.M))


# ---- the compiled consumer ----
def _build(tmp, lang):
    exe = os.path.join(tmp, f"abi_ground_{lang}")
    cc = ["gcc", "-std=c11"] if lang == "c" else ["g++", "-std=c++17", "-x", "c++"]
    subprocess.check_call(cc + ["-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(T.ROOT, "include"), SRC, "-L", LIBDIR,
                                "-lthreecrate_hip_ground", "-lthreecrate_hip", f"-Wl,-rpath,{LIBDIR}", "-o", exe])
    return exe


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("abi_ground"))
    return {lang: _layout(_build(tmp, lang)) for lang in ("c", "cpp")}


def test_c_and_cpp_compilers_agree_and_the_null_calls_answer(layouts):
    lay = layouts["c"]
    assert lay == layouts["cpp"]
    assert lay["count.exports"] == N_EXPORTS
    for call in ("segment_null", "segment_device_null"):
        assert lay["call." + call] == lay["const.TC_INVALID_DATA"] == _lib.TC_INVALID_DATA, call
    assert lay["call.null_wrote"] == 0              # nothing is written without a context
    assert (lay["default.n_zones"], lay["default.height_ok"], lay["default.patches"], lay["default.null_patches"], lay["default.radii_ok"]) == (4, 1, 504, 0, 1)
    assert lay["const.TC_GROUND_MAX_ZONES"] == _lib.TC_GROUND_MAX_ZONES
    assert [lay["const.TC_GROUND_PATCH_" + s] for s in _lib.TC_GROUND_STATUS] == list(range(9))


def test_compiled_layouts_equal_the_ctypes_mirror(surface, layouts):
    lay, seen = layouts["c"], set()
    for name, cls in surface.structs.items():
        assert lay[f"sizeof.{name}"] == C.sizeof(cls) and lay[f"alignof.{name}"] == C.alignment(cls), name
        for fname, _ in cls._fields_:
            assert lay[f"offsetof.{name}.{fname}"] == getattr(cls, fname).offset, (name, fname)
            assert lay[f"fieldsize.{name}.{fname}"] == getattr(cls, fname).size, (name, fname)
            seen.add(f"offsetof.{name}.{fname}")
    assert {k for k in lay if k.startswith("offsetof.")} == seen
    assert (lay["sizeof.tc_ground_config"], lay["alignof.tc_ground_config"]) == (144, 4)
    assert (lay["sizeof.tc_ground_patch"], lay["alignof.tc_ground_patch"]) == (36, 4)
    import threecrate_amd as tc
    dt = tc.GpuContext.GROUND_PATCH_DTYPE
    assert dt.itemsize == 36 and {n: dt.fields[n][1] for n in dt.names} == {f: getattr(_lib.GroundPatchC, f).offset for f, _ in _lib.GroundPatchC._fields_}


def test_rust_structs_have_the_compiled_layout(surface, layouts):
    """the C layout rules applied to the #[repr(C)] structs of ffi_ground.rs (no Rust toolchain compiles the shim); `[T; N]` is N of T"""
    lay = layouts["c"]
    prim = {"f32": (4, 4), "u32": (4, 4), "u64": (8, 8)}

    def size_align(t):
        m = re.fullmatch(r"\[(\w+); (\d+)\]", t)
        if m:
            return prim[m.group(1)][0] * int(m.group(2)), prim[m.group(1)][1]
        return prim[t]

    rs = {}
    for m in re.finditer(r"#\[repr\(C\)\](?:\s*#\[derive\([^)]*\)\])?\s*pub struct (\w+)\s*\{([^}]*)\}", T.rust_text(RUST)):
        rs[m.group(1)] = [(fm.group(1),) + size_align(fm.group(2).strip()) for fm in re.finditer(r"pub (\w+)\s*:\s*(\[[^\]]+\]|[^,\[]+?)\s*(?:,|$)", m.group(2).strip())]
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
    from tests import ground_cases as GCASES

    L = _lib.load_companion(HEADER)
    fn = L.tc_segment_ground if road == "host" else L.tc_segment_ground_device
    I, U, OK = _lib.TC_INVALID_DATA, _lib.TC_UNSUPPORTED, _lib.TC_OK
    ctx = tc.GpuContext(0)
    try:
        message = lambda: _lib.load().tc_last_error_message(ctx._h).decode()
        dev = road == "device"
        points, cfg = GCASES.case("statuses")
        want = GCASES.expected("statuses")
        n = len(points)
        p = torch.from_numpy(np.array(points)).to("cuda:0") if dev else points
        labels = torch.full((n,), 7, dtype=torch.uint8, device="cuda:0") if dev else np.full(n, 7, np.uint8)
        ptr = lambda a: a.data_ptr() if dev else a.ctypes.data
        host = lambda a: a.cpu().numpy() if dev else a
        count = C.c_size_t(7)
        untouched = lambda: bool((host(labels) == 7).all()) and count.value == 7

        def call(c, n=n, p_ptr=True, l_ptr=True, n_ptr=True):
            if dev:
                torch.cuda.synchronize()
            return fn(ctx._h, ptr(p) if p_ptr else None, n, None if c is None else C.byref(c), ptr(labels) if l_ptr else None, None, None, None,
                      C.byref(count) if n_ptr else None)

        def config(**over):
            c = tc.GpuContext.ground_config(**cfg)
            for k, v in over.items():
                if isinstance(v, tuple):
                    getattr(c, k)[v[0]] = v[1]
                else:
                    setattr(c, k, v)
            return c

        every = dict(n_zones=0, zone_radii=(1, float("nan")), dist_threshold=0.0, num_seed_points=0, uprightness_threshold=2.0, num_rings=(0, 0))
        without = lambda *keys: config(**{k: v for k, v in every.items() if k not in keys})
        # 1 (the NULLs) before everything
        assert call(None, n=2 ** 40) == I and "config is NULL" in message()
        for kw in ({"l_ptr": False}, {"n_ptr": False}, {"p_ptr": False}):
            assert call(config(**every), n=2 ** 40, **kw) == I and "NULL" in message()
        # 2, validate_config in its order and with its messages, before 3 and 4
        assert call(config(**every), n=2 ** 40) == I and message() == "num_rings_per_zone must be non-empty"
        assert call(without("n_zones"), n=2 ** 40) == I and message() == "zone_radii must be strictly increasing"
        assert call(config(zone_radii=(1, 0.0)), n=2 ** 40) == I and message() == "zone_radii must be strictly increasing"      # equal radii
        assert call(without("n_zones", "zone_radii"), n=2 ** 40) == I and message() == "dist_threshold must be positive"
        assert call(without("n_zones", "zone_radii", "dist_threshold"), n=2 ** 40) == I and message() == "num_seed_points must be at least 1"
        assert call(without("n_zones", "zone_radii", "dist_threshold", "num_seed_points"), n=2 ** 40) == I and message() == "uprightness_threshold must be in (0, 1]"
        assert call(config(uprightness_threshold=0.0, num_rings=(0, 0)), n=2 ** 40) == I and message() == "uprightness_threshold must be in (0, 1]"
        # 3: the struct's own two conditions, too many zones first
        many = config(n_zones=9, num_rings=(0, 0))
        for z in range(9):
            many.zone_radii[z] = float(z)
        assert call(many, n=2 ** 40) == I and "TC_GROUND_MAX_ZONES" in message()
        assert call(config(num_rings=(0, 0)), n=2 ** 40) == I and "no ring or no sector" in message()
        assert call(config(num_sectors=(0, 0)), n=2 ** 40) == I and "no ring or no sector" in message()
        # 4: the patch count before the point count, each at its exact bound
        too_many = tc.GpuContext.ground_config(**GCASES.too_many_patches())
        assert call(too_many, n=2 ** 40) == U and "65536" in message()
        assert call(config(), n=2 ** 32 - 16) == U and "n is" in message()
        assert untouched()                                      # a failed call wrote nothing
        # 5: the empty cloud is fine, with or without points
        for kw in ({}, {"p_ptr": False}):
            count.value = 7
            assert call(config(), n=0, **kw) == OK and count.value == 0 and bool((host(labels) == 7).all())
        # and a full call on the same context afterwards
        assert call(config()) == OK and count.value == int(want["labels"].sum()) and np.array_equal(host(labels) != 0, want["labels"])
    finally:
        ctx.close()
