"""The contract of every ABI surface, once: an entry of _lib.SURFACES (a header of include/, its Rust declarations file, its ctypes
rows) is held to its header, its Rust file, the other surfaces, the loaded library and the function-try-block rule of
tests/test_abi_exceptions.py.  A new header is one more entry in _lib.SURFACES, a Rust file, and one count in EXPORT_COUNTS below;
the layouts of its structs are compiled and compared in tests/test_abi_conformance.py.  No compute calls: this runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from threecrate_amd import _lib
from tests import abi_text as T

# the one place that says how many functions each header declares, and which ABI version the library answers
EXPORT_COUNTS = {"threecrate_hip.h": 90, "threecrate_hip_filters.h": 6, "threecrate_hip_segmentation.h": 4, "threecrate_hip_ndt.h": 4}
ABI_VERSION = 2

# entry points whose whole body is one expression that cannot throw (plain member reads / constants / delete of a POD holder)
TRIVIAL = {"tc_abi_version", "tc_last_error_message", "tc_icp_shard_sums", "tc_icp_shard_destroy", "tc_cloud_size",
           "tc_cloud_points_device", "tc_comm_rank", "tc_comm_size", "tc_search_index_size", "tc_profile_enable"}


@pytest.fixture(params=_lib.SURFACES, ids=[s.header for s in _lib.SURFACES])
def surface(request):
    return request.param


def test_counts_and_version():
    assert list(EXPORT_COUNTS) == [s.header for s in _lib.SURFACES]
    assert sum(EXPORT_COUNTS.values()) == 104
    assert _lib.load().tc_abi_version() == ABI_VERSION


def test_header_table_and_rust_declare_the_same_functions(surface):
    h, r, t = T.header_decls(surface.header), T.rust_decls(surface.rust), _lib.signatures(surface)
    assert len(h) == len(t) == EXPORT_COUNTS[surface.header]
    assert sorted(h) == sorted(t), sorted(set(h) ^ set(t))
    assert sorted(r) == sorted(h), sorted(set(h) ^ set(r))
    counts = {name: n for name, (n, _) in h.items()}
    assert {name: n for name, (n, _) in r.items()} == counts
    assert {name: len(argtypes or ()) for name, (_, argtypes) in t.items()} == counts
    # the table's return type is the header's (a pointer other than a string comes back as an address)
    restype = {"": None, "c_int": C.c_int, "usize": C.c_size_t, "u64": C.c_ulonglong, "*const c_char": C.c_char_p}
    for name, (_, (_, ret)) in h.items():
        assert t[name][0] is restype.get(ret, C.c_void_p if ret.startswith("*") else ret), (name, ret)
    # a host entry point and its device twin take the same list
    for name in h:
        if name + "_device" in h:
            assert h[name + "_device"] == h[name], name


def test_header_and_rust_agree_on_every_type(surface):
    """parameter by parameter and for the return value: what a `bindgen` run + a Rust compile would check"""
    h, r = T.header_decls(surface.header), T.rust_decls(surface.rust)
    bad = {k: (h[k][1], r[k][1]) for k in h if k not in r or h[k][1] != r[k][1]}
    assert not bad, bad


def test_structs_are_the_headers_field_by_field(surface):
    """the structs of an entry are the ones ITS header defines, with the header's field names in the header's order
    (sizes and offsets: the compiled layouts of tests/test_abi_conformance.py)"""
    mirror = {name: [f[0] for f in cls._fields_] for name, cls in surface.structs.items()}
    assert mirror == T.header_structs(surface.header)


def test_surfaces_stay_apart(surface):
    names = set(_lib.signatures(surface))
    lib_rs = open(os.path.join(T.RUST_DIR, "lib.rs")).read()
    for other in _lib.SURFACES:
        if other is not surface:
            assert not names & set(_lib.signatures(other)), other.header
            text = T.header_text(other.header)            # (their comments may speak of tc_abi_version())
            assert not [n for n in names if re.search(r"\b" + n + r"\b", text)], other.header
    mod = surface.rust[:-len(".rs")]
    assert re.search(r"^pub mod " + mod + ";", lib_rs, re.M)
    # every call of this file's functions in lib.rs names a declared function
    used = set(re.findall(r"\b" + mod + r"::(tc_[a-z0-9_]+)\(", lib_rs))
    assert used <= set(T.rust_decls(surface.rust)), used - set(T.rust_decls(surface.rust))


def test_library_has_every_symbol_with_the_tables_types(surface):
    L = _lib.load()
    for name, (restype, argtypes) in _lib.signatures(surface).items():
        fn = getattr(L, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name


def test_every_export_is_a_function_try_block(surface):
    src = T.csrc_text()
    unguarded = []
    for name in _lib.signatures(surface):
        m = T.definition(name, src)
        assert m, f"definition of {name} not found"
        if name == "tc_comm_create_local":        # delegates to a guarded entry point
            continue
        if not m.group(1) and name not in TRIVIAL:
            unguarded.append(name)
    assert not unguarded, f"extern \"C\" entry points without a function-try-block: {unguarded}"


def test_every_try_block_of_an_entry_point_is_closed_by_a_handler_macro():
    src = T.csrc_text()
    assert src.count(") try {") == len(re.findall(r"^\} TC_CATCH_(STATUS|VOID|VALUE)|\} TC_CATCH_STATUS\(", src, re.M))
