"""The C ABI read as text: the declarations of a header of include/, those of a Rust declarations file of bindings/rust (no Rust
toolchain compiles the shim: the text is all there is), a C type spelled in Rust, and the definition of an entry point in csrc/.
One copy of each, for tests/test_abi_surfaces.py, test_abi_symbols.py and test_abi_conformance.py."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST_DIR = os.path.join(ROOT, "bindings", "rust", "threecrate-hip", "src")

# a C type has exactly one Rust spelling; pointers to the opaque / repr(C) structs keep their names (tc_* is spelled alike on both sides)
PRIMITIVES = {"float": "f32", "double": "f64", "int": "c_int", "int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "uint8_t": "u8",
              "size_t": "usize", "char": "c_char", "void": "c_void", "unsigned long long": "u64", "tc_status": "c_int",
              "tc_host_collective_fn": "tc_host_collective_fn"}


def header_text(name):
    """a header of include/ without its comments"""
    text = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def rust_text(name):
    return re.sub(r"//[^\n]*", "", open(os.path.join(RUST_DIR, name)).read())


def nparams(args):
    args = args.strip()
    return 0 if args in ("", "void") else args.count(",") + 1


def c2r(t):
    toks = t.replace("*", " * ").split()
    base_const = toks[0] == "const"
    toks = toks[1:] if base_const else toks
    cut = toks.index("*") if "*" in toks else len(toks)
    base, ptrs = " ".join(toks[:cut]), toks[cut:]
    r = PRIMITIVES.get(base, base)
    pointee_const = base_const
    i = 0
    while i < len(ptrs):                         # `*` [const]: a pointer whose Rust mutability is its POINTEE's constness
        assert ptrs[i] == "*", t
        r = ("*const " if pointee_const else "*mut ") + r
        pointee_const = i + 1 < len(ptrs) and ptrs[i + 1] == "const"
        i += 2 if pointee_const else 1
    return r


def c_sig(ret, args):
    out = []
    args = args.strip()
    for prm in ([] if args in ("", "void") else args.split(",")):
        prm = " ".join(prm.split())
        m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)(\[[A-Za-z0-9_]*\])?$", prm)
        out.append(c2r(m.group(1).strip() + (" *" if m.group(3) else "")))       # an array parameter is a pointer
    ret = " ".join(ret.split())
    return out, ("" if ret == "void" else c2r(ret))


def r_sig(args, ret):
    norm = lambda t: " ".join(t.split()).replace("std::os::raw::", "")
    return [norm(x.split(":", 1)[1]) for x in args.split(",") if x.strip()], norm((ret or "").replace("->", ""))


def header_decls(name):
    """{function: (parameter count, (parameter types, return type) in their Rust spelling)} of a header, in its order"""
    return {m.group(2): (nparams(m.group(3)), c_sig(m.group(1), m.group(3)))
            for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(tc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text(name))}


def header_structs(name):
    """{struct: [field names, in order]} of the structs a header defines (the opaque handles have no body)"""
    return {m.group(1): re.findall(r"(\w+)(?:\[\w+\])?\s*[,;]", m.group(2))       # `double total_ms, min_ms, max_ms;` is three fields
            for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} \1;", header_text(name), re.S)}


def rust_decls(name):
    """the same of a Rust declarations file"""
    return {m.group(1): (nparams(m.group(2)), r_sig(m.group(2), m.group(3)))
            for m in re.finditer(r"pub fn (tc_[a-z0-9_]+)\s*\(([^()]*)\)\s*(->\s*[^;]+)?;", rust_text(name))}


def csrc_text():
    return "\n".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "threecrate_amd", "csrc", "*.hip"))))


def definition(name, src):
    """the match of an entry point's definition in the .hip text; group 1 is its `try ` when the body is a function-try-block"""
    return re.search(r"^[^\n/]*\b" + name + r"\([^;{]*\)\s*(try )?\{", src, re.M)
