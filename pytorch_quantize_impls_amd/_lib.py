"""ctypes binding of libqt_hip.so (the C-ABI declared in include/qt_hip.h).

The shared library is built IN-TREE (pytorch_quantize_impls_amd/lib/libqt_hip.so) by
``__graft_entry__.build()`` / ``make -C pytorch_quantize_impls_amd/csrc``.  There is no fallback:
if the library is missing or a symbol is absent, every GPU op raises ``QtLibraryError``.

include/qt_hip.h is the only statement of the ABI: it is parsed once at import into ``SIGNATURES`` (the restype and
argtypes every entry point gets in ``load()``), ``DEFINES`` (the QT_* integer constants) and ``STRUCTS`` (the ``_fields_`` of
the structures passed by pointer).  A new entry point is declared in the header and defined under csrc/; nothing is added here.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
from collections import Counter
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
# QT_HIP_LIB: A/B builds of the same ABI (tools/); the product path is the in-tree library
LIB_PATH = os.environ.get("QT_HIP_LIB") or os.path.join(_HERE, "lib", "libqt_hip.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "qt_hip.h"))


class QtLibraryError(RuntimeError):
    """libqt_hip.so could not be loaded (not built, wrong arch, missing symbol)."""


class QtStatusError(RuntimeError):
    """A C-ABI entry point returned a negative qt_status."""


class Header(NamedTuple):
    """What parse_header() reads out of the text of include/qt_hip.h."""
    functions: dict     # name -> (restype, [(parameter name, ctype), ...]), in declaration order
    defines: dict       # "QT_<NAME>" -> int, every #define of an integer literal
    structs: dict       # name -> [(field, ctype), ...]: a ctypes.Structure's _fields_


# The whole type map of the C-ABI.  Any pointer but (const) char* is a c_void_p; every other spelling is an error.
_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "qt_stream_t": ctypes.c_void_p}


def _strip_comments(text: str) -> str:
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _loose_function_names(stripped: str):
    return sorted(set(re.findall(r"\b(qt_[a-z0-9_]+)\s*\(", stripped)))


def _ctype(spelling: str, where: str):
    words = [w for w in spelling.replace("*", " * ").split() if w != "const"]
    if len(words) == 1 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    if len(words) >= 2 and re.fullmatch(r"\w+", words[0]) and set(words[1:]) == {"*"}:
        return ctypes.c_char_p if words == ["char", "*"] else ctypes.c_void_p
    raise QtLibraryError(f"{where}: the type '{spelling.strip()}' is not in the binding's type map")


def _declarators(decl: str, where: str):
    """'int64_t ld, rows, K' -> [("ld", c_int64), ("rows", c_int64), ("K", c_int64)]."""
    m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)", decl.strip())
    if not m:
        raise QtLibraryError(f"{where}: cannot parse '{decl.strip()}'")
    names = [n.strip() for n in m.group(2).split(",")]
    if len(names) > 1 and "*" in m.group(1):      # in C the star of 'float* a, b' binds to a alone
        raise QtLibraryError(f"{where}: several declarators of a pointer type in '{decl.strip()}'")
    ctype = _ctype(m.group(1), where)
    return [(n, ctype) for n in names]


def parse_header(text: str, source: str = "header") -> Header:
    """Functions, integer #defines and structs of a C header written like include/qt_hip.h.  Everything that is left after the
    comments, preprocessor lines, enums, the qt_stream_t typedef and the extern "C" braces must be a struct typedef or a
    prototype over the closed type map: anything else raises QtLibraryError, so no declaration is dropped quietly."""
    text = _strip_comments(text)
    loose = _loose_function_names(text)
    defines = {name: int(value, 0) for name, value in
               re.findall(r"^[ \t]*#[ \t]*define[ \t]+(QT_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M)
    structs = {}

    def take_struct(m):
        name, where = m.group(1), f"{source}: struct {m.group(1)}"
        structs[name] = [f for decl in m.group(2).split(";") if decl.strip() for f in _declarators(decl, where)]
        return ""

    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", take_struct, text)
    text = re.sub(r"(?:typedef\s+)?enum\b[^{};]*\{[^{}]*\}[^;]*;", "", text)
    text = re.sub(r"typedef\s+void\s*\*\s*qt_stream_t\s*;", "", text)
    text, n_extern = re.subn(r'extern\s+"C"\s*\{', "", text)
    *statements, tail = text.split(";")
    if "".join(tail.split()) != "}" * n_extern:
        raise QtLibraryError(f"{source}: cannot parse the end of the header '{tail.strip()}'")
    functions = {}
    for stmt in statements:
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = re.fullmatch(r"(.*?[\s*])(qt_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        if not m or m.group(2) in functions:
            raise QtLibraryError(f"{source}: cannot parse the declaration '{stmt}'")
        ret, name, params = m.groups()
        where = f"{source}: {name}()"
        params = [] if params.strip() == "void" else [d for p in params.split(",") for d in _declarators(p, where)]
        functions[name] = (_ctype(ret, where), params)
    if sorted(functions) != loose:
        raise QtLibraryError(f"{source}: parsed functions differ from the names the header mentions: "
                             f"{sorted(set(functions) ^ set(loose))}")
    return Header(functions, defines, structs)


def _read_header(header_path: str) -> str:
    try:
        with open(header_path, "r", encoding="utf-8") as fh:
            return fh.read()
    except OSError as e:
        raise QtLibraryError(f"cannot read the C-ABI header {header_path}: {e}") from e


def header_declared_functions(header_path: str = HEADER_PATH):
    """Names of all functions declared in include/qt_hip.h (comments stripped): a loose scan that knows no types, which
    parse_header() has to agree with."""
    return _loose_function_names(_strip_comments(_read_header(header_path)))


HEADER = parse_header(_read_header(HEADER_PATH), HEADER_PATH)
DEFINES = HEADER.defines
STRUCTS = HEADER.structs
#: name -> (restype, argtypes) of every function include/qt_hip.h declares
SIGNATURES = {name: (restype, [ctype for _, ctype in params]) for name, (restype, params) in HEADER.functions.items()}

_lock = threading.Lock()
_lib = None
#: number of successful calls per entry point in this process — the GPU tests assert on it so a
#: silent non-HIP path cannot pass them.
call_counts: Counter = Counter()


def load():
    """Load (once) and return the ctypes handle.  Raises QtLibraryError loudly on any problem."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise QtLibraryError(
                f"{LIB_PATH} not found: the HIP extension is not built. Run "
                "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                "pytorch_quantize_impls_amd/csrc`). There is no CPU/PyTorch fallback for GPU tensors.")
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover - depends on the box
            raise QtLibraryError(f"cannot dlopen {LIB_PATH}: {e}") from e
        for name, (restype, argtypes) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise QtLibraryError(f"{LIB_PATH} does not export {name}") from e
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def is_built() -> bool:
    return os.path.exists(LIB_PATH)


def strerror(code: int) -> str:
    return load().qt_strerror(int(code)).decode()


def call(name: str, *args) -> None:
    """Invoke an int-returning entry point and raise on a negative status."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise QtStatusError(f"{name} failed: {strerror(rc)} (qt_status {rc})")
    call_counts[name] += 1


def version() -> int:
    return int(load().qt_version())


def target_arch() -> str:
    return load().qt_target_arch().decode()


def device_info():
    buf = ctypes.create_string_buffer(64)
    cus = load().qt_device_info(buf, 64)
    if cus < 0:
        raise QtStatusError(f"qt_device_info failed: {strerror(cus)}")
    return buf.value.decode(), int(cus)
