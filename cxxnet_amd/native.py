"""Loaders for the in-tree native libraries.

* ``rt()``      -> the pybind11 runtime module (config parser, NetConfig, IO, metrics).
* ``kernels()`` -> ctypes handle on ``libcxxnet_kernels.so`` (all HIP kernels, gfx950).

Both are built in-tree by ``cxxnet_amd.build``.  On a machine with a GPU the
kernel library is mandatory: a missing library raises instead of silently
falling back to another implementation.

The kernel library's C ABI is declared once, in ``csrc/kernels/cxn_api.h``.  The compiler checks
every definition against that header, and this module reads the same text for the ``argtypes`` /
``restype`` of every ``cxn_*`` entry point and the fields of ``CxnOperand``: a new entry point
needs its prototype there and nothing here.
"""
from __future__ import annotations

import ctypes
import importlib.machinery
import importlib.util
import os
import re
import sysconfig
import threading

_PKG = os.path.dirname(os.path.abspath(__file__))
_NATIVE = os.environ.get("CXXNET_NATIVE_DIR") or os.path.join(_PKG, "_native")
if not os.path.isabs(_NATIVE):
    _NATIVE = os.path.abspath(_NATIVE)
_lock = threading.Lock()
_rt = None
_k = None


def _load_ext(name: str, path: str):
    loader = importlib.machinery.ExtensionFileLoader(name, path)
    spec = importlib.util.spec_from_file_location(name, path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    return mod


def rt():
    """The native runtime module (builds it on first use if absent)."""
    global _rt
    if _rt is None:
        with _lock:
            if _rt is None:
                path = os.path.join(_NATIVE, "_cxxnet_rt" + sysconfig.get_config_var("EXT_SUFFIX"))
                if not os.path.exists(path):
                    from . import build
                    build.build_runtime()
                _rt = _load_ext("_cxxnet_rt", path)
    return _rt


# Reader of cxn_api.h.  The header's grammar is narrow on purpose (see its head comment): whatever
# the reader does not recognise raises ValueError, it never guesses a type.
_HEADER = os.path.join(_PKG, "csrc", "kernels", "cxn_api.h")
_SCALAR = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float,
           "uint32_t": ctypes.c_uint, "unsigned": ctypes.c_uint}
_RETURN = {"int": ctypes.c_int, "long": ctypes.c_long, "void *": ctypes.c_void_p, "void": None}
_NOISE = re.compile(r"//[^\n]*|^[ \t]*#[^\n]*|static_assert\([^;]*;", re.M)  # comments, # lines, static_asserts
_STRUCT = re.compile(r"struct\s+CxnOperand\s*\{([^{}]*)\}\s*;")
_PROTO = re.compile(r"CXN_API\s+([\w\s*]+?)\s*\b(cxn_\w+)\s*\(([^()]*)\)\s*;\s*")


def _norm(ctype: str) -> str:
    return " ".join(ctype.replace("*", " * ").split())


def _decl(decl: str, where: str):
    """(name, ctypes type) of one ``<type> <name>`` parameter or member of ``where``."""
    m = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", decl, re.S)
    ctype, name = (_norm(m.group(1)), m.group(2)) if m else ("", "")
    if name and name not in _SCALAR and name not in ("const", "void"):
        if ctype in _SCALAR:
            return name, _SCALAR[ctype]
        if ctype.endswith("*") and re.fullmatch(r"[\w\s*]+", ctype):
            is_operand = [t for t in ctype.split() if t != "const"] == ["CxnOperand", "*"]
            return name, ctypes.POINTER(CxnOperand) if is_operand else ctypes.c_void_p
    raise ValueError(f"cxn_api.h: {where}: cannot map declaration {' '.join(decl.split())!r}")


def _read_struct(text: str):
    """The ``_fields_`` of CxnOperand from the header's one ``struct CxnOperand { ... };``."""
    found = _STRUCT.findall(_NOISE.sub("", text))
    if len(found) != 1:
        raise ValueError(f"cxn_api.h: expected one struct CxnOperand, found {len(found)}")
    return [_decl(member, "struct CxnOperand") for member in found[0].split(";") if member.strip()]


def _read_protos(text: str):
    """{entry point: (argtypes, restype)} from the header's prototypes; nothing else may stand between them."""
    text = _STRUCT.sub("", _NOISE.sub("", text)).strip()
    api, pos = {}, 0
    while pos < len(text):
        m = _PROTO.match(text, pos)
        if not m:
            raise ValueError(f"cxn_api.h: not a prototype: {' '.join(text[pos:].split(';')[0].split())[:200]!r}")
        ret, name, params = _norm(m.group(1)), m.group(2), m.group(3)
        if ret not in _RETURN:
            raise ValueError(f"cxn_api.h: {name}: cannot map return type {ret!r}")
        if name in api:
            raise ValueError(f"cxn_api.h: {name}: declared twice")
        api[name] = ([_decl(p, name)[1] for p in params.split(",")] if params.strip() else [], _RETURN[ret])
        pos = m.end()
    return api


with open(_HEADER) as _f:
    _header_text = _f.read()


class CxnOperand(ctypes.Structure):
    _fields_ = _read_struct(_header_text)


_API = _read_protos(_header_text)


def kernel_lib_path() -> str:
    return os.path.join(_NATIVE, "libcxxnet_kernels.so")


def kernels():
    """ctypes handle on the HIP kernel library; raises if it cannot be loaded."""
    global _k
    if _k is None:
        with _lock:
            if _k is None:
                path = kernel_lib_path()
                if not os.path.exists(path):
                    from . import build
                    build.build_kernels()
                lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
                for name, (args, res) in _API.items():
                    fn = getattr(lib, name)
                    fn.argtypes = args
                    fn.restype = res
                _k = lib
    return _k


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"cxxnet_amd kernel {what} failed (rc={rc})")
