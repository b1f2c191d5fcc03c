"""ctypes binding of libmusicgan_hip.so, derived at import from include/musicgan_hip.h.

The header is the single description of the C ABI: every prototype in it becomes an entry of SIGNATURES, every struct a
ctypes.Structure and every MG_* constant an attribute of this module.  A new entry point is declared there and nowhere else; a
declaration this reader does not fully understand raises at import, it is never skipped.

There is NO CPU or eager-PyTorch fallback: if the library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes
import keyword
import os
import re

import torch  # noqa: F401  -- must be imported BEFORE the library: both link libamdhip64.so.7 and the HIP runtime that
#                             torch ships has to be the one the process binds (loading /opt/rocm's first breaks torch's device)
from ctypes import c_char_p, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmusicgan_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "musicgan_hip.h")


class MusicGanHipError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char", "uint8_t", "uint32_t"}
# [const] type [*] name -- a parameter, a struct field, or a function's return type and name
_DECL = re.compile(r"(?:const\s+)?(unsigned\s+char|\w+)(?:\s*(\*)\s*|\s+)(\w+)")
# the Python classes of the header's structs; a struct without an entry is an error
STRUCT_NAMES = {"mg_adam_tensor_t": "AdamTensor", "mg_adam_tensor_dev_t": "AdamTensorDev",
                "mg_adam_tensor_dev_ema_t": "AdamTensorDevEma", "mg_wgrad_job_t": "WgradJob", "mg_wgrad_desc_t": "WgradDesc",
                "mg_pack_desc_t": "PackDesc", "mg_sn_op_t": "SnOp"}


def _bad(what: str, text: str):
    return MusicGanHipError(f"include/musicgan_hip.h: {what}: {' '.join(text.split())!r}")


def _ctype(base: str, star: str, structs, text: str):
    """Scalars by the table; mg_stream_t and every pointer c_void_p, except [const] char* which is c_char_p."""
    base = " ".join(base.split())
    if star:
        if base not in _POINTEES and base not in structs:
            raise _bad(f"unknown type {base}*", text)
        return c_char_p if base == "char" else c_void_p
    if base == "mg_stream_t":
        return c_void_p
    if base not in _SCALARS:
        raise _bad(f"unknown type {base}", text)
    return _SCALARS[base]


def read_header(text: str):
    """(constants, structs, signatures) of a header in the grammar the top comment of include/musicgan_hip.h states:
    {MG_X: int}, {mg_x_t: [(field, ctype)]} and {mg_name: (restype, [argtypes])}."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S).replace("\\\n", " ")
    constants, structs, signatures, rest = {}, {}, {}, []
    for line in text.split("\n"):
        m = re.match(r"\s*#\s*define\s+(MG_\w+)(.*)", line)
        if m:
            v = re.fullmatch(r"\s+(?:\(\s*(-?\d+)\s*\)|(-?\d+))\s*", m.group(2))
            if not v:
                raise _bad("#define MG_* that is not an integer", line)
            constants[m.group(1)] = int(v.group(1) or v.group(2))
        elif not line.lstrip().startswith("#"):
            rest.append(line)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", "\n".join(rest), flags=re.S)

    def enum(m):
        value = -1
        for item in filter(None, (s.strip() for s in m.group(1).split(","))):
            e = re.fullmatch(r"(MG_\w+)(?:\s*=\s*(-?\d+))?", item)
            if not e:
                raise _bad("enumerator", item)
            value = constants[e.group(1)] = int(e.group(2)) if e.group(2) else value + 1
        return ""

    def struct(m):
        fields = []
        for decl in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *more = (s.strip() for s in decl.split(","))
            d = _DECL.fullmatch(first)
            if not d or not all(re.fullmatch(r"\w+", n) for n in more):
                raise _bad("struct field", decl)
            ctype = _ctype(d.group(1), d.group(2), structs, decl)
            fields += [(n + "_" if keyword.iskeyword(n) else n, ctype) for n in (d.group(3), *more)]
        structs[m.group(2)] = fields
        return ""

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    *statements, tail = text.split(";")
    if tail.strip():
        raise _bad("declaration", tail)
    for stmt in statements:
        if re.fullmatch(r"\s*typedef\s+void\s*\*\s*mg_stream_t\s*", stmt):
            continue
        m = re.fullmatch(r"\s*(.*?)\s*\((.*)\)\s*", stmt, flags=re.S)
        head = m and _DECL.fullmatch(m.group(1))
        if not head or not head.group(3).startswith("mg_"):
            raise _bad("declaration", stmt)
        argtypes = []
        if m.group(2).strip() != "void":
            for param in m.group(2).split(","):
                p = _DECL.fullmatch(param.strip())
                if not p:
                    raise _bad(f"parameter {' '.join(param.split())!r} of", stmt)
                argtypes.append(_ctype(p.group(1), p.group(2), structs, stmt))
        void = head.group(1) == "void" and not head.group(2)
        signatures[head.group(3)] = (None if void else _ctype(head.group(1), head.group(2), structs, stmt), argtypes)
    return constants, structs, signatures


def struct_classes(structs, names=STRUCT_NAMES):
    """{Python class name: ctypes.Structure} for the structs of read_header, fields under their C names."""
    missing = sorted(set(structs) - set(names))
    if missing:
        raise MusicGanHipError(f"include/musicgan_hip.h: struct(s) {', '.join(missing)} have no class name in _lib.STRUCT_NAMES")
    return {names[c]: type(names[c], (ctypes.Structure,), {"_fields_": fields}) for c, fields in structs.items()}


with open(HEADER_PATH) as _f:
    _constants, _structs, SIGNATURES = read_header(_f.read())  # SIGNATURES: name -> (restype, argtypes)
globals().update(_constants)
globals().update(struct_classes(_structs))
SnOp.inp = SnOp.in_  # noqa: F821 -- mg_sn_op_t.in under the name it had before the binding was derived; tests/poison.py reads it

_lib = None


def load() -> ctypes.CDLL:
    """Load the shared library (once).  Raises MusicGanHipError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MusicGanHipError(
            f"{LIB_PATH} not found: build it with `python -m musicgan_amd._build` (hipcc, gfx950). "
            "musicgan_amd has no CPU / eager fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == ABI mismatch, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mg_last_error()
        raise MusicGanHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")
