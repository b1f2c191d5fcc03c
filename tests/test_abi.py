"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/musicgan_hip.h declares (no compute
calls -- there is no GPU here); and the binding musicgan_amd/_lib.py derives from that header is the header's: the reader on a
header written for it, on the real one against expectations written by hand, the struct layouts against the host compiler's, and
every call site's argument count against the prototype it calls."""
import ast
import ctypes
import glob
import keyword
import os
import re
import subprocess
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "musicgan_hip.h")


def declared_symbols():
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mg_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_expected_surface():
    syms = declared_symbols()
    for must in ("mg_conv3x3", "mg_conv3x3_pack", "mg_conv3x3_wgrad", "mg_conv1x1", "mg_conv1x1_wgrad", "mg_adam_step",
                 "mg_stft_1024", "mg_pixelnorm_fwd", "mg_gp_finish", "mg_last_error"):
        assert must in syms
    assert len(syms) >= 28


def test_library_builds_loads_and_exports_every_declared_symbol():
    from musicgan_amd import _build, _lib
    path = _build.build()
    assert os.path.exists(path)
    lib = _lib.load()
    raw = ctypes.CDLL(path)
    for name in declared_symbols():
        assert hasattr(raw, name), f"{name} declared in include/musicgan_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes prototype in musicgan_amd/_lib.py"
    for name in _lib.SIGNATURES:
        assert name in declared_symbols(), f"{name} bound but not declared in the header"
    assert lib.mg_version() >= 100
    # pure host-side size queries are callable without a GPU
    assert lib.mg_conv3x3_packed_floats(64, 48) == 8 * 72 * 48
    assert lib.mg_conv3x3_packed_floats(8, 8) == 1 * 72 * 16
    assert lib.mg_conv3x3_wgrad_ws_bytes(64, 64, 48, 128, 128) > 0
    assert lib.mg_conv1x1_wgrad_ws_bytes(64, 2, 48, 128 * 128) > 0


def test_adam_descriptor_layout_matches_header():
    from musicgan_amd._lib import AdamTensor
    assert ctypes.sizeof(AdamTensor) == 48  # 4 pointers + int64 + 2 floats


def test_ops_refuse_cpu_tensors_loudly():
    import pytest
    import torch
    from musicgan_amd import _lib, ops
    from musicgan_amd.networks import Generator
    with pytest.raises(_lib.MusicGanHipError):
        ops.axpby(1.0, torch.zeros(4))
    gen = Generator(8)
    with pytest.raises(_lib.MusicGanHipError):
        gen(torch.zeros(1, 8, 2, 2), 1.0)


# ---------------------------------------------------------------- the reader of musicgan_amd/_lib.py on a header written for it
SYNTHETIC = r'''
/*
 * a top comment (with parentheses) and a look-alike inside it: int mg_foo(int x);
 */
#ifndef SYNTHETIC_H
#define SYNTHETIC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* mg_stream_t;
#define MG_A (-3)
#define MG_B 7    /* a comment that runs over a line end behind a backslash: mg_bar( \
                     and goes on here (as the one of MG_CONV_UNPOOL does) */
#define MG_C ( 12 )
enum { MG_E0 = 4, MG_E1, MG_E2 = -2, MG_E3,
       MG_E4 };
typedef struct {
  int32_t a, b, c;
  const float* in; /* a Python keyword */
  void* p;
  size_t n;
  uint8_t* bytes;
} mg_thing_t;
int mg_none(void);
const char* mg_text(void);
int64_t
mg_three_lines(const mg_thing_t* t, int64_t n, const unsigned char* bytes, /* mg_baz( */
               double d, float f, const char* path, uint32_t* crc,
               mg_stream_t stream);
size_t mg_size(int a,int32_t b);
#ifdef __cplusplus
}
#endif
#endif
'''


def _with(decl):
    return SYNTHETIC.replace("size_t mg_size(", decl + "\nsize_t mg_size(")


def test_reader_on_a_synthetic_header():
    from musicgan_amd import _lib
    constants, structs, signatures = _lib.read_header(SYNTHETIC)
    assert constants == {"MG_A": -3, "MG_B": 7, "MG_C": 12, "MG_E0": 4, "MG_E1": 5, "MG_E2": -2, "MG_E3": -1, "MG_E4": 0}
    assert structs == {"mg_thing_t": [("a", c_int32), ("b", c_int32), ("c", c_int32), ("in_", c_void_p), ("p", c_void_p),
                                      ("n", c_size_t), ("bytes", c_void_p)]}
    assert signatures == {
        "mg_none": (c_int, []),
        "mg_text": (c_char_p, []),
        "mg_three_lines": (c_int64, [c_void_p, c_int64, c_void_p, c_double, c_float, c_char_p, c_void_p, c_void_p]),
        "mg_size": (c_size_t, [c_int, c_int32]),
    }
    cls = _lib.struct_classes(structs, {"mg_thing_t": "Thing"})["Thing"]
    assert issubclass(cls, ctypes.Structure) and cls.__name__ == "Thing" and [f for f, _ in cls._fields_][3] == "in_"
    assert (cls.a.offset, cls.c.offset, cls.in_.offset, ctypes.sizeof(cls)) == (0, 8, 16, 48)
    with pytest.raises(_lib.MusicGanHipError, match="mg_thing_t"):
        _lib.struct_classes(structs)  # no class name for it in _lib.STRUCT_NAMES


@pytest.mark.parametrize("decl, says", [
    ("int mg_bad(const wchar_t* s);", "wchar_t"),                         # an unknown pointee
    ("int mg_bad(long n);", "long"),                                      # an unknown scalar
    ("uint8_t mg_bad(int n);", "uint8_t"),                                # known as a pointee only
    ("int mg_bad(const float** rows);", "rows"),                          # pointer to pointer
    ("int mg_bad(int (*callback)(int), int n);", "callback"),             # a function-pointer parameter
    ("int mg_bad(int n, float taps[11]);", "taps"),                       # an array declarator
    ("int mg_bad(int);", "mg_bad"),                                       # an unnamed parameter
    ("int mg_bad(const mg_other_t* d);", "mg_other_t"),                   # a struct the header does not define
    ("MG_DECLARE(mg_bad, int n);", "MG_DECLARE"),                         # a prototype generated by a macro
    ("extern int mg_counter;", "mg_counter"),                             # a declaration that is no prototype
    ("int mg_bad(int n) { return n; }", "mg_bad"),                        # a definition
    ("// int mg_bad(int n);", "mg_bad"),                                  # a line comment
    ("#define MG_BAD 1.5", "MG_BAD"),
    ("#define MG_BAD (1 << 4)", "MG_BAD"),
    ("#define MG_BAD(x) (x)", "MG_BAD"),
    ("#define MG_BAD", "MG_BAD"),
    ("enum { MG_BAD = MG_A + 1 };", "MG_BAD"),
    ("typedef struct { int32_t a; float* p, *q; } mg_bad_t;", "q"),
    ("typedef struct { long a; } mg_bad_t;", "long"),
])
def test_reader_refuses_what_it_does_not_understand(decl, says):
    from musicgan_amd import _lib
    with pytest.raises(_lib.MusicGanHipError, match=re.escape(says)):
        _lib.read_header(_with(decl))


# ---------------------------------------------------------------- the reader on the real header
def test_reader_finds_every_declared_symbol_and_the_awkward_ones_right():
    from musicgan_amd import _lib
    constants, structs, signatures = _lib.read_header(open(HEADER).read())
    assert sorted(signatures) == declared_symbols()
    assert signatures == _lib.SIGNATURES and set(structs) == set(_lib.STRUCT_NAMES)
    S = _lib.SIGNATURES
    assert S["mg_last_error"] == (c_char_p, [])
    assert S["mg_version"] == (c_int, []) and S["mg_loudness_chunk"] == (c_int, [])
    assert S["mg_resample_len"] == (c_int64, [c_int64, c_int, c_int])
    assert S["mg_resample_bank_size"] == (c_size_t, [c_int, c_int, c_int, c_double, c_void_p, c_void_p])
    assert S["mg_ssim_mean"] == (c_int, [c_void_p, c_int64, c_void_p, c_void_p])
    assert S["mg_ssim_tiles"] == (c_int64, [c_int, c_int])
    assert len(S["mg_vorbis_decode"][1]) == 23
    assert S["mg_axpby"] == (c_int, [c_float, c_void_p, c_float, c_void_p, c_void_p, c_size_t, c_void_p])
    assert S["mg_pt_write_samples"][1] == [c_void_p, c_int, c_int64, c_char_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64]
    assert S["mg_host_io_probe"][1][0] is c_char_p
    assert (_lib.MG_OK, _lib.MG_EINVAL, _lib.MG_ELAUNCH, _lib.MG_EWORKSPACE, _lib.MG_EIO) == (0, -1, -2, -3, -4)
    assert (_lib.MG_SN_LOAD, _lib.MG_SN_LINBWD, _lib.MG_SN_MAX_OPS, _lib.MG_PACK_WINOUPS) == (0, 11, 32, 5)
    assert (_lib.MG_CONV_UNPOOL, _lib.MG_CONV_UPSUM_OUT, _lib.MG_C1_ACCUM, _lib.MG_PCM_U8) == (128, 256, 32, 3)
    for name, value in constants.items():
        assert getattr(_lib, name) == value
    assert [f for f, _ in _lib.SnOp._fields_] == "op src dst C C2 H W flags in_ aux bias out out2".split()
    import poison  # reads and rewrites the pointers of SmallNet ops by field name on the GPU; the names are checked here
    assert [getattr(_lib.SnOp, f).offset for f in poison._SN_FIELDS] == [getattr(_lib.SnOp, f).offset for f, t in _lib.SnOp._fields_
                                                                         if t is c_void_p]  # `inp`: the older name of `in_`
    assert _lib.SnOp.inp is _lib.SnOp.in_ and set(poison._SN_WRITTEN) <= set(poison._SN_FIELDS)
    op = _lib.SnOp(0, 0, 0, 0, 0, 0, 0, 0, 1234)
    assert (op.inp, op.in_) == (1234, 1234)
    op.inp = 99
    assert op.in_ == 99
    for cname, pyname in _lib.STRUCT_NAMES.items():
        cls = getattr(_lib, pyname)
        assert issubclass(cls, ctypes.Structure) and cls._fields_ == structs[cname]


def _c_name(field):
    return field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field


def test_struct_layouts_are_the_host_compilers(tmp_path):
    """sizeof and every offsetof, printed by a program that includes the header, against the ctypes classes."""
    from musicgan_amd import _lib
    lines = []
    for cname, pyname in _lib.STRUCT_NAMES.items():
        lines.append(f'  std::printf("{pyname} sizeof %zu\\n", sizeof({cname}));')
        for field, _ in getattr(_lib, pyname)._fields_:
            lines.append(f'  std::printf("{pyname} {field} %zu\\n", offsetof({cname}, {_c_name(field)}));')
    src, exe = tmp_path / "layouts.cpp", tmp_path / "layouts"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "musicgan_hip.h"\nint main() {\n' + "\n".join(lines) +
                   "\n  return 0;\n}\n")
    subprocess.run(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    seen = 0
    for pyname, what, value in (ln.split() for ln in out if ln):
        cls = getattr(_lib, pyname)
        ours = ctypes.sizeof(cls) if what == "sizeof" else getattr(cls, what).offset
        assert ours == int(value), f"{pyname} {what}: ctypes {ours}, compiler {value}"
        seen += 1
    assert seen == len(lines) == sum(1 + len(getattr(_lib, p)._fields_) for p in _lib.STRUCT_NAMES.values()) and seen >= 7 + 63
    assert ctypes.sizeof(_lib.SnOp) == 72 and ctypes.sizeof(_lib.WgradDesc) == 80


# ---------------------------------------------------------------- call sites
# ctypes refuses a call with FEWER arguments than argtypes lists but passes surplus ones on by its default conversions (a Python
# integer as a 32-bit int), so nothing at run time notices a call site and a prototype that disagree in that direction.
# Calls that cannot be counted (*args, keywords): (file, enclosing function, entry point), each as often as it occurs.
UNCOUNTED = sorted([
    ("musicgan_amd/hpss_ops.py", "hpss", "mg_hpss"),
    ("tests/test_ema_gpu.py", "test_bad_arguments_are_refused_by_the_library", "mg_adam_step_dev_ema"),
    ("tests/test_ema_gpu.py", "test_bad_arguments_are_refused_by_the_library", "mg_adam_step_dev_ema"),
    ("tests/test_project_cpu.py", "test_plan_covers_every_plane_once", "mg_pyramid_l2_ws_bytes"),
    ("tests/test_project_cpu.py", "test_plan_refuses", "mg_pyramid_l2_ws_bytes"),
])


def _calls(node, func="<module>"):
    """(enclosing function, ast.Call) of every call under node whose callee is an attribute, e.g. lib.mg_axpby(...)."""
    for child in ast.iter_child_nodes(node):
        if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
            yield func, child
        yield from _calls(child, child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else func)


def test_call_sites_pass_as_many_arguments_as_the_header_declares():
    from musicgan_amd import _lib
    files = [os.path.join(ROOT, "bench.py")]
    for d in ("musicgan_amd", "tests", "tools"):
        files += glob.glob(os.path.join(ROOT, d, "**", "*.py"), recursive=True)
    counted, uncounted, reached, wrong = 0, [], set(), []
    for path in sorted(files):
        rel = os.path.relpath(path, ROOT).replace(os.sep, "/")
        for func, call in _calls(ast.parse(open(path).read(), path)):
            name = call.func.attr
            if name not in _lib.SIGNATURES:
                continue
            if call.keywords or any(isinstance(a, ast.Starred) for a in call.args):
                uncounted.append((rel, func, name))
                continue
            counted += 1
            reached.add(name)
            if len(call.args) != len(_lib.SIGNATURES[name][1]):
                wrong.append(f"{rel}:{call.lineno}: {name} called with {len(call.args)} arguments, the header declares "
                             f"{len(_lib.SIGNATURES[name][1])}")
    assert not wrong, "\n".join(wrong)
    assert sorted(uncounted) == UNCOUNTED
    # a walker that finds nothing proves nothing: 182 of the 184 entry points are called by name somewhere (mg_adam_step and
    # mg_conv3x3_wgrad_reduce go through a variable)
    assert len(reached) >= len(_lib.SIGNATURES) - 4 >= 180 and counted >= 250, (len(reached), counted)
