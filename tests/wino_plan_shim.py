"""The forward / data-gradient Winograd convolution's launch planner (musicgan_amd/csrc/wino_plan.h) on the CPU: a C shim around the
header, compiled by g++ into a shared object and called through ctypes.  The planner is plain host C++ with the layer, the CU count,
the strip kernel's workgroups per CU and the switches as arguments, so what it decides for any call, on any device size, can be
checked without a device."""
import ctypes
import os
import subprocess

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musicgan_amd", "csrc")

# the MG_CONV_* bits of include/musicgan_hip.h and the two internal ones of mg_wino3x3_fade (wino_plan.h); shim_flag checks them
FLAGS = {"LRELU": 2, "MASK_AUX": 4, "PIXNORM": 8, "POOL_OUT": 16, "MASK_OUT": 32, "MASK_BYTES": 64, "UNPOOL": 128, "BLEND": 256,
         "BLEND_BWD": 512}
LAYER = "N Cin Cout H W flags has_bias has_y".split()
SWITCHES = "cfg wt narrow narrow_wt few persist strip strip_niw strip_wgs strip_padw strip_min_blocks strip_ablate".split()
# one row of int64 per call: the layer, the strip plan (strip = 1: the strip kernel takes it), the staged plan (valid where strip = 0)
FIELDS = (LAYER + "strip niw nwave kind pool rows g_full g_pad grid lds ablate s_nchunk s_NT s_blocks_x s_blocks_y shape_ok "
          "status cfg wt narrow TBW TBH TBN lgTBW lgTBH blocks_x blocks_y blocks_n nchunk NT grid_x grid_y persistent st_lds "
          "mask_bytes_y".split())

SHIM = r'''
#include "wino_plan.h"
static WinoSwitches sw_of(const double* s) {
  WinoSwitches sw;
  sw.cfg = (int)s[0]; sw.wt = (int)s[1]; sw.narrow = s[2] != 0; sw.narrow_wt = (int)s[3]; sw.few = s[4] != 0; sw.persist = s[5] != 0;
  sw.strip = (int)s[6]; sw.strip_niw = (int)s[7]; sw.strip_wgs = (int)s[8]; sw.strip_padw = s[9]; sw.strip_min_blocks = (long long)s[10];
  sw.strip_ablate = (int)s[11];
  return sw;
}
extern "C" void shim_defaults(double* s) {
  const WinoSwitches sw;
  const double d[] = {(double)sw.cfg, (double)sw.wt, (double)sw.narrow, (double)sw.narrow_wt, (double)sw.few, (double)sw.persist,
                      (double)sw.strip, (double)sw.strip_niw, (double)sw.strip_wgs, sw.strip_padw, (double)sw.strip_min_blocks,
                      (double)sw.strip_ablate};
  for (int k = 0; k < 12; ++k) s[k] = d[k];
}
extern "C" int shim_unset() { return WINO_UNSET; }
extern "C" int shim_flag(int i) {
  const int f[] = {MG_CONV_LRELU, MG_CONV_MASK_AUX, MG_CONV_PIXNORM, MG_CONV_POOL_OUT, MG_CONV_MASK_OUT, MG_CONV_MASK_BYTES,
                   MG_CONV_UNPOOL, WF_BLEND, WF_BLEND_BWD};
  return f[i];
}
extern "C" int shim_kind(int i) {
  const int k[] = {SK_ACT, SK_ACT_POOL_MOUT, SK_MB_POOL, SK_MASKF, SK_UNPOOL, SK_BLEND_FWD, SK_BLEND_TAN, SK_BLEND_BWD, SK_PN, SK_MB_Y};
  return k[i];
}
// n calls {N, Cin, Cout, H, W, flags, has_bias, has_y}
extern "C" int shim_plan(const int* layer, int n, int n_cu, int per_cu, const double* s, long long* out) {
  const WinoSwitches sw = sw_of(s);
  for (int i = 0; i < n; ++i) {
    const int* l = layer + 8 * i;
    const WinoLayer L = {l[0], l[1], l[2], l[3], l[4], l[5], l[6] != 0, l[7] != 0};
    const WinoStripPlan p = wino_strip_plan(L, n_cu, per_cu, sw);
    const WinoStagedPlan q = p.takes ? WinoStagedPlan() : wino_staged_plan(L, n_cu, sw);
    const long long row[] = {l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7],
                             p.takes, p.niw, p.nwave, p.kind, p.pool, p.rows, p.g_full, p.g_pad, p.grid, (long long)p.lds, p.ablate,
                             p.nchunk, p.NT, p.blocks_x, p.blocks_y, wino_strip_shape_ok(L),
                             q.status, q.cfg, q.wt, q.narrow, q.TBW, q.TBH, q.TBN, q.lgTBW, q.lgTBH, q.blocks_x, q.blocks_y, q.blocks_n,
                             q.nchunk, q.NT, q.grid_x, q.grid_y, q.persistent, (long long)q.lds,
                             wino_mask_bytes_y_supported(l[0], l[1], l[2], l[3], l[4], sw)};
    if (out == nullptr) return (int)(sizeof(row) / sizeof(row[0]));  // the row's width
    const size_t w = sizeof(row) / sizeof(row[0]);
    for (size_t k = 0; k < w; ++k) out[(size_t)i * w + k] = row[k];
  }
  return 0;
}
'''

_lib = None


def load(tmp_dir):
    """Compile the shim (plain g++, no HIP header in reach) and load it; once per process."""
    global _lib
    if _lib is None:
        src, so = os.path.join(str(tmp_dir), "wino_plan_shim.cpp"), os.path.join(str(tmp_dir), "wino_plan_shim.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
        _lib = ctypes.CDLL(so)
        one = (ctypes.c_int * len(LAYER))(1, 16, 16, 16, 32, 0, 0, 1)
        assert _lib.shim_plan(one, 1, 256, 1, switches(_lib), None) == len(FIELDS)
        assert [_lib.shim_flag(i) for i in range(len(FLAGS))] == list(FLAGS.values())
    return _lib


def switches(lib, **kw):
    """The planner's switches as the shim takes them: the header's defaults, changed by keyword (strip=0, cfg=2, ...)."""
    s = (ctypes.c_double * len(SWITCHES))()
    lib.shim_defaults(s)
    for k, v in kw.items():
        s[SWITCHES.index(k)] = float(v)
    return s


class Plans:
    """Rows of FIELDS, one per call: p.strip, p.g_full, ... are int64 arrays."""

    def __init__(self, table):
        self.table = table

    def __getattr__(self, name):
        return self.table[:, FIELDS.index(name)]

    def __len__(self):
        return len(self.table)


def plan(lib, layers, n_cu, per_cu, sw):
    """layers: (n, 8) of LAYER."""
    layers = np.ascontiguousarray(layers, dtype=np.int32).reshape(-1, len(LAYER))
    out = np.zeros((len(layers), len(FIELDS)), dtype=np.int64)
    lib.shim_plan(layers.ctypes.data_as(ctypes.c_void_p), len(layers), int(n_cu), int(per_cu), sw, out.ctypes.data_as(ctypes.c_void_p))
    return Plans(out)


def layer_of(rec):
    """A census record of ops.conv3x3(..., wino=) or ops.conv3x3_fade as the library's entry point sees it -- LAYER -- with the flags
    derived as ops.conv3x3, ops._conv3x3_tilemask and ops.conv3x3_fade derive them; None for any other record."""
    name, r = rec[0], dict(rec[1])
    F = FLAGS
    if name == "conv3x3_fade":
        n, cin, h, w = r["x"]
        flags = {1: F["BLEND"] | F["LRELU"], 2: F["BLEND"] | F["MASK_AUX"] | F["MASK_BYTES"], 3: F["BLEND_BWD"]}[r["mode"]]
        return (n, cin, r["cout"], h, w, flags, int(r.get("bias") is not None), 1)
    if name != "conv3x3" or r.get("wino") is None:
        return None
    n, cin, h, w = r["x"]
    bias, mask_aux = int(r.get("bias") is not None), r.get("mask_aux")
    pool = bool(r.get("pool")) or r.get("pool_out") is not None
    u8 = lambda v: v is not None and v[0] == "u8"
    if r.get("unpool_mask") is not None:
        flags, bias, y = F["UNPOOL"], 0, 1
    elif r.get("mask_out") or u8(mask_aux):
        if not pool:
            flags, bias, y = F["MASK_AUX"] | F["MASK_BYTES"], 0, 1
        elif r.get("mask_out"):
            flags, y = F["LRELU"] | F["POOL_OUT"] | F["MASK_OUT"], 1
        else:
            flags, y = F["MASK_AUX"] | F["POOL_OUT"] | F["MASK_BYTES"], 0
    else:
        pn = bool(r.get("pixnorm"))
        flags = (F["LRELU"] if r.get("lrelu") else 0) | (F["MASK_AUX"] if mask_aux is not None else 0) | (F["PIXNORM"] if pn else 0) | \
            (F["POOL_OUT"] if pool else 0)
        y = int(r.get("out") is not None or r.get("want_y", True) or not pn)
    return (n, cin, r["cout"], h, w, flags, bias, y)
