"""The weight gradient's launch planner (musicgan_amd/csrc/wino_wgrad_plan.h) on the CPU: a C shim around the header, compiled by g++
into a shared object and called through ctypes.  The planner is plain host C++ with the CU count and the switches as arguments, so
what it decides for any layer or sweep, on any device size, can be checked without a device."""
import ctypes
import os
import subprocess

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "musicgan_amd", "csrc")

# one row of int64 per layer
FIELDS = ("N Cin Cout H W TBW TBH TBN lgTBW lgTBH blocks_x blocks_y blocks_n nblk per CinP CoutP nob "
          "CT OT ncb nsplit nsplit_ws ws_floats rows small var fast group form reduce_lanes reduce_blocks").split()

SHIM = r'''
#include "wino_wgrad_plan.h"
static WwSwitches sw_of(const int* s) {  // rows, rows_ups, ablate, fast, group_fixed, group_slots_q
  WwSwitches sw;
  sw.rows = s[0]; sw.rows_ups = s[1] != 0; sw.ablate = s[2]; sw.fast = s[3] != 0; sw.group_fixed = s[4]; sw.group_slots_q = s[5];
  return sw;
}
extern "C" void shim_defaults(int* s) {
  const WwSwitches sw;
  s[0] = sw.rows; s[1] = sw.rows_ups; s[2] = sw.ablate; s[3] = sw.fast; s[4] = sw.group_fixed; s[5] = sw.group_slots_q;
}
extern "C" int shim_limits(int what) { return what == 0 ? WW_GROUP : WW_MAX_LAYERS; }
// `total` layers {N, Cin, Cout, H, W, ups} in sweeps of `per_sweep` consecutive ones; returns the number of sweeps or layers whose
// plan broke the workspace invariant
extern "C" int shim_sweeps(const int* shape, int total, int per_sweep, int group_max_chunks, int n_cu, const int* s, long long* out) {
  const WwSwitches sw = sw_of(s);
  int broken = 0;
  for (int first = 0; first < total; first += per_sweep) {
    const int n = total - first < per_sweep ? total - first : per_sweep;
    WwSweep S;
    for (int i = 0; i < n; ++i) {
      const int* L = shape + 6 * (first + i);
      if (!ww_plan_layer(L[0], L[1], L[2], L[3], L[4], L[5] != 0, group_max_chunks, n_cu, sw, S.pl[i])) ++broken;
    }
    if (!ww_plan_groups(S, n, n_cu, sw)) ++broken;
    for (int i = 0; i < n; ++i) {
      const int* L = shape + 6 * (first + i);
      const WwPlan& p = S.pl[i];
      const WwGeo& a = p.a;
      const int total_e = a.CinP * a.CoutP;
      const long long row[] = {a.N, a.Cin, a.Cout, a.H, a.W, a.TBW, a.TBH, a.TBN, a.lgTBW, a.lgTBH, a.blocks_x, a.blocks_y, a.blocks_n,
                               a.nblk, a.per, a.CinP, a.CoutP, a.nob, p.CT, p.OT, p.ncb, p.nsplit, p.nsplit_ws, (long long)p.ws_floats,
                               p.rows, p.small, p.var, S.group_of[i] < 0 && !p.rows && ww_fast(a, sw), S.group_of[i],
                               ww_form(L[0], L[1], L[2], L[3], L[4], L[5] != 0, group_max_chunks, n_cu, sw),
                               ww_reduce_lanes(p.nsplit, total_e), ww_reduce_blocks(p.nsplit, total_e)};
      for (unsigned k = 0; k < sizeof(row) / sizeof(row[0]); ++k) out[(size_t)(first + i) * (sizeof(row) / sizeof(row[0])) + k] = row[k];
    }
  }
  return broken;
}
extern "C" int shim_var(int CT, int OT, int ups) { return ww_var(CT, OT, ups != 0); }
'''

_lib = None


def load(tmp_dir):
    """Compile the shim (plain g++, no HIP header in reach) and load it; once per process."""
    global _lib
    if _lib is None:
        src, so = os.path.join(str(tmp_dir), "wgrad_plan_shim.cpp"), os.path.join(str(tmp_dir), "wgrad_plan_shim.so")
        with open(src, "w") as f:
            f.write(SHIM)
        subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, src, "-o", so], check=True)
        _lib = ctypes.CDLL(so)
    return _lib


def switches(lib, **kw):
    """The planner's switches as the shim takes them: the header's defaults, changed by keyword (rows=0, fast=0, ...)."""
    s = (ctypes.c_int * 6)()
    lib.shim_defaults(s)
    names = ["rows", "rows_ups", "ablate", "fast", "group_fixed", "group_slots_q"]
    for k, v in kw.items():
        s[names.index(k)] = int(v)
    return s


class Plans:
    """Rows of FIELDS, one per layer: p.nsplit, p.rows, ... are int64 arrays."""

    def __init__(self, table, broken):
        self.table, self.broken = table, broken

    def __getattr__(self, name):
        return self.table[:, FIELDS.index(name)]


def plan(lib, shapes, per_sweep, group_max_chunks, n_cu, sw):
    """shapes: (n, 6) of N, Cin, Cout, H, W, ups; planned as sweeps of `per_sweep` consecutive layers."""
    shapes = np.ascontiguousarray(shapes, dtype=np.int32).reshape(-1, 6)
    out = np.zeros((len(shapes), len(FIELDS)), dtype=np.int64)
    broken = lib.shim_sweeps(shapes.ctypes.data_as(ctypes.c_void_p), len(shapes), int(per_sweep), int(group_max_chunks), int(n_cu), sw,
                             out.ctypes.data_as(ctypes.c_void_p))
    return Plans(out, broken)
