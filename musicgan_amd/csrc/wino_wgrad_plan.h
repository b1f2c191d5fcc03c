// Launch planner of the Winograd weight gradient (wino_wgrad*.hip): chunk geometry, channel blocks, split-K, which form a layer
// takes (row-staged, scalar-addressed), which layers of a sweep share a grouped launch and how the group's splits are balanced.
// Pure integer arithmetic on plain host C++ -- no HIP header, compiles with g++ -std=c++17 -- so that tests/test_wgrad_plan_cpu.py
// can run it without a device.  Everything it needs from outside comes in as an argument: the CU count and the switches.
#pragma once
#include <cstddef>

constexpr int WW_KT = 8;           // tiles per chunk
constexpr int WW_GROUP = 16;       // layers per grouped launch
constexpr int WW_MAX_LAYERS = 64;  // layers per sweep

// the MG_WGRAD_* measurement switches (read from the environment by ww_switches() in wino_wgrad.hip, once per entry-point call)
struct WwSwitches {
  int rows = 1;              // MG_WGRAD_ROWS: 0 = never the row-staged form; 2 = also the narrow block shapes
  bool rows_ups = true;      // MG_WGRAD_ROWS_UPS=0: the up-sampled-input layers stay on the chunk-staged kernels
  int ablate = 0;            // MG_WGRAD_ROWS_ABLATE & 126 (wrong results): 2 = no staging, 4 = no barriers, 8 = staging never waited for, 16 = every stage re-reads the slab's first one, 64 = every second x copy instruction dropped
  bool fast = true;          // MG_WGRAD_FAST=0: never the scalar-addressed form
  int group_fixed = 6;       // MG_WGRAD_GROUP_FIXED: the per-chunk staging term of the group's cost model
  int group_slots_q = 4;     // MG_WGRAD_GROUP_SLOTS: workgroups per group launch in units of 1/4 of the CUs
};

// integer launch geometry of one layer: what the kernels read of a plan (WwArgs embeds it)
struct WwGeo {
  int N, Cin, Cout, H, W;
  int TBW, TBH, TBN, lgTBW, lgTBH;  // chunk geometry in TILES: TBW * TBH * TBN == 8
  int blocks_x, blocks_y, blocks_n, nblk, per;
  int CinP, CoutP;
  int nob;  // out-channel blocks (blockIdx.y = cb * nob + ob)
};

struct WwPlan {
  WwGeo a;
  int CT, OT, ncb, nsplit;
  int nsplit_ws;      // splits of the chunk plan: the workspace is sized for these, no later re-plan may use more
  size_t ws_floats;   // of the chunk plan
  bool rows = false;  // the row-staged kernel (wino_wgrad_rows_mfma) and its stage geometry
  bool small = false; // few enough chunks to share a grouped launch (ww_small)
  int var = 0;        // ww_var(CT, OT, ups)
};

inline int ww_ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
inline int ww_pow2_ceil(int v) { return 1 << ww_ilog2(v); }
inline int ww_cdiv(int a, int b) { return (a + b - 1) / b; }

inline int blocks_of(int tiles) {  // channel tiles -> blocks of <= 4 tiles, balanced
  return ww_cdiv(tiles, 4);
}

// block shape and input kind of a layer as one number: selects the body in wino_wgrad_group_mfma
constexpr int ww_var(int CT, int OT, bool UPS) { return (CT * 10 + OT) * 2 + (UPS ? 1 : 0); }

// splits of `nblk` blocks over `ns` workgroups per channel block pair, no empty slab
inline void ww_split(WwPlan& pl, int ns) {
  WwGeo& a = pl.a;
  if (ns > a.nblk) ns = a.nblk;
  a.per = ww_cdiv(a.nblk, ns);
  pl.nsplit = ww_cdiv(a.nblk, a.per);
}

inline void plan_ww(int N, int Cin, int Cout, int H, int W, int n_cu, WwPlan& pl) {
  WwGeo& a = pl.a;
  a.N = N; a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W;
  const int Ht = H / 2, Wt = W / 2;
  a.TBW = ww_pow2_ceil(Wt) < WW_KT ? ww_pow2_ceil(Wt) : WW_KT;
  a.TBH = ww_pow2_ceil(Ht) < WW_KT / a.TBW ? ww_pow2_ceil(Ht) : WW_KT / a.TBW;
  a.TBN = WW_KT / (a.TBW * a.TBH);
  a.lgTBW = ww_ilog2(a.TBW); a.lgTBH = ww_ilog2(a.TBH);
  a.blocks_x = ww_cdiv(Wt, a.TBW); a.blocks_y = ww_cdiv(Ht, a.TBH); a.blocks_n = ww_cdiv(N, a.TBN);
  a.nblk = a.blocks_x * a.blocks_y * a.blocks_n;
  const int ct = ww_cdiv(Cin, 16), ot = ww_cdiv(Cout, 16);
  pl.ncb = blocks_of(ct);
  a.nob = blocks_of(ot);
  pl.CT = ww_cdiv(ct, pl.ncb);  // 1..4 channel tiles per block: the kernel is instantiated for each (no MFMAs on padding tiles)
  pl.OT = ww_cdiv(ot, a.nob);
  a.CinP = ct * 16; a.CoutP = ot * 16;
  const int ny = pl.ncb * a.nob;
  // one 8-wave workgroup (128 KB of LDS) per CU; the narrow form (64 KB) runs two
  // (when that still leaves every workgroup >= 96 chunks: each slab costs a G^T M G pass and a share of the reduction)
  const int per_cu = (pl.CT + pl.OT <= 4 && (long long)a.nblk * ny >= 96ll * 2 * n_cu) ? 2 : 1;
  ww_split(pl, per_cu * n_cu / ny > 0 ? per_cu * n_cu / ny : 1);
  pl.nsplit_ws = pl.nsplit;
  pl.ws_floats = (size_t)pl.nsplit * (9 * (size_t)a.CinP * a.CoutP + a.CoutP);
  pl.rows = pl.small = false;
}

// ---- the row-staged form: stages of 16 x 1 x 1 tiles.  rows mode 0: never; 2: also the narrow block shapes (measurements)
inline bool ww_rows_takes(const WwPlan& pl, bool ups, const WwSwitches& sw) {
  if (sw.rows == 0 || (pl.a.W % 32) != 0 || (pl.a.H % 2) != 0) return false;
  if (ups && !sw.rows_ups) return false;
  if (pl.CT == 4 && pl.OT == 4) return false;  // (256 accumulators + raw set + two operand sets: 68 bytes of scratch per lane; not instantiated)
  return sw.rows >= 2 || pl.CT * pl.OT >= 4;  // (blocks of one channel tile on either side: 2 MFMAs per wave and k-step -- the chunk-staged narrow form is as fast or faster, profiles/r06_wgrad_rows_steps.txt)
}

inline void plan_rows(WwPlan& pl, int n_cu, const WwSwitches& sw) {
  WwGeo& a = pl.a;
  a.TBW = 16; a.TBH = 1; a.TBN = 1; a.lgTBW = 4; a.lgTBH = 0;
  a.TBN |= sw.ablate;
  a.blocks_x = a.W / 32; a.blocks_y = a.H / 2; a.blocks_n = a.N;
  a.nblk = a.blocks_x * a.blocks_y * a.blocks_n;
  const int ny = pl.ncb * a.nob;
  ww_split(pl, n_cu / ny > 0 ? n_cu / ny : 1);  // one 8-wave workgroup per CU
  pl.rows = true;
}

// the scalar-addressed form (ww_body FAST): chunks of 8 x 1 x 1 tiles, whole chunks per tile row
inline bool ww_fast(const WwGeo& a, const WwSwitches& sw) {
  return sw.fast && a.TBW == 8 && a.TBH == 1 && a.TBN == 1 && (a.W % 16) == 0;
}

// the block shapes inlined in wino_wgrad_group_mfma
inline bool ww_groupable(int CT, int OT) { return CT >= 3 && OT >= 3; }

// small enough to share a launch: at most group_max_chunks 8-tile chunks per workgroup at one workgroup per CU (of the chunk plan)
inline bool ww_small(const WwPlan& pl, int group_max_chunks, int n_cu) {
  const long long work = (long long)pl.a.nblk * pl.ncb * pl.a.nob;  // chunks x channel blocks
  return group_max_chunks > 0 && ww_groupable(pl.CT, pl.OT) && work <= (long long)group_max_chunks * n_cu;
}

// the workspace is sized by the chunk plan: a re-plan (rows, group) that used more splits would write past it
inline bool ww_plan_fits(const WwPlan& pl) { return pl.nsplit >= 1 && pl.nsplit <= pl.nsplit_ws; }

// One layer on its own terms: the chunk plan; row-staged where taken, unless the layer is small (group_max_chunks <= 0: never).
// false: the final plan has more splits than the workspace holds.
inline bool ww_plan_layer(int N, int Cin, int Cout, int H, int W, bool ups, int group_max_chunks, int n_cu, const WwSwitches& sw,
                          WwPlan& pl) {
  plan_ww(N, Cin, Cout, H, W, n_cu, pl);
  pl.var = ww_var(pl.CT, pl.OT, ups);
  pl.small = ww_small(pl, group_max_chunks, n_cu);
  if (!pl.small && ww_rows_takes(pl, ups, sw)) plan_rows(pl, n_cu, sw);
  return ww_plan_fits(pl);
}

// 0 / 1 / 2: chunk-staged, row-staged, row-staged for an up-sampled input
inline int ww_form(int N, int Cin, int Cout, int H, int W, bool ups, int group_max_chunks, int n_cu, const WwSwitches& sw) {
  WwPlan pl;
  ww_plan_layer(N, Cin, Cout, H, W, ups, group_max_chunks, n_cu, sw, pl);
  return pl.rows ? (ups ? 2 : 1) : 0;
}

// The grouped launches of a sweep whose layers went through ww_plan_layer: the small layers, in order, in lots of at most WW_GROUP;
// a lot of one launches alone (chunk-staged).  group_of[i] = -1: layer i launches alone, in the form pl[i].rows / ww_fast say.
struct WwSweep {
  WwPlan pl[WW_MAX_LAYERS];
  int group_of[WW_MAX_LAYERS];
  int ngroups;
};

inline bool ww_plan_groups(WwSweep& S, int n, int n_cu, const WwSwitches& sw) {
  WwPlan* pl = S.pl;
  S.ngroups = 0;
  for (int i = 0; i < n; ++i) S.group_of[i] = -1;
  for (int next = 0;;) {
    int idx[WW_GROUP], m = 0;
    for (; next < n && m < WW_GROUP; ++next)
      if (pl[next].small) idx[m++] = next;
    if (m < 2) break;
    // The splits of the group: about the same TIME per workgroup (a chunk of a <CT, OT> block costs ~ CT * OT MFMA groups + its
    // staging), at most one workgroup per CU over the whole group -- a 257th workgroup would run alone after the others.
    auto cost = [&](int i) { return pl[i].CT * pl[i].OT + sw.group_fixed; };
    long long work = 0;
    for (int k = 0; k < m; ++k) work += (long long)pl[idx[k]].a.nblk * pl[idx[k]].ncb * pl[idx[k]].a.nob * cost(idx[k]);
    const int slots = n_cu * sw.group_slots_q / 4;
    long long budget = (work + slots - 1) / slots;  // cost units per workgroup
    int ns[WW_GROUP], total;
    for (;;) {
      total = 0;
      bool floor_reached = true;  // every layer at one split: nothing left to shrink
      for (int k = 0; k < m; ++k) {
        const WwPlan& q = pl[idx[k]];
        long long per = budget / cost(idx[k]);
        if (per < 1) per = 1;
        int v = (int)((q.a.nblk + per - 1) / per);
        if (v > q.nsplit) v = q.nsplit;  // (the workspace was sized for the single-layer plan)
        ns[k] = v;
        floor_reached = floor_reached && v == 1;
        total += v * q.ncb * q.a.nob;
      }
      if (total <= slots || floor_reached) break;
      budget += (budget + 15) / 16;
    }
    for (int k = 0; k < m; ++k) {
      ww_split(pl[idx[k]], ns[k]);
      if (!ww_plan_fits(pl[idx[k]])) return false;
      S.group_of[idx[k]] = S.ngroups;
    }
    ++S.ngroups;
  }
  return true;
}

// ---- the slab reduce: split-lanes per filter element and workgroups per job (wino_wgrad_reduce_multi)
constexpr int ww_reduce_lanes(int nsplit, int total) { return (nsplit >= 128 && total <= 8192) ? 32 : 8; }  // (the kernel calls it too)
inline int ww_reduce_blocks(int nsplit, int total) { return ww_cdiv(total, 512 / ww_reduce_lanes(nsplit, total)); }
