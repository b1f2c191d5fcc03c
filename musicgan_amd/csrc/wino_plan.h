// Launch planner of the forward / data-gradient Winograd convolution (wino3x3.hip: LDS-staged tile blocks; wino_strip.hip: one wave
// per tile block): which of the two kernels takes a call, out-channel tiles and tile groups per workgroup, tile-block geometry, grids
// and LDS sizes.  Plain host C++ -- no HIP header, compiles with g++ -std=c++17 -- and integer arithmetic apart from the padding row's
// weight, so that tests/test_wino_plan_cpu.py can run it without a device.  Everything it needs from outside comes in as an argument:
// the layer, the CU count, the strip kernel's workgroups per CU and the switches.
#pragma once
#include <climits>
#include <cstddef>

#include "../../include/musicgan_hip.h"  // the MG_CONV_* flag bits (plain C)

constexpr int WINO_CC = 8;          // input channels per LDS chunk
constexpr int WINO_LDS_MAX = 160 * 1024;

// internal epilogue selectors of mg_wino3x3_fade (above the public MG_CONV_* bits of mg_wino3x3)
constexpr int WF_BLEND = 1 << 8;      // y = coef[0] * result + coef[1] * other
constexpr int WF_BLEND_BWD = 1 << 9;  // y = (coef[0] * acc) * lrelu'(mi),  p = (coef[1] * acc) * lrelu'(other)

// the epilogue kinds wino3x3_strip is instantiated for
enum StripKind {
  SK_ACT = 0,        // bias + LeakyReLU -> y (+ pooled)
  SK_ACT_POOL_MOUT,  // bias + LeakyReLU -> pooled + tile-mask bytes (y never written)
  SK_MB_POOL,        // x tile-mask bytes -> pooled
  SK_MASKF,          // x fp32 LeakyReLU mask of aux -> y (+ pooled)
  SK_UNPOOL,         // 0.25 * up2(result) x mask bytes of the layer below -> y at twice the size
  SK_BLEND_FWD,      // fade-in forward: act, tile mask out, alpha * new + (1 - alpha) * old -> y
  SK_BLEND_TAN,      // fade-in tangent: x mask bytes, blend -> y
  SK_BLEND_BWD,      // fade-in backward: two masked, scaled copies -> y, p
  SK_PN,             // bias + LeakyReLU + PixelNorm -> p, rn (+ y)
  SK_MB_Y,           // x tile-mask bytes -> y (a data gradient times the LeakyReLU derivative of the layer below, kept as bytes)
};

// The MG_WINO_* measurement switches (read from the environment by wino_switches() in wino3x3.hip, once per entry-point call).
// Some rules are switched off by a variable merely being SET: those fields have WINO_UNSET as a value of its own.
constexpr int WINO_UNSET = INT_MIN;
struct WinoSwitches {
  int cfg = WINO_UNSET;        // MG_WINO_CFG: 2, 3 or 4 out-channel tiles per workgroup; set at all: none of the automatic rules
  int wt = WINO_UNSET;         // MG_WINO_WT: 2 or 4 tile groups per workgroup; set at all: none of the automatic rules
  bool narrow = true;          // MG_WINO_NARROW set (to anything): the two-tile forms for at most 16 out-channels
  int narrow_wt = 2;           // MG_WINO_NARROW_WT: 4 or 8 tile groups per workgroup of the narrow form
  bool few = true;             // MG_WINO_FEW=0: keep the large tilings
  bool persist = true;         // MG_WINO_PERSIST=0: one workgroup per tile block
  int strip = 1;               // MG_WINO_STRIP: 0 = never the strip kernel, 2 = whenever the shape allows (tests, A/B)
  int strip_niw = 0;           // MG_WINO_STRIP_NIW: 1 / 2 / 3 out-channel tiles per wave (0: the planner's choice)
  int strip_wgs = 0;           // MG_WINO_STRIP_WGS: workgroups per CU (0: what the occupancy query says)
  double strip_padw = 0.7;     // MG_WINO_STRIP_PADW: a padding row's work relative to a full row's
  long long strip_min_blocks = 2048;  // MG_WINO_STRIP_MIN_BLOCKS: tile blocks from which the strip kernel takes a layer
  int strip_ablate = 0;        // MG_WINO_STRIP_ABLATE & 6 (wrong results): 2 = every input row through a zero-record descriptor (reads
                               // return 0, nothing is fetched), 4 = every epilogue access likewise (stores dropped, masks read as 0),
                               // 6 = both: what is left is issue time
};

// one call of mg_wino3x3 / mg_wino3x3_fade as the decisions see it
struct WinoLayer {
  int N, Cin, Cout, H, W;
  int flags;      // MG_CONV_* | WF_*
  bool has_bias;  // bias != nullptr
  bool has_y;     // y != nullptr
};
inline bool wino_pn(const WinoLayer& L) { return (L.flags & MG_CONV_PIXNORM) != 0; }

inline int wino_ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
inline int wino_pow2_ceil(int v) { return 1 << wino_ilog2(v); }
constexpr int wino_cdiv(int a, int b) { return (a + b - 1) / b; }

// out-channel tiles in the packed weights: padded so that the 3- and the 4-tile workgroups both find whole groups
// (the pack kernel goes by the same function: pack_wino_nt_padded, pack_kernels.h)
constexpr int wino_nt_padded(int Cout) {
  const int nt = wino_cdiv(Cout, 16);
  const int p4 = wino_cdiv(nt, 4) * 4, p3 = wino_cdiv(nt, 3) * 3;
  return p4 > p3 ? p4 : p3;
}

// ---------------------------------------------------------------------------------------------------------------- the strip kernel
struct WinoStripPlan {
  bool takes = false;
  int niw = 0, nwave = 0;  // out-channel tiles per wave, waves per workgroup
  int kind = SK_ACT;
  bool pool = false;
  int nchunk = 0, NT = 0, blocks_x = 0, blocks_y = 0;  // 8-channel chunks, padded out-channel tiles, 16-tile blocks per row, tile rows
  int ablate = 0;
  size_t lds = 0;  // the filter bank of a workgroup's tiles
  // the grid (wino_strip_grid): rows of workgroups one after the other in a 1-D grid
  int rows = 0, g_full = 0, g_pad = 0, grid = 0;
};

inline int wino_strip_kind(int flags) {  // the dispatch of wino_epilogue.h, by name
  if (flags & MG_CONV_PIXNORM) return SK_PN;
  if (flags & MG_CONV_UNPOOL) return SK_UNPOOL;
  if (flags & WF_BLEND_BWD) return SK_BLEND_BWD;
  if (flags & WF_BLEND) return (flags & MG_CONV_MASK_BYTES) ? SK_BLEND_TAN : SK_BLEND_FWD;
  if (flags & MG_CONV_MASK_AUX) return (flags & MG_CONV_MASK_BYTES) ? ((flags & MG_CONV_POOL_OUT) ? SK_MB_POOL : SK_MB_Y) : SK_MASKF;
  return (flags & MG_CONV_MASK_OUT) ? SK_ACT_POOL_MOUT : SK_ACT;
}

// the kinds that exist with and without the pooled output; the others are instantiated for one of the two only
inline bool wino_strip_pool(int kind, int flags) {
  if (kind == SK_ACT || kind == SK_MASKF) return (flags & MG_CONV_POOL_OUT) != 0;
  return kind == SK_ACT_POOL_MOUT || kind == SK_MB_POOL;
}

// Out-channel tiles per wave for a layer of nt tiles, or 0 = leave the call to wino3x3.hip.  Two wherever there are two or more (128
// accumulators, two waves per SIMD; further tile pairs go to further workgroup rows, which read and transform the input again; an odd
// count ends in a row that computes ONE tile on the two-tile filter image and gets a smaller share of the grid), one for 16
// out-channels.  The choice follows tools/ab_wino_strip.py (profiles/r05_ab_wino_strip.txt), us per launch against wino3x3.hip:
// 32 channels 0.72-0.92;  64 channels (the dominant launches of level 5: 48->64 @128 x 192 images 929 -> 782) 0.81-0.94;  48 channels
// 0.73-0.96 (64->48 @128 x 192, the largest launch of a level-5 step: 1016 -> 903);  80 / 96 channels 0.78-0.97 -- each from ~2 000
// tile blocks on (whole steps: 4096 -> 2048 is -0.3 % at level 5, -0.5 % at level 4, nothing at levels 3 / 6 / 7; 1536 is +1.3 % at
// level 6);  16 channels (one tile per wave: the 32 -> 16 data gradient of level 7) 0.81-0.91 since the in-block halo pixels come
// by DPP (1.01-1.06 before).  sw.strip == 2 (tests, A/B): whatever the shape allows.  sw.strip_niw (1 / 2 / 3) overrides the tile
// count per wave (3: the 192-accumulator, one-wave-per-SIMD form for exactly 48 channels; measurements).
inline int wino_strip_niw(const WinoLayer& L, const WinoSwitches& sw) {
  const int nt = L.Cout / 16;
  const long long blocks = (long long)L.N * (L.H / 2) * (L.W / 32);
  int niw = (sw.strip >= 2 || blocks >= sw.strip_min_blocks) ? (nt == 1 ? 1 : 2) : 0;
  // 96 .. 160 input channels: the filter bank of TWO out-channel tiles does not fit the LDS (8 KB per 8-channel chunk and tile), that
  // of one does -- one tile per wave then (the input is read and transformed once per tile, and still 0.82 of the staged kernel's time:
  // 96 -> 80 @32 x 192 images 168 -> 138 us, profiles/r06_ab_strip_small.txt)
  if (niw == 2 && (size_t)(L.Cin / WINO_CC) * 2 * 8192 > (size_t)WINO_LDS_MAX) niw = 1;
  if (wino_pn(L)) niw = nt <= 2 ? (niw ? nt : 0) : 0;  // PixelNorm: all channels of a pixel in one wave
  if (!wino_pn(L) && niw != 0) {
    const int v = sw.strip_niw;
    if (v == 1 || (v == 2 && nt >= 2) || (v == 3 && nt == 3)) niw = v;
  }
  return niw;
}

// Whether the strip kernel takes this call, and as which instantiation.  Shape: whole 16-channel chunk pairs and out tiles, whole
// 16-tile blocks per tile row, whole groups of 8 tile rows, the filter bank of a workgroup's tiles within LDS, every plane within
// 32-bit byte offsets, masked kinds bias-free, PixelNorm without y; then wino_strip_niw's choice.  sw.strip == 0: never; 2: whenever
// the shape allows.  Few channels on a large map is what it was written for: one wave per tile block, operands built in registers,
// filters resident in LDS.
inline bool wino_strip_shape_ok(const WinoLayer& L) {
  const int nt = L.Cout / 16;
  if ((L.Cin % 16) != 0 || (L.Cout % 16) != 0 || nt > 10 || (L.W % 32) != 0 || ((L.H / 2) % 8) != 0 || (L.H % 2) != 0) return false;
  if (wino_pn(L) && (nt > 2 || L.has_y)) return false;  // (PixelNorm: all channels of a pixel in one wave, p and rn only)
  if ((L.flags & (MG_CONV_MASK_AUX | MG_CONV_UNPOOL | WF_BLEND_BWD)) && L.has_bias) return false;  // masked kinds: bias-free
  if ((long long)L.Cout * L.H * L.W * 16 >= (1ll << 31) || (long long)L.Cin * L.H * L.W * 4 >= (1ll << 31)) return false;
  return true;
}

inline WinoStripPlan wino_strip_form(const WinoLayer& L, const WinoSwitches& sw) {
  WinoStripPlan p;
  if (sw.strip == 0 || !wino_strip_shape_ok(L)) return p;
  const int niw = wino_strip_niw(L, sw);
  if (niw == 0 || (size_t)(L.Cin / WINO_CC) * niw * 8192 > (size_t)WINO_LDS_MAX) return p;  // the filter bank of a workgroup's tiles fits LDS
  p.takes = true;
  // out-channel tiles per wave: two (or all three) of them -- the input transform is done once for them -- or ONE (half the
  // registers, twice the waves per SIMD, the input read and transformed once per tile); PixelNorm needs all channels in a wave
  p.niw = niw;
  p.nwave = niw == 3 ? 4 : 8;  // (niw == 1 in four-wave workgroups, i.e. up to four waves per SIMD: no effect,
                               //  profiles/r05_ab_wino_strip_nt1_occupancy.txt)
  p.kind = wino_strip_kind(L.flags);
  p.pool = wino_strip_pool(p.kind, L.flags);
  p.nchunk = L.Cin / WINO_CC;
  p.NT = wino_nt_padded(L.Cout);
  p.blocks_x = L.W / 32; p.blocks_y = L.H / 2;
  p.ablate = sw.strip_ablate;
  p.lds = (size_t)p.nchunk * niw * 2048 * sizeof(float);
  p.rows = wino_cdiv(L.Cout / 16, niw);  // (an odd tile count: the last workgroup row carries one padding tile of zero filters)
  return p;
}

// The grid of a call the strip kernel takes.  per_cu: what the occupancy query says for the instantiation and p.lds.
// Persistent workgroups: as many per CU as registers and the filter bank's LDS allow (the one-tile kernels: two, i.e. four waves
// per SIMD -- the waves are independent, occupancy is what hides a block's load latency), never more than there are groups.
inline void wino_strip_grid(WinoStripPlan& p, const WinoLayer& L, int n_cu, int per_cu, const WinoSwitches& sw) {
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 16 / p.nwave) per_cu = 16 / p.nwave;
  if (sw.strip_wgs >= 1) per_cu = sw.strip_wgs;  // (tools/ab_wino_strip.py flips it inside one process)
  // a last row whose second tile is padding does ~0.7 of a full row's work (half the MFMAs and epilogue, the same input loads and
  // transform; swept 0.6 .. 1.0 on 64->48@128, 64->80@64, 48->48@128: 0.7) and gets that share of the workgroups
  const int rows = p.rows, nt = L.Cout / 16;
  const bool has_pad = p.niw == 2 && (nt & 1) != 0 && rows > 1;
  const int total = per_cu * n_cu;
  int g_pad = 0, g_full;
  if (has_pad) {
    g_pad = (int)(total * sw.strip_padw / ((rows - 1) + sw.strip_padw)) & ~7;
    if (g_pad < 8) g_pad = 8;
    g_full = ((total - g_pad) / (rows - 1)) & ~7;
  } else {
    g_full = (total / rows) & ~7;
  }
  if (g_full < 8) g_full = 8;
  const int nitems = L.N * (p.blocks_y / p.nwave) * p.blocks_x;
  if (g_full > nitems) g_full = nitems;  // (small launches: fewer workgroups than CUs; the XCD mapping then is whatever it is)
  if (g_pad > nitems) g_pad = nitems;
  p.g_full = g_full; p.g_pad = g_pad;
  p.grid = (rows - (g_pad ? 1 : 0)) * g_full + g_pad;
}

inline WinoStripPlan wino_strip_plan(const WinoLayer& L, int n_cu, int per_cu, const WinoSwitches& sw) {
  WinoStripPlan p = wino_strip_form(L, sw);
  if (p.takes) wino_strip_grid(p, L, n_cu, per_cu, sw);
  return p;
}

// mg_wino3x3_mask_bytes_y_supported: MASK_AUX | MASK_BYTES without POOL_OUT is an epilogue of the strip kernel only
inline bool wino_mask_bytes_y_supported(int N, int Cin, int Cout, int H, int W, const WinoSwitches& sw) {
  if (N <= 0 || Cin <= 0 || Cout <= 0 || H <= 0 || W <= 0 || (H % 2) || (W % 2)) return false;
  const WinoLayer L = {N, Cin, Cout, H, W, MG_CONV_MASK_AUX | MG_CONV_MASK_BYTES, false, false};
  return wino_strip_form(L, sw).takes;
}

// --------------------------------------------------------------------------------------------------------------- the staged kernel
enum WinoStatus {
  WINO_OK = 0,
  WINO_MASK_BYTES_SHAPE,  // MASK_BYTES without POOL_OUT on a shape the strip kernel does not take
  WINO_TILE_ERROR,        // internal: the workgroup's tile groups run past the packed weights
  WINO_BLOCK_TOO_LARGE,   // image block too large for 32-bit offsets
};

struct WinoStagedPlan {
  int status = WINO_OK;
  int cfg = 0, wt = 0;  // out-channel tiles and 16-tile groups per workgroup: wino3x3_mfma<NIW, WC, WT> with NIW * WC == cfg
  bool narrow = false;
  int TBW = 0, TBH = 0, TBN = 0, lgTBW = 0, lgTBH = 0;  // tile-block geometry in TILES: TBW * TBH * TBN == 16 * wt
  int blocks_x = 0, blocks_y = 0, blocks_n = 0;
  int nchunk = 0, NT = 0;
  int grid_x = 0, grid_y = 0;
  bool persistent = false;  // grid_x workgroups walk blocks_x * blocks_y * blocks_n tile blocks
  size_t lds = 0;
};

// tiles per wave x wave groups of the `cfg` out-channel tiles of a workgroup: 4 = 2x2, 3 = 1x3, 2 = 1x2, 1 = 1x1
constexpr int wino_staged_niw(int cfg) { return cfg == 4 ? 2 : 1; }
constexpr int wino_staged_wc(int cfg) { return cfg == 4 ? 2 : cfg; }
// input tiles [WT][8 component pairs][64 lanes][4] x 8 channels, filters [WC * NIW tiles][2048], PixelNorm partial sums [WC][TPB][4]
constexpr size_t wino_staged_lds(int niw, int wc, int wt) {
  return (size_t)(16 * (wt * 16) * WINO_CC + wc * niw * 2048 + wc * (wt * 16) * 4) * sizeof(float);
}

inline WinoStagedPlan wino_staged_plan(const WinoLayer& L, int n_cu, const WinoSwitches& sw) {
  WinoStagedPlan p;
  const int N = L.N, Cin = L.Cin, Cout = L.Cout, H = L.H, W = L.W;
  const bool pn = wino_pn(L), cfg_set = sw.cfg != WINO_UNSET, wt_set = sw.wt != WINO_UNSET;
  const int nt = wino_cdiv(Cout, 16);
  p.nchunk = wino_cdiv(Cin, WINO_CC);
  p.NT = wino_nt_padded(Cout);
  const int Ht = H / 2, Wt = W / 2;
  // (tile-mask bytes applied to a full-resolution result: an epilogue of the strip kernel only -- mg_wino3x3_mask_bytes_y_supported)
  if ((L.flags & MG_CONV_MASK_BYTES) && !(L.flags & (MG_CONV_POOL_OUT | WF_BLEND))) {
    p.status = WINO_MASK_BYTES_SHAPE;
    return p;
  }
  // out-channel tiles per workgroup (wave groups x tiles per wave): 4 = 2x2, 3 = 3x1, 2 = 2x1 -- least padding wins
  int cfg = 4, best = wino_cdiv(nt, 4) * 4;
  if (wino_cdiv(nt, 3) * 3 < best) { cfg = 3; best = wino_cdiv(nt, 3) * 3; }
  if (wino_cdiv(nt, 2) * 2 < best) { cfg = 2; best = wino_cdiv(nt, 2) * 2; }
  // five or more channel tiles (80 .. 160 out-channels: the 64x64 .. 8x8 layers): two tiles per workgroup in the 32-tile form --
  // four-wave workgroups, several per CU -- beat the 12- and 16-wave tilings by 6-8 % at 64x64 / 32x32 and by ~20 % at 16x16
  // (tools/tune_wino.py, every (cfg, wt) per layer shape of a level-5 step); 48 and 64 out-channels stay on their one
  // workgroup per CU (3x1 and 2x2 tiles)
  if (nt >= 5) cfg = 2;
  if (pn) cfg = nt <= 2 ? 2 : (nt == 3 ? 3 : 4);
  // at most 16 out-channels: ONE channel tile per workgroup and 128 tiles instead of a second, all-padding channel tile
  // (the 32 -> 16 data gradient at 512x512 spent half its MFMAs on zero filters)
  const bool narrow = nt == 1 && !pn && !cfg_set && !wt_set && sw.narrow;
  if (narrow) cfg = 1;
  if (cfg_set && !pn) {  // measurement override: 2, 3 or 4 out-channel tiles per workgroup
    const int v = sw.cfg;
    if (v == 2 || v == 4 || (v == 3 && wino_cdiv(nt, 3) * 3 <= p.NT)) cfg = v;
  }
  if (wino_cdiv(nt, cfg) * cfg > p.NT) {
    p.status = WINO_TILE_ERROR;
    return p;
  }
  // tiles per workgroup: 64 (one 8..12-wave workgroup per CU: every wave of the CU is in the same phase, so the VALU staging
  // and epilogue never queue behind another workgroup's matrix instructions -- measured 70..140 cycles per VALU instruction
  // when they do, tools/hwtests/valu_latency_under_mfma.hip -- and the filters are staged once per 64 tiles) when that still
  // gives every CU two or more workgroups, else 32 (two workgroups per CU).
  int wt = ((long long)N * Ht * Wt / 64) * wino_cdiv(nt, cfg) >= 2ll * n_cu ? 4 : 2;
  if (narrow) {
    // 32 tiles per two-wave workgroup, ~6 of them per CU: with 16 out-channels a block is a few hundred cycles of MFMAs between
    // memory round trips, and occupancy hides those where one 128-tile workgroup per CU (the first form of this variant) waited:
    // 32->16@512, 18 images: 0.70 (two-tile form) -> 0.49 (128 tiles) -> 0.40 ms
    wt = 2;
    if (sw.narrow_wt == 4 || sw.narrow_wt == 8) wt = sw.narrow_wt;  // measurement override
    if (wt == 8 && (long long)N * Ht * Wt / 128 < 2ll * n_cu) wt = 2;
  }
  // two out-channel tiles (<= 32 channels): few MFMAs per staged item and per epilogue, so a block is mostly memory latency and
  // vector work -- four-wave workgroups, several per CU, overlap that where one eight-wave workgroup per CU waits (measured
  // 11-16 % on 16->32@512, 32->32@256, 48->32@256; the opposite of the 48- and 64-channel tilings, tools/bench_l67.py)
  if (cfg == 2 && !narrow && !pn && !wt_set && !cfg_set) wt = 2;
  if (sw.wt == 2 || sw.wt == 4) wt = sw.wt;  // measurement override
  // a grid that leaves CUs idle even in the 32-tile form takes two out-channel tiles per workgroup instead of three or four: more,
  // lighter workgroups (the input tile is staged by more of them, which a half-empty chip does not notice)
  if (wt == 2 && !pn && cfg > 2 && !cfg_set && ((long long)N * Ht * Wt + 31) / 32 * wino_cdiv(nt, cfg) < n_cu &&
      wino_cdiv(nt, 2) * 2 <= p.NT)
    cfg = 2;
  // Few 64-tile blocks per CU (the 48- and 64-channel layers at the reference's batch of 6: 128x128 / 64x64 maps at levels 6-7):
  // the one-workgroup-per-CU tilings idle through most of their last round and have nobody to overlap their vector phases with;
  // two out-channel tiles per four-wave workgroup, several per CU, are 5-18 % ahead there (tools/tune_wino.py 6 6 and 7 6:
  // 64 channels up to 4.5 blocks per CU, 48 channels at 1.5 but not at 4.5; at 16 per CU -- level 5, batch 64 -- the large tilings win)
  if (!pn && !narrow && !cfg_set && !wt_set && sw.few) {
    const long long b64 = (long long)N * Ht * Wt / 64;
    if (((cfg == 4 && b64 < 6ll * n_cu) || (cfg == 3 && 2 * b64 < 5ll * n_cu)) && wino_cdiv(nt, 2) * 2 <= p.NT) {
      cfg = 2;
      wt = 2;
    }
  }
  p.cfg = cfg; p.wt = wt; p.narrow = narrow;
  const int tpb = wt * 16;
  p.TBW = wino_pow2_ceil(Wt) < 16 ? wino_pow2_ceil(Wt) : 16;  // 16 tiles = 32 pixels = one 128-byte line per row and channel
  p.TBH = wino_pow2_ceil(Ht) < tpb / p.TBW ? wino_pow2_ceil(Ht) : tpb / p.TBW;
  p.TBN = tpb / (p.TBW * p.TBH);
  p.lgTBW = wino_ilog2(p.TBW); p.lgTBH = wino_ilog2(p.TBH);
  p.blocks_x = wino_cdiv(Wt, p.TBW); p.blocks_y = wino_cdiv(Ht, p.TBH); p.blocks_n = wino_cdiv(N, p.TBN);
  if ((long long)p.TBN * Cin * H * W >= (1ll << 29)) {
    p.status = WINO_BLOCK_TOO_LARGE;
    return p;
  }
  p.grid_x = p.blocks_x * p.blocks_y * p.blocks_n;
  p.grid_y = wino_cdiv(nt, cfg);
  // persistent launch of the 64-tile form: one workgroup per CU, each walking its tile blocks
  if (wt >= 4 && sw.persist && p.grid_x > n_cu) {
    p.grid_x = n_cu;
    p.persistent = true;
  }
  p.lds = wino_staged_lds(wino_staged_niw(cfg), wino_staged_wc(cfg), wt);
  return p;
}
