// Launch plan of the multi-scale L2 loss: tile sides, tiles per plane, grid, LDS bytes and workspace bytes from
// (N, C, H, W, L).  Plain C++ -- no HIP header, compiles with g++ -std=c++17 -- and the one set of functions that the kernels of
// pyrloss.hip and the host entries mg_pyramid_l2 / mg_pyramid_l2_ws_bytes both call, so that tests/test_project_cpu.py checks on
// the CPU what the device runs.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define PL_HD __host__ __device__
#else
#define PL_HD
#endif

constexpr int PL_MAX_LEVELS = 7;                 // levels 0 .. 6: the coarsest pixel of the deepest pyramid is 64 x 64 fine ones
constexpr int PL_TILE = 1 << (PL_MAX_LEVELS - 1);  // 64: a multiple of 2^(L - 1) for every L, so no level crosses a tile
constexpr int PL_THREADS = 256;                  // one thread: four quads of four columns, on the row pairs r, r + 16 of the tile
constexpr int PL_RED = 32;                       // partial sums per level after the first pass of the in-tile reduction
constexpr size_t PL_LDS_LIMIT = 160 * 1024;      // LDS of one CU, which one workgroup may declare in full

// where level s (1 <= s < L) of a tile lives in LDS, in floats, and its row stride; level 0 stays in registers
PL_HD constexpr int pl_level_stride(int s) { return PL_TILE >> s; }
PL_HD constexpr int pl_level_off(int s) {
  int off = 0;
  for (int q = 1; q < s; ++q) off += pl_level_stride(q) * pl_level_stride(q);
  return off;
}
// the pyramid floats rounded up to 8 bytes, then PL_THREADS + PL_RED float64 partials per level
PL_HD constexpr int pl_pyr_floats(int L) { return (pl_level_off(L) + 1) & ~1; }
PL_HD constexpr size_t pl_lds_bytes(int L) {
  return (size_t)pl_pyr_floats(L) * sizeof(float) + (size_t)L * (PL_THREADS + PL_RED) * sizeof(double);
}
// rows (columns) of tile t along a side of `size` pixels
PL_HD constexpr int pl_tile_extent(int size, int t) { return size - t * PL_TILE < PL_TILE ? size - t * PL_TILE : PL_TILE; }

struct PyrPlan {
  int ok;                        // 0: the shape is refused (every other field is 0 then)
  int tile_h, tile_w;            // sides of a full tile; the last tile of a row / column may be shorter, by a multiple of 2^(L-1)
  int tiles_y, tiles_x;          // tiles per plane
  long long tiles_per_sample;    // C * tiles_y * tiles_x: float64 partials per sample and level
  long long grid;                // workgroups of the tile launch: N * tiles_per_sample (the reduce launch: N)
  long long elems;               // N * C * H * W
  size_t lds_bytes;              // dynamic LDS of the tile launch
  size_t ws_bytes;               // N * L * tiles_per_sample float64
};

PL_HD inline PyrPlan pyr_plan(int N, int C, int H, int W, int L) {
  PyrPlan p = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (N < 1 || C < 1 || H < 1 || W < 1 || L < 1 || L > PL_MAX_LEVELS) return p;
  const int G = 1 << (L - 1);
  if (H % G != 0 || W % G != 0) return p;
  const int ty = (H + PL_TILE - 1) / PL_TILE, tx = (W + PL_TILE - 1) / PL_TILE;
  const long long per_sample = (long long)C * ty * tx, grid = per_sample * N;
  if (grid >= (1ll << 31)) return p;  // one launch's grid
  p.ok = 1;
  p.tile_h = H < PL_TILE ? H : PL_TILE;
  p.tile_w = W < PL_TILE ? W : PL_TILE;
  p.tiles_y = ty;
  p.tiles_x = tx;
  p.tiles_per_sample = per_sample;
  p.grid = grid;
  p.elems = (long long)N * C * H * W;
  p.lds_bytes = pl_lds_bytes(L);
  p.ws_bytes = (size_t)grid * L * sizeof(double);
  return p;
}
