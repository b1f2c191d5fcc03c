// DiffAugment's random parameters: one row of eight uniform numbers in [0, 1) -> the shift and the cutout box of one
// sample.  Plain C++ with float32 arithmetic spelled out -- no HIP header, compiles with g++ -std=c++17 -- and the one function the
// kernels of diffaug.hip and the host entry mg_diffaug_decode both call, so that tests/test_diffaug_cpu.py checks on the CPU what the
// device runs.
#pragma once

#if defined(__HIPCC__)
#define DA_HD __host__ __device__
#else
#define DA_HD
#endif

constexpr int DA_TRANSLATION = 1, DA_CUTOUT = 2;  // MG_DIFFAUG_* of include/musicgan_hip.h
constexpr int DA_U = 8;                           // numbers per sample: on/off, dy, dx | on/off, oy, ox | two reserved

struct DaParams {
  int dy, dx;          // T x[i, j] = x[i - dy, j - dx]
  int y0, y1, x0, x1;  // rows [y0, y1) x columns [x0, x1) become +0.0; empty (all 0) when cutout is off
};

// min(floor(u * bins), bins - 1) for u in [0, 1): one float32 product, rounded once.  Anything else (negative, NaN, >= 1) still lands
// in [0, bins), so that no value of u can send a kernel out of its image.
DA_HD inline int da_bin(float u, int bins) {
  const float t = u * (float)bins;
  return t >= 0.f ? (t < (float)bins ? (int)t : bins - 1) : 0;
}

DA_HD inline DaParams da_decode(const float* u, int H, int W, int ops, float p) {
  DaParams q = {0, 0, 0, 0, 0, 0};
  if ((ops & DA_TRANSLATION) && u[0] < p) {
    const int ry = (H + 4) / 8, rx = (W + 4) / 8;  // floor(H / 8 + 0.5)
    q.dy = da_bin(u[1], 2 * ry + 1) - ry;
    q.dx = da_bin(u[2], 2 * rx + 1) - rx;
  }
  if ((ops & DA_CUTOUT) && u[3] < p) {
    const int ch = (H + 1) / 2, cw = (W + 1) / 2;  // floor(H / 2 + 0.5)
    const int oy = da_bin(u[4], H + 1 - ch % 2), ox = da_bin(u[5], W + 1 - cw % 2);
    const int t = oy - ch / 2, l = ox - cw / 2;
    q.y0 = t > 0 ? t : 0;
    q.y1 = t + ch < H ? t + ch : H;
    q.x0 = l > 0 ? l : 0;
    q.x1 = l + cw < W ? l + cw : W;
  }
  return q;
}
