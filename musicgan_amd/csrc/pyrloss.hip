// Multi-scale L2 loss with its gradient on (N, C, H, W) float32:
//   d_0 = x - t,  d_{s+1}[i, j] = ((d_s[2i, 2j] + d_s[2i, 2j+1]) + (d_s[2i+1, 2j] + d_s[2i+1, 2j+1])) * 0.25f   (avgpool2_fwd_k's expression)
//   loss_n = sum_s lambda_s / (C H_s W_s) * sum (double)d_s^2            float64, fixed order, no atomics
//   g      = (lambda_{L-1} d_{L-1}, then fmaf(lambda_s, d_s, .) for s = L-2 .. 0) * k,  k = (float)(2 / (C H W))
// Two launches.  pyr_tile_k: one workgroup per 64 x 64 tile of one plane (pyrloss_plan.h; 64 is a multiple of 2^(L-1), so no level
// crosses a tile) reads x and t once, keeps d_0 in registers -- a thread owns four quads of four columns on the row pairs r and
// r + 16 of the tile, so level 1 comes out of its own registers -- builds levels 1 .. L-1 in LDS, writes g and the tile's L float64
// partial sums.  pyr_reduce_k: one workgroup per sample adds the partials of each level in index order and weighs them.  A tile
// belongs to one sample and the reduction walks one sample's partials, so a sample's results depend on that sample alone.
#include "pyrloss_plan.h"
#include "mg_common.h"

#include <cmath>

namespace {

struct PlWeights {
  float lam[PL_MAX_LEVELS];
  float k;
};
struct PlCoef {
  double c[PL_MAX_LEVELS];  // lambda_s / (C H_s W_s)
};

__device__ __forceinline__ double pl_sq(float v) { return (double)v * (double)v; }  // exact: 48 bits

template <int L, bool VEC>
__global__ __launch_bounds__(PL_THREADS) void pyr_tile_k(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ g,
                                                         double* __restrict__ ws, int C, int H, int W, int tiles_y, int tiles_x,
                                                         PlWeights wt) {
  extern __shared__ double pl_lds[];
  float* pyr = reinterpret_cast<float*>(pl_lds);
  double* red = reinterpret_cast<double*>(pyr + pl_pyr_floats(L));
  double* red2 = red + L * PL_THREADS;
  const int tid = threadIdx.x;
  const int tpp = tiles_y * tiles_x;
  const int plane = blockIdx.x / tpp, tile = blockIdx.x - plane * tpp;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int th = pl_tile_extent(H, ty), tw = pl_tile_extent(W, tx);
  const size_t base = (size_t)plane * H * W + (size_t)(ty * PL_TILE) * W + (size_t)tx * PL_TILE;
  const int q = tid & 15, r = tid >> 4, j0 = q << 2;

  // level 0: d[2h + e] is row 2 (r + 16 h) + e of the tile, columns j0 .. j0 + 3; +0 outside the tile
  f32x4 d[4];
  double sq[L];
#pragma unroll
  for (int s = 0; s < L; ++s) sq[s] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 2 * (r + 16 * (k >> 1)) + (k & 1);
    const size_t o = base + (size_t)i * W + j0;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i < th) {
      if constexpr (VEC) {
        if (j0 < tw) v = *reinterpret_cast<const f32x4*>(x + o) - *reinterpret_cast<const f32x4*>(t + o);
      } else {
        if (j0 + 0 < tw) v.x = x[o + 0] - t[o + 0];
        if (j0 + 1 < tw) v.y = x[o + 1] - t[o + 1];
        if (j0 + 2 < tw) v.z = x[o + 2] - t[o + 2];
        if (j0 + 3 < tw) v.w = x[o + 3] - t[o + 3];
      }
    }
    d[k] = v;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) sq[0] += (pl_sq(d[k].x) + pl_sq(d[k].y)) + (pl_sq(d[k].z) + pl_sq(d[k].w));

  // level 1 from the registers: row r + 16 h, columns 2 q and 2 q + 1
  float l1[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  if constexpr (L >= 2) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 a = d[2 * h], b = d[2 * h + 1];
      l1[h][0] = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
      l1[h][1] = ((a.z + a.w) + (b.z + b.w)) * 0.25f;
      sq[1] += pl_sq(l1[h][0]) + pl_sq(l1[h][1]);
      if constexpr (L >= 3) {
        const float2 o = {l1[h][0], l1[h][1]};
        *reinterpret_cast<float2*>(pyr + pl_level_off(1) + (r + 16 * h) * pl_level_stride(1) + 2 * q) = o;
      }
    }
  }
  // levels 2 .. L-1 in LDS: at most 256 elements each, one per thread.  Outside the tile the sources are +0 and so is the result.
#pragma unroll
  for (int s = 2; s < L; ++s) {
    __syncthreads();
    const int st = pl_level_stride(s), sp = pl_level_stride(s - 1);
    if (tid < st * st) {
      const int i = tid / st, j = tid - i * st;
      const float* src = pyr + pl_level_off(s - 1) + (2 * i) * sp + 2 * j;
      const float2 a = *reinterpret_cast<const float2*>(src), b = *reinterpret_cast<const float2*>(src + sp);
      const float v = ((a.x + a.y) + (b.x + b.y)) * 0.25f;
      pyr[pl_level_off(s) + i * st + j] = v;
      sq[s] += pl_sq(v);
    }
  }
  if constexpr (L >= 3) __syncthreads();

  if (g != nullptr) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int p = r + 16 * h;  // row of level 1
      float a1[2];
      if constexpr (L == 1) {
        a1[0] = a1[1] = 0.f;
      } else if constexpr (L == 2) {
        a1[0] = wt.lam[1] * l1[h][0];
        a1[1] = wt.lam[1] * l1[h][1];
      } else {
        float acc = wt.lam[L - 1] * pyr[pl_level_off(L - 1) + (p >> (L - 2)) * pl_level_stride(L - 1) + (j0 >> (L - 1))];
#pragma unroll
        for (int s = L - 2; s >= 2; --s)
          acc = fmaf(wt.lam[s], pyr[pl_level_off(s) + (p >> (s - 1)) * pl_level_stride(s) + (j0 >> s)], acc);
        a1[0] = fmaf(wt.lam[1], l1[h][0], acc);
        a1[1] = fmaf(wt.lam[1], l1[h][1], acc);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int i = 2 * p + e;
        const f32x4 v = d[2 * h + e];
        f32x4 o;
        if constexpr (L == 1) {
          o.x = (wt.lam[0] * v.x) * wt.k, o.y = (wt.lam[0] * v.y) * wt.k, o.z = (wt.lam[0] * v.z) * wt.k, o.w = (wt.lam[0] * v.w) * wt.k;
        } else {
          o.x = fmaf(wt.lam[0], v.x, a1[0]) * wt.k, o.y = fmaf(wt.lam[0], v.y, a1[0]) * wt.k;
          o.z = fmaf(wt.lam[0], v.z, a1[1]) * wt.k, o.w = fmaf(wt.lam[0], v.w, a1[1]) * wt.k;
        }
        if (i < th) {
          float* dst = g + base + (size_t)i * W + j0;
          if constexpr (VEC) {
            if (j0 < tw) *reinterpret_cast<f32x4*>(dst) = o;
          } else {
            if (j0 + 0 < tw) dst[0] = o.x;
            if (j0 + 1 < tw) dst[1] = o.y;
            if (j0 + 2 < tw) dst[2] = o.z;
            if (j0 + 3 < tw) dst[3] = o.w;
          }
        }
      }
    }
  }

  // the tile's L sums, in a fixed order: thread (s, q2) adds eight of level s's 256 partials, thread s then those 32 sums
#pragma unroll
  for (int s = 0; s < L; ++s) red[s * PL_THREADS + tid] = sq[s];
  __syncthreads();
  {
    const int s = tid / PL_RED, q2 = tid - s * PL_RED;
    if (s < L) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < PL_THREADS / PL_RED; ++k) acc += red[s * PL_THREADS + q2 + PL_RED * k];
      red2[s * PL_RED + q2] = acc;
    }
  }
  __syncthreads();
  if (tid < L) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < PL_RED; ++k) acc += red2[tid * PL_RED + k];
    const long long per_sample = (long long)C * tpp;
    const long long n = plane / C;
    ws[((size_t)n * L + tid) * (size_t)per_sample + (size_t)(blockIdx.x - n * per_sample)] = acc;
  }
}

// one workgroup per sample: thread s adds the partials of level s in index order, thread 0 weighs the L sums in level order.  The
// partials come through LDS, PL_THREADS per level at a time in one coalesced load each: a thread that walked its level in global
// memory paid a memory round trip per handful of additions (measured: more than the tile launch).
__global__ __launch_bounds__(PL_THREADS) void pyr_reduce_k(const double* __restrict__ ws, double* __restrict__ loss, int L,
                                                           long long per_sample, PlCoef cf) {
  __shared__ double part[PL_MAX_LEVELS][PL_THREADS + 1];  // (+ 1: the L threads that add read one column of L rows at a time)
  __shared__ double sums[PL_MAX_LEVELS];
  const int s = threadIdx.x;
  const double* base = ws + (size_t)blockIdx.x * L * (size_t)per_sample;
  double acc = 0.0;
  for (long long k0 = 0; k0 < per_sample; k0 += PL_THREADS) {
    const int m = per_sample - k0 < PL_THREADS ? (int)(per_sample - k0) : PL_THREADS;
    if (s < m)
      for (int q = 0; q < L; ++q) part[q][s] = base[(size_t)q * (size_t)per_sample + (size_t)k0 + s];
    __syncthreads();
    if (s < L) {
#pragma unroll 8
      for (int k = 0; k < m; ++k) acc += part[s][k];
    }
    __syncthreads();
  }
  if (s < L) sums[s] = acc;
  __syncthreads();
  if (s == 0) {
    double l = 0.0;
#pragma unroll
    for (int q = 0; q < PL_MAX_LEVELS; ++q)
      if (q < L) l += cf.c[q] * sums[q];
    loss[blockIdx.x] = l;
  }
}

template <int L>
void pyr_launch(const PyrPlan& P, bool vec, const float* x, const float* t, float* g, double* ws, int c, int h, int w,
                const PlWeights& wt, hipStream_t stream) {
  const dim3 grid((unsigned)P.grid), block(PL_THREADS);
  if (vec)
    hipLaunchKernelGGL((pyr_tile_k<L, true>), grid, block, P.lds_bytes, stream, x, t, g, ws, c, h, w, P.tiles_y, P.tiles_x, wt);
  else
    hipLaunchKernelGGL((pyr_tile_k<L, false>), grid, block, P.lds_bytes, stream, x, t, g, ws, c, h, w, P.tiles_y, P.tiles_x, wt);
}

}  // namespace

extern "C" size_t mg_pyramid_l2_ws_bytes(int n, int c, int h, int w, int levels) { return pyr_plan(n, c, h, w, levels).ws_bytes; }

extern "C" int mg_pyramid_l2(const float* x, const float* t, int n, int c, int h, int w, int levels, const float* weights, double* loss,
                             float* grad, void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(x && t && weights && loss && ws && n > 0 && c > 0 && h > 0 && w > 0, "mg_pyramid_l2: bad arguments");
  MG_CHECK_ARG(levels >= 1 && levels <= PL_MAX_LEVELS, "mg_pyramid_l2: levels = %d outside 1 .. %d", levels, PL_MAX_LEVELS);
  MG_CHECK_ARG(h % (1 << (levels - 1)) == 0 && w % (1 << (levels - 1)) == 0,
               "mg_pyramid_l2: %d x %d is no multiple of %d, which %d levels need", h, w, 1 << (levels - 1), levels);
  const PyrPlan P = pyr_plan(n, c, h, w, levels);
  MG_CHECK_ARG(P.ok, "mg_pyramid_l2: %d x %d x %d x %d is more than one launch takes", n, c, h, w);
  MG_CHECK_ARG(P.lds_bytes <= PL_LDS_LIMIT, "mg_pyramid_l2: %zu bytes of LDS", P.lds_bytes);
  MG_CHECK_ARG(ws_bytes >= P.ws_bytes && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
               "mg_pyramid_l2: the workspace needs %zu bytes at an 8-byte boundary, got %zu", P.ws_bytes, ws_bytes);
  PlWeights wt;
  PlCoef cf;
  for (int s = 0; s < PL_MAX_LEVELS; ++s) {
    const float lam = s < levels ? weights[s] : 0.f;
    MG_CHECK_ARG(std::isfinite(lam) && lam >= 0.f, "mg_pyramid_l2: weight %d = %g is not a finite number >= 0", s, (double)lam);
    wt.lam[s] = lam;
    cf.c[s] = s < levels ? (double)lam / ((double)c * (double)(h >> s) * (double)(w >> s)) : 0.0;
  }
  wt.k = (float)(2.0 / ((double)c * (double)h * (double)w));
  if (grad != nullptr) {
    const size_t bytes = (size_t)P.elems * sizeof(float);
    const char *g0 = reinterpret_cast<const char*>(grad), *x0 = reinterpret_cast<const char*>(x), *t0 = reinterpret_cast<const char*>(t);
    MG_CHECK_ARG((g0 + bytes <= x0 || x0 + bytes <= g0) && (g0 + bytes <= t0 || t0 + bytes <= g0),
                 "mg_pyramid_l2: the gradient overlaps an input");
  }
  const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (reinterpret_cast<uintptr_t>(t) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(grad) & 15) == 0;
  double* part = reinterpret_cast<double*>(ws);
  hipStream_t st = (hipStream_t)stream;
  switch (levels) {
    case 1: pyr_launch<1>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    case 2: pyr_launch<2>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    case 3: pyr_launch<3>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    case 4: pyr_launch<4>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    case 5: pyr_launch<5>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    case 6: pyr_launch<6>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
    default: pyr_launch<7>(P, vec, x, t, grad, part, c, h, w, wt, st); break;
  }
  MG_CHECK_LAUNCH("mg_pyramid_l2");
  hipLaunchKernelGGL(pyr_reduce_k, dim3((unsigned)n), dim3(PL_THREADS), 0, st, part, loss, levels, P.tiles_per_sample, cf);
  MG_CHECK_LAUNCH("mg_pyramid_l2 (reduce)");
  return MG_OK;
}
