// Log-mel feature rows of magnitude images: the kernel behind mel_ops.logmel_rows and metrics.LogMel.
//
//   p[h,t] = (x[n,c,h,t] scale[h] + scale[h])^2                       float32, three roundings
//   s[m,t] = sum over h in [lo[m], hi[m]) of weight[m,h] p[h,t]       float32, ascending h, product and sum rounded apart
//   v[m,t] = log((double)s[m,t] + floor)                              float64
//   out[n, m P + j] = (float)(sum of v[m,t] over the W / P columns of pool j, ascending t, / (W / P))
//
// A workgroup owns one image, LM_G neighbouring bands and one tile of columns: a whole number of pools, 64 columns where a pool is
// narrower than a wave, the pool itself where it is wider.  Its (band, column) pairs are dealt to the threads column-fastest, so a
// wave reads 256 consecutive bytes of one image row per load and, with a tile of 64 columns, each of the four waves walks one band.
// A lane keeps one float32 accumulator and LM_LOADS rows in flight; the rows two neighbouring bands share are read again by the
// next band and come from the cache.  The logarithms of a tile go to LDS as float64, one thread per (band, pool) then adds its
// pool's columns in ascending order: a chain of W / P additions, fixed by the shape alone.  A row of `out` is therefore a function
// of its image and of the shapes; nothing is accumulated across workgroups, there are no atomics and no scratch memory.
//
// The band limits arrive as HOST arrays, are checked against H on the host and passed to the kernel by value: no row index that the
// kernel forms depends on device memory.
#include <cmath>

#include "mg_common.h"

namespace {

constexpr int LM_G = 4;             // bands per workgroup
constexpr int LM_LOADS = 8;         // rows a lane has in flight (no part of the result)
constexpr int LM_MAX_BANDS = 256;   // band limits passed by value: 2 KB of kernel arguments
constexpr int LM_MAX_POOL = 1024;   // widest pool: LM_G x 1024 float64 of LDS
constexpr int LM_MAX_IMAGES = 32768;   // images per launch (grid z)

struct LmBands {
  int lo[LM_MAX_BANDS];
  int hi[LM_MAX_BANDS];
};

template <int UNITS>   // LM_G x the widest tile, in float64 of LDS
__global__ void __launch_bounds__(256) logmel_rows_k(const float* __restrict__ x, const float* __restrict__ scale,
                                                     const float* __restrict__ weight, const LmBands bands, float* __restrict__ out,
                                                     int C, int c, int H, int W, int M, int P, int pw, int tw, double floor_) {
  __shared__ double sv[UNITS];
  __shared__ int s_lo[LM_G], s_hi[LM_G];
  const int tid = threadIdx.x, m0 = blockIdx.y * LM_G, col0 = blockIdx.x * tw;
  const size_t img = blockIdx.z;
  if (tid < LM_G) {
    const int m = m0 + tid;
    s_lo[tid] = m < M ? bands.lo[m] : 0;
    s_hi[tid] = m < M ? bands.hi[m] : 0;
  }
  __syncthreads();
  const float* plane = x + (img * C + c) * (size_t)H * W;
  for (int u = tid; u < LM_G * tw; u += 256) {
    const int g = u / tw, col = col0 + (u - g * tw), m = m0 + g;
    double v = 0.0;
    if (m < M && col < W) {
      const int lo = s_lo[g], hi = s_hi[g];
      const float* wrow = weight + (size_t)m * H;
      const float* px = plane + col;
      float s = 0.f;
      for (int h0 = lo; h0 < hi; h0 += LM_LOADS) {   // LM_LOADS rows in flight, added in ascending h
        float xv[LM_LOADS], sc[LM_LOADS], wv[LM_LOADS];
#pragma unroll
        for (int q = 0; q < LM_LOADS; ++q) {
          const int h = min(h0 + q, hi - 1);   // past the band's end: its last row again, loaded and not added
          xv[q] = px[(size_t)h * W];
          sc[q] = scale[h];
          wv[q] = wrow[h];
        }
#pragma unroll
        for (int q = 0; q < LM_LOADS; ++q) {
          if (h0 + q < hi) {
            float t = xv[q] * sc[q];
            t = t + sc[q];
            s = s + wv[q] * (t * t);
          }
        }
      }
      v = log((double)s + floor_);
    }
    sv[u] = v;
  }
  __syncthreads();
  const int ppt = tw / pw;   // pools of a tile
  for (int q = tid; q < LM_G * ppt; q += 256) {
    const int g = q / ppt, jp = q - g * ppt, m = m0 + g, pool = blockIdx.x * ppt + jp;
    if (m < M && pool < P) {
      const double* p = sv + g * tw + jp * pw;
      double a = p[0];
      for (int t = 1; t < pw; ++t) a += p[t];
      out[(img * M + m) * (size_t)P + pool] = (float)(a / (double)pw);
    }
  }
}

}  // namespace

extern "C" int mg_logmel_rows(const float* x, int n, int channels, int c, int h, int w, const float* scale, const float* weight,
                              const int32_t* lo, const int32_t* hi, int bands, double floor, int pools, float* out,
                              mg_stream_t stream) {
  MG_CHECK_ARG(x && scale && weight && lo && hi && out, "mg_logmel_rows: bad arguments");
  MG_CHECK_ARG(n >= 1 && channels >= 1 && c >= 0 && c < channels && h >= 1 && w >= 1,
               "mg_logmel_rows: n, channels, h, w >= 1 and 0 <= c < channels expected, got %d %d %d %d and c = %d", n, channels, h, w, c);
  MG_CHECK_ARG(bands >= 1 && bands <= LM_MAX_BANDS, "mg_logmel_rows: bands in 1 .. %d expected, got %d", LM_MAX_BANDS, bands);
  MG_CHECK_ARG(pools >= 1 && w % pools == 0, "mg_logmel_rows: a pool count that divides w = %d expected, got %d", w, pools);
  const int pw = w / pools;
  MG_CHECK_ARG(pw <= LM_MAX_POOL, "mg_logmel_rows: pools of at most %d columns expected, got %d", LM_MAX_POOL, pw);
  MG_CHECK_ARG(floor > 0.0 && std::isfinite(floor), "mg_logmel_rows: a finite floor > 0 expected");
  MG_CHECK_ARG((long long)h * w < (1ll << 31), "mg_logmel_rows: planes of %d x %d are more than one launch takes", h, w);
  LmBands b;
  for (int m = 0; m < LM_MAX_BANDS; ++m) {
    b.lo[m] = m < bands ? lo[m] : 0;
    b.hi[m] = m < bands ? hi[m] : 0;
    MG_CHECK_ARG(0 <= b.lo[m] && b.lo[m] <= b.hi[m] && b.hi[m] <= h, "mg_logmel_rows: band %d: 0 <= lo <= hi <= %d expected, got %d, %d",
                 m, h, b.lo[m], b.hi[m]);
  }
  const int ppt = pw >= 64 ? 1 : 64 / pw, tw = ppt * pw;
  const unsigned tiles = (unsigned)((pools + ppt - 1) / ppt), groups = (unsigned)((bands + LM_G - 1) / LM_G);
  const size_t in_img = (size_t)channels * h * w, out_img = (size_t)bands * pools;
  for (int n0 = 0; n0 < n; n0 += LM_MAX_IMAGES) {
    const dim3 grid(tiles, groups, (unsigned)(n - n0 < LM_MAX_IMAGES ? n - n0 : LM_MAX_IMAGES));
    if (tw <= 64)
      hipLaunchKernelGGL(logmel_rows_k<LM_G * 64>, grid, dim3(256), 0, (hipStream_t)stream, x + n0 * in_img, scale, weight, b,
                         out + n0 * out_img, channels, c, h, w, bands, pools, pw, tw, floor);
    else
      hipLaunchKernelGGL(logmel_rows_k<LM_G * LM_MAX_POOL>, grid, dim3(256), 0, (hipStream_t)stream, x + n0 * in_img, scale, weight, b,
                         out + n0 * out_img, channels, c, h, w, bands, pools, pw, tw, floor);
  }
  MG_CHECK_LAUNCH("mg_logmel_rows");
  return MG_OK;
}
