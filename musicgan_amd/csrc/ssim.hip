// Multi-scale structural similarity (Wang, Simoncelli & Bovik 2003; used for sample diversity by Karras et al., ICLR 2018) between
// pairs of images: the kernels behind metrics.ms_ssim / metrics.MSSSIM.  The reference project has no such metric; the definition
// implemented here is the one DESIGN.md states ("Evaluation: MS-SSIM sample diversity").
//
//   scale     ssim_scale_k, one launch per scale.  A workgroup takes one tile of SS_TH x SS_TW = 32 x 64 valid outputs of one
//             channel plane of one pair.  It stages the (32 + 10) x (64 + 10) pixels of a and of b that the tile needs in LDS
//             (zeros beyond the image), writes the 2 x 2 means of the part of the plane it owns (its 32 x 64 corner pixels; the
//             last tile of a row / column also owns the 10-pixel rim) as the next scale's input, runs the horizontal pass of the
//             five maps (a, b, a^2, b^2, ab) from LDS into LDS, the vertical pass from LDS into registers, forms cs and ssim per
//             pixel and leaves the tile's two float64 sums in its own slot [pair, channel, tile, 2]: nothing is added atomically.
//   LDS       a and b rows have a stride of 78 dwords: the horizontal pass reads 8-byte pairs at column 4 q + 2 j, 16 lanes per
//             row, so the two rows of a 32-lane ds_read_b64 group cover the 64 banks once (78 = 14 mod 64 puts the second row's
//             pairs into the gaps of the first).  The filtered maps have a stride of 64: a thread stores 4 columns as one
//             16-byte write (8 lanes = 32 consecutive dwords) and the vertical pass reads one dword per lane, consecutive lanes
//             consecutive columns.  79 968 bytes per workgroup: two workgroups per CU.
//   registers a thread of the horizontal pass makes 4 columns x 5 maps of one row out of 14 + 14 pixels; a thread of the vertical
//             pass makes 8 rows x 5 maps of one column out of 18 rows: 40 accumulators, every index known at compile time.
//   finish    ssim_finish_k, one thread per pair: adds the slots of every scale in index order, forms the S means, clamps, raises
//             to the weights and multiplies, all in float64.  ssim_mean_k: the mean of the per-pair values in an order that
//             depends on their number alone.
// The same instruction sequence filters all five maps, and every sum of two terms is written so that exchanging a and b
// exchanges the operands of commutative operations only: ms_ssim(x, x) is exactly 1 and ms_ssim(a, b) == ms_ssim(b, a) bit for bit.
#include <cmath>

#include "mg_common.h"

namespace {

constexpr int SS_WIN = 11, SS_HALO = SS_WIN - 1, SS_MAX_SCALES = 5;
constexpr int SS_TW = 64, SS_TH = 32, SS_R = 8;              // valid outputs per tile; rows per thread of the vertical pass
constexpr int SS_IW = SS_TW + SS_HALO, SS_IH = SS_TH + SS_HALO;  // staged pixels: 74 x 42
constexpr int SS_SA = 78;                                    // row stride of the staged images, dwords
constexpr int SS_AB = SS_IH * SS_SA, SS_HM = SS_IH * SS_TW;  // dwords per staged image / per horizontally filtered map
constexpr size_t SS_LDS = (size_t)(2 * SS_AB + 5 * SS_HM) * sizeof(float);
constexpr float SS_C1 = 0.0004f, SS_C2 = 0.0036f;            // (0.01 L)^2, (0.03 L)^2 for L = 2
static_assert(SS_TH == 4 * SS_R && SS_TW == 64, "the vertical pass maps 4 waves x 64 lanes to 4 strips x 64 columns");
static_assert(2 * SS_LDS <= 160 * 1024, "two workgroups per CU");

struct SsimTaps {
  float g[SS_WIN];
};
struct SsimWeights {
  double w[SS_MAX_SCALES];
};
typedef float f32x2 __attribute__((ext_vector_type(2)));

int ssim_scales(int H, int W) {
  if (H < SS_WIN || W < SS_WIN) return 0;
  int s = 1;
  while (s < SS_MAX_SCALES && H % (1 << s) == 0 && W % (1 << s) == 0 && ((H < W ? H : W) >> s) >= SS_WIN) ++s;
  return s;
}
__host__ __device__ inline int ssim_tiles_x(int W) { return (W - SS_HALO + SS_TW - 1) / SS_TW; }
__host__ __device__ inline int ssim_tiles_y(int H) { return (H - SS_HALO + SS_TH - 1) / SS_TH; }
__host__ __device__ inline int ssim_tiles(int H, int W) { return ssim_tiles_x(W) * ssim_tiles_y(H); }

void ssim_window(float* g) {  // float64 taps, divided by their sum, then rounded
  double t[SS_WIN], sum = 0.0;
  for (int i = 0; i < SS_WIN; ++i) {
    const double d = (double)(i - SS_WIN / 2);
    t[i] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += t[i];
  }
  for (int i = 0; i < SS_WIN; ++i) g[i] = (float)(t[i] / sum);
}

__global__ void __launch_bounds__(256, 2) ssim_scale_k(const float* __restrict__ a, const float* __restrict__ b,
                                                       float* __restrict__ a_next, float* __restrict__ b_next,
                                                       double* __restrict__ slots, int H, int W, int ntx, int ntiles, SsimTaps taps) {
  extern __shared__ __attribute__((aligned(16))) float ss_lds[];
  float* sa = ss_lds;
  float* sb = sa + SS_AB;
  float* hm = sb + SS_AB;
  const int tid = threadIdx.x;
  const int tile = blockIdx.x % ntiles;
  const size_t plane = blockIdx.x / ntiles;
  const int ty = tile / ntx, tx = tile - ty * ntx;
  const int oy0 = ty * SS_TH, ox0 = tx * SS_TW;
  const float* pa = a + plane * (size_t)H * W;
  const float* pb = b + plane * (size_t)H * W;

  for (int i = tid; i < SS_IH * SS_IW; i += 256) {
    const int r = i / SS_IW, c = i - r * SS_IW;
    const int gy = oy0 + r, gx = ox0 + c;
    const bool ok = gy < H && gx < W;  // a tile that overhangs the image reads zeros there and counts no output there
    const size_t off = ok ? (size_t)gy * W + gx : 0;
    const float va = pa[off], vb = pb[off];
    sa[r * SS_SA + c] = ok ? va : 0.f;
    sb[r * SS_SA + c] = ok ? vb : 0.f;
  }
  __syncthreads();

  if (a_next != nullptr) {  // the next scale's input: the 2 x 2 means of the pixels this tile owns (H, W, oy0 and ox0 are even)
    const int rows = (oy0 + SS_TH + SS_HALO >= H ? H - oy0 : SS_TH) >> 1;
    const int cols = (ox0 + SS_TW + SS_HALO >= W ? W - ox0 : SS_TW) >> 1;
    const int Wn = W >> 1;
    const size_t base = plane * (size_t)(H >> 1) * Wn + (size_t)(oy0 >> 1) * Wn + (ox0 >> 1);
    for (int i = tid; i < rows * cols; i += 256) {
      const int r = i / cols, c = i - r * cols;
      const float* qa = sa + 2 * r * SS_SA + 2 * c;
      const float* qb = sb + 2 * r * SS_SA + 2 * c;
      a_next[base + (size_t)r * Wn + c] = ((qa[0] + qa[1]) + (qa[SS_SA] + qa[SS_SA + 1])) * 0.25f;
      b_next[base + (size_t)r * Wn + c] = ((qb[0] + qb[1]) + (qb[SS_SA] + qb[SS_SA + 1])) * 0.25f;
    }
  }

  // horizontal pass: an item is 4 neighbouring columns of one staged row, all five maps
  for (int it = tid; it < SS_IH * (SS_TW / 4); it += 256) {
    const int r = it >> 4, q = it & 15;
    const f32x2* ra = reinterpret_cast<const f32x2*>(sa + r * SS_SA + 4 * q);
    const f32x2* rb = reinterpret_cast<const f32x2*>(sb + r * SS_SA + 4 * q);
    float va[14], vb[14];
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const f32x2 u = ra[j], v = rb[j];
      va[2 * j] = u[0];
      va[2 * j + 1] = u[1];
      vb[2 * j] = v[0];
      vb[2 * j + 1] = v[1];
    }
    float o[5][4];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[m][j] = 0.f;
#pragma unroll
    for (int k = 0; k < 14; ++k) {
      const float x = va[k], y = vb[k];
      const float v[5] = {x, y, x * x, y * y, x * y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (k - j >= 0 && k - j < SS_WIN) {
          const float w = taps.g[k - j];
#pragma unroll
          for (int m = 0; m < 5; ++m) o[m][j] = __builtin_fmaf(w, v[m], o[m][j]);
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
      *reinterpret_cast<f32x4*>(hm + m * SS_HM + r * SS_TW + 4 * q) = f32x4{o[m][0], o[m][1], o[m][2], o[m][3]};
  }
  __syncthreads();

  // vertical pass: a thread takes SS_R rows of one column; a wave takes one strip of rows, its lanes consecutive columns
  const int x = tid & 63, row0 = (tid >> 6) * SS_R;
  float acc[5][SS_R];
#pragma unroll
  for (int m = 0; m < 5; ++m)
#pragma unroll
    for (int j = 0; j < SS_R; ++j) acc[m][j] = 0.f;
#pragma unroll
  for (int k = 0; k < SS_R + SS_HALO; ++k) {
    float v[5];
#pragma unroll
    for (int m = 0; m < 5; ++m) v[m] = hm[m * SS_HM + (row0 + k) * SS_TW + x];
#pragma unroll
    for (int j = 0; j < SS_R; ++j) {
      if (k - j >= 0 && k - j < SS_WIN) {
        const float w = taps.g[k - j];
#pragma unroll
        for (int m = 0; m < 5; ++m) acc[m][j] = __builtin_fmaf(w, v[m], acc[m][j]);
      }
    }
  }
  double dcs = 0.0, dss = 0.0;
  const bool col_ok = ox0 + x < W - SS_HALO;
#pragma unroll
  for (int j = 0; j < SS_R; ++j) {
    const float mua = acc[0][j], mub = acc[1][j];
    const float mab = mua * mub, maa = mua * mua, mbb = mub * mub;
    const float saa = acc[2][j] - maa, sbb = acc[3][j] - mbb, sab = acc[4][j] - mab;
    const float cs = (2.f * sab + SS_C2) / ((saa + sbb) + SS_C2);
    const float lum = (2.f * mab + SS_C1) / ((maa + mbb) + SS_C1);
    const float ss = cs * lum;
    if (col_ok && oy0 + row0 + j < H - SS_HALO) {
      dcs += (double)cs;
      dss += (double)ss;
    }
  }
  // the tile's sums: lanes of a wave in a fixed tree, then the four waves in order (the staged images are no longer read)
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    dcs += __shfl_down(dcs, s);
    dss += __shfl_down(dss, s);
  }
  double* red = reinterpret_cast<double*>(ss_lds);
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = dcs;
    red[2 * (tid >> 6) + 1] = dss;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = slots + ((size_t)plane * ntiles + tile) * 2;
    o[0] = ((red[0] + red[2]) + red[4]) + red[6];
    o[1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

__global__ void __launch_bounds__(64) ssim_finish_k(const double* __restrict__ slots, long long n, int C, int H, int W, int S,
                                                    SsimWeights wts, double* __restrict__ values, double* __restrict__ terms,
                                                    long long row0) {
  const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  size_t off = 0;
  double prod = 1.0;
  for (int s = 0; s < S; ++s) {
    const int h = H >> s, w = W >> s;
    const size_t cnt = (size_t)C * ssim_tiles(h, w);
    const double* q = slots + off + (size_t)i * cnt * 2;
    double cs = 0.0, ss = 0.0;
    for (size_t t = 0; t < cnt; ++t) {
      cs += q[2 * t];
      ss += q[2 * t + 1];
    }
    const double mean = (s == S - 1 ? ss : cs) / ((double)C * (double)(h - SS_HALO) * (double)(w - SS_HALO));
    if (terms != nullptr) terms[(size_t)(row0 + i) * S + s] = mean;
    prod *= pow(mean < 0.0 ? 0.0 : mean, wts.w[s]);  // the clamp: a negative mean scores 0 (a NaN stays a NaN)
    off += (size_t)n * cnt * 2;
  }
  values[row0 + i] = prod;
}

__global__ void __launch_bounds__(256) ssim_mean_k(const double* __restrict__ values, long long n, double* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (long long i = threadIdx.x; i < n; i += 256) acc += values[i];
  acc = mg_block_sum_f64(acc, red);
  if (threadIdx.x == 0) out[0] = acc / (double)n;
}

size_t ssim_slot_doubles(int64_t N, int C, int H, int W) {
  size_t total = 0;
  for (int s = 0, S = ssim_scales(H, W); s < S; ++s) total += (size_t)N * C * ssim_tiles(H >> s, W >> s) * 2;
  return total;
}

}  // namespace

extern "C" int mg_ssim_scales(int H, int W) { return ssim_scales(H, W); }

extern "C" int mg_ssim_window(float* taps) {
  MG_CHECK_ARG(taps, "mg_ssim_window: bad arguments");
  ssim_window(taps);
  return MG_OK;
}

extern "C" int64_t mg_ssim_tiles(int H, int W) { return H < SS_WIN || W < SS_WIN ? 0 : (int64_t)ssim_tiles(H, W); }

extern "C" size_t mg_ssim_scratch_bytes(int64_t N, int C, int H, int W) {
  const int S = ssim_scales(H, W);
  if (S < 1 || N < 1 || C < 1) return 0;
  size_t bytes = ssim_slot_doubles(N, C, H, W) * sizeof(double);
  for (int s = 1; s < S; ++s) bytes += 2 * (size_t)N * C * (H >> s) * (W >> s) * sizeof(float);
  return bytes;
}

extern "C" int mg_ssim_scale(const float* a, const float* b, float* a_next, float* b_next, double* slots, int64_t N, int C, int H, int W,
                             mg_stream_t stream) {
  MG_CHECK_ARG(a && b && slots && N > 0 && C > 0, "mg_ssim_scale: bad arguments");
  MG_CHECK_ARG(H >= SS_WIN && W >= SS_WIN, "mg_ssim_scale: sides >= %d expected, got %dx%d", SS_WIN, H, W);
  MG_CHECK_ARG((a_next == nullptr) == (b_next == nullptr), "mg_ssim_scale: both or none of the next scale's images expected");
  MG_CHECK_ARG(a_next == nullptr || (H % 2 == 0 && W % 2 == 0), "mg_ssim_scale: even sides expected for the 2x2 means, got %dx%d", H, W);
  const int ntx = ssim_tiles_x(W), ntiles = ssim_tiles(H, W);
  const int64_t blocks = N * C * (int64_t)ntiles;
  MG_CHECK_ARG(blocks < (1ll << 31), "mg_ssim_scale: batch too large (%lld tiles)", (long long)blocks);
  static MgPerDevice once;
  if (mg_first_use_on_device(once))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ssim_scale_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SS_LDS);
  SsimTaps taps;
  ssim_window(taps.g);
  hipLaunchKernelGGL(ssim_scale_k, dim3((unsigned)blocks), dim3(256), SS_LDS, (hipStream_t)stream, a, b, a_next, b_next, slots, H, W, ntx,
                     ntiles, taps);
  MG_CHECK_LAUNCH("mg_ssim_scale");
  return MG_OK;
}

extern "C" int mg_ssim_finish(const double* slots, size_t slot_doubles, int64_t N, int C, int H, int W, double* values, double* terms,
                              int64_t row0, int64_t rows_total, mg_stream_t stream) {
  MG_CHECK_ARG(slots && values && N > 0 && C > 0, "mg_ssim_finish: bad arguments");
  const int S = ssim_scales(H, W);
  MG_CHECK_ARG(S >= 1, "mg_ssim_finish: sides >= %d expected, got %dx%d", SS_WIN, H, W);
  MG_CHECK_ARG(slot_doubles == ssim_slot_doubles(N, C, H, W), "mg_ssim_finish: %zu slot values given, %zu expected", slot_doubles,
               ssim_slot_doubles(N, C, H, W));
  MG_CHECK_ARG(row0 >= 0 && row0 + N <= rows_total, "mg_ssim_finish: rows %lld .. %lld do not fit a buffer of %lld rows",
               (long long)row0, (long long)(row0 + N), (long long)rows_total);
  static const double full[SS_MAX_SCALES] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
  SsimWeights wts = {};
  double sum = 0.0;
  for (int s = 0; s < S; ++s) sum += full[s];
  for (int s = 0; s < S; ++s) wts.w[s] = full[s] / sum;
  hipLaunchKernelGGL(ssim_finish_k, dim3((unsigned)((N + 63) / 64)), dim3(64), 0, (hipStream_t)stream, slots, (long long)N, C, H, W, S,
                     wts, values, terms, (long long)row0);
  MG_CHECK_LAUNCH("mg_ssim_finish");
  return MG_OK;
}

extern "C" int mg_ssim_mean(const double* values, int64_t n, double* out, mg_stream_t stream) {
  MG_CHECK_ARG(values && out && n > 0, "mg_ssim_mean: bad arguments");
  hipLaunchKernelGGL(ssim_mean_k, dim3(1), dim3(256), 0, (hipStream_t)stream, values, (long long)n, out);
  MG_CHECK_LAUNCH("mg_ssim_mean");
  return MG_OK;
}
