// Sliced Wasserstein distance between local patches of Laplacian-pyramid levels (Karras et al., "Progressive Growing of GANs",
// ICLR 2018, section 5 / appendix): the kernels behind musicgan_amd/metrics.py.  The reference project has no such metric; the
// definition implemented here is the one DESIGN.md states ("Evaluation: sliced Wasserstein distance").
//
//   pyramid   swd_down_k: G_{i+1} = (G_i * g) at even rows / columns, g = outer([1,4,6,4,1]/16), mirrored borders (torch "reflect").
//             swd_lap_k:  L_i = G_i - up(G_{i+1}); up = zero-stuffing then 4g, of which only the taps that land on an even (non-zero)
//             position are evaluated: 3 x 3, 3 x 2, 2 x 3 or 2 x 2 of the 5 x 5, by the parity of the output row / column (mirroring
//             keeps an index's parity, so the parity of y + dy decides).
//   gather    one workgroup per image copies its P patches (C x p x p each, channel-major) into the (M, K) descriptor buffer at a
//             row offset and leaves that image's per-channel (sum, sum of squares) in float64.  swd_stats_finish_k adds the per-image
//             pairs in a fixed order: the statistics do not depend on how the images were split into batches, nor on the run.
//   project   out[d][m] = sum_k ((desc[m][k] - mean_c) * rstd_c) * dirs[d][k] on v_mfma_f32_16x16x4_f32: the directions of a block
//             (up to 128 x K) stay in LDS, tiles of 64 descriptors stream through it; K = 98 is padded to 100 in registers (the
//             lanes of the last k-step that would read k >= K take zeros).  A row stride of K = 98 = 2 (mod 32) dwords makes the
//             16 rows x 2 k of a ds_read_b32 lane group hit 32 different banks.  The tile is direction-major so that every sort
//             segment is contiguous.
//   sort      segmented bitonic sort of S contiguous segments of M floats, in place, any M: tiles of 2^14 keys are sorted in LDS,
//             the merge phases above that size run their wide strides in global memory and their last 14 strides in LDS again.
//             The network is the form whose compare-exchanges all point the same way (first step of a merge mirrored, then
//             half-cleaners), so a segment is padded to a power of two with +inf that is never stored: a pair whose upper index
//             is >= M is skipped.  A segment is cdiv(M, 2^14) workgroups' job.  NaN is outside the contract (a NaN never swaps).
//   distance  mean |a - b| of two sorted arrays: per-workgroup float64 partial sums, then one workgroup adds them in a fixed order.
#include "mg_common.h"

namespace {

__device__ __forceinline__ int swd_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

// ------------------------------------------------------------------ pyramid
__global__ void __launch_bounds__(256) swd_down_k(const float* __restrict__ x, float* __restrict__ out, int H, int W, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int Wo = W >> 1, Ho = H >> 1;
  const int ox = (int)(idx % Wo);
  const size_t t = idx / Wo;
  const int oy = (int)(t % Ho);
  const float* p = x + (t / Ho) * (size_t)H * W;
  const float k[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
  int xs[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) xs[d] = swd_reflect(2 * ox + d - 2, W);
  float acc = 0.f;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const float* row = p + (size_t)swd_reflect(2 * oy + dy - 2, H) * W;
    float r = 0.f;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) r += k[dx] * row[xs[dx]];
    acc += k[dy] * r;
  }
  out[idx] = acc;
}

__global__ void __launch_bounds__(256) swd_lap_k(const float* __restrict__ x, const float* __restrict__ coarse,
                                                 float* __restrict__ out, int H, int W, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int xx = (int)(idx % W);
  const size_t t = idx / W;
  const int y = (int)(t % H);
  const int Wc = W >> 1;
  const float* c = coarse + (t / H) * (size_t)(H >> 1) * Wc;
  const float k2[5] = {0.125f, 0.5f, 0.75f, 0.5f, 0.125f};  // 2 * [1,4,6,4,1]/16 per axis = 4 g
  float up = 0.f;
#pragma unroll
  for (int dy = -2; dy <= 2; ++dy) {
    if ((y + dy) & 1) continue;  // a zero of the stuffed image
    const float* row = c + (size_t)(swd_reflect(y + dy, H) >> 1) * Wc;
    float r = 0.f;
#pragma unroll
    for (int dx = -2; dx <= 2; ++dx) {
      if ((xx + dx) & 1) continue;
      r += k2[dx + 2] * row[swd_reflect(xx + dx, W) >> 1];
    }
    up += k2[dy + 2] * r;
  }
  out[idx] = x[idx] - up;
}

// ------------------------------------------------------------------ gather + statistics
__global__ void __launch_bounds__(256) swd_gather_k(const float* __restrict__ img, const int* __restrict__ centres,
                                                    float* __restrict__ desc, double* __restrict__ stats, int C, int H, int W, int P,
                                                    int p, size_t row0) {
  __shared__ double red[256];
  const int n = blockIdx.x, half = p >> 1, pp = p * p, K = C * pp;
  const int* cen = centres + (size_t)n * P * 2;
  float* drow = desc + (row0 + (size_t)n * P) * K;
  for (int c = 0; c < C; ++c) {
    const float* plane = img + ((size_t)n * C + c) * H * W;
    double s = 0.0, q = 0.0;
    for (int e = threadIdx.x; e < P * pp; e += 256) {
      const int j = e / pp, t = e - j * pp, r = t / p, col = t - r * p;
      int cy = cen[2 * j], cx = cen[2 * j + 1];
      cy = min(max(cy, half), H - 1 - half);  // an illegal centre is clamped, never read out of bounds
      cx = min(max(cx, half), W - 1 - half);
      const float v = plane[(size_t)(cy - half + r) * W + cx - half + col];
      drow[(size_t)j * K + c * pp + t] = v;
      s += (double)v;
      q += (double)v * (double)v;  // exact: a float32 squared has 48 significant bits
    }
    s = mg_block_sum_f64(s, red);
    q = mg_block_sum_f64(q, red);
    if (threadIdx.x == 0) {
      double* o = stats + ((row0 / P + n) * C + c) * 2;
      o[0] = s;
      o[1] = q;
    }
  }
}

// norm[c] = (mean, 1 / std, std) in float32, each rounded once from float64; a constant channel gets 1 / std = 0
__global__ void __launch_bounds__(256) swd_stats_finish_k(const double* __restrict__ stats, float* __restrict__ norm, long long images,
                                                          int C, double count) {
  __shared__ double red[256];
  const int c = blockIdx.x;
  double s = 0.0, q = 0.0;
  for (long long i = threadIdx.x; i < images; i += 256) {
    s += stats[(i * C + c) * 2];
    q += stats[(i * C + c) * 2 + 1];
  }
  s = mg_block_sum_f64(s, red);
  q = mg_block_sum_f64(q, red);
  if (threadIdx.x == 0) {
    const double mean = s / count;
    double var = q / count - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double sd = sqrt(var);
    norm[3 * c] = (float)mean;
    norm[3 * c + 1] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
    norm[3 * c + 2] = (float)sd;
  }
}

// ------------------------------------------------------------------ projection
constexpr int PJ_BM = 64;    // descriptors per tile (16 per wave)
constexpr int PJ_DT = 128;   // directions per workgroup (8 MFMA tiles of 16)

__global__ void __launch_bounds__(256, 2) swd_project_k(const float* __restrict__ desc, const float* __restrict__ norm,
                                                        const float* __restrict__ dirs, float* __restrict__ out, long long M, int K,
                                                        int pp, int D, int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float pj_lds[];
  float* dirsL = pj_lds;                    // [PJ_DT][K]
  float* descL = dirsL + PJ_DT * K;         // [PJ_BM][K]
  float* meanL = descL + PJ_BM * K;         // [K]
  float* rstdL = meanL + K;                 // [K]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ml = lane & 15, kq = lane >> 4;
  const int d0 = blockIdx.y * PJ_DT;
  const int nd = min(PJ_DT, D - d0), ndt = (nd + 15) >> 4;
  for (int i = tid; i < ndt * 16 * K; i += 256) dirsL[i] = i < nd * K ? dirs[(size_t)d0 * K + i] : 0.f;
  for (int k = tid; k < K; k += 256) {
    meanL[k] = norm[3 * (k / pp)];
    rstdL[k] = norm[3 * (k / pp) + 1];
  }
  const bool vec_ok = (reinterpret_cast<size_t>(desc) & 15) == 0;
  const int kstep = 1024 % K, ksteps = (K + 3) >> 2;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long m0 = (long long)tile * PJ_BM;
    const int rows = (int)min((long long)PJ_BM, M - m0);
    const int lim = rows * K;
    const float* src = desc + (size_t)m0 * K;  // 16-byte aligned with desc: PJ_BM * K * 4 is a multiple of 16
    __syncthreads();  // the previous tile's operand reads are done; first pass: dirsL / meanL / rstdL are written
    int k = (tid * 4) % K;
    for (int i = tid * 4; i < PJ_BM * K; i += 1024) {
      float v[4];
      if (vec_ok && i + 3 < lim) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(src + i);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = i + u < lim ? src[i + u] : 0.f;  // never past the last row
      }
      int ku = k;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        descL[i + u] = i + u < lim ? (v[u] - meanL[ku]) * rstdL[ku] : 0.f;
        ku = ku + 1 == K ? 0 : ku + 1;
      }
      k += kstep;
      k = k >= K ? k - K : k;
    }
    __syncthreads();
    f32x4 acc[PJ_DT / 16];
#pragma unroll
    for (int t = 0; t < PJ_DT / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* brow = descL + (w * 16 + ml) * K;
    const float* arow = dirsL + ml * K;
    for (int ks = 0; ks < ksteps; ++ks) {
      const int kk = ks * 4 + kq;
      const bool ok = kk < K;  // K is padded to a multiple of 4 with zeros, in registers
      const int ka = ok ? kk : 0;
      const float b = ok ? brow[ka] : 0.f;
#pragma unroll
      for (int t = 0; t < PJ_DT / 16; ++t) {
        if (t < ndt) {
          const float a = ok ? arow[t * 16 * K + ka] : 0.f;
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[t], 0, 0, 0);
        }
      }
    }
    const long long m = m0 + w * 16 + ml;
#pragma unroll
    for (int t = 0; t < PJ_DT / 16; ++t) {
      if (t < ndt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int d = d0 + t * 16 + kq * 4 + r;
          if (d < D && m < M) out[(size_t)d * M + m] = acc[t][r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ segmented sort
constexpr int SB_LOG = 14, SB = 1 << SB_LOG, ST = 1024;  // keys per LDS tile (64 KB: two workgroups per CU), threads per workgroup

__device__ __forceinline__ void swd_cas(float* s, int i, int j) {
  const float a = s[i], b = s[j];
  if (a > b) {
    s[i] = b;
    s[j] = a;
  }
}

// full == 1: bitonic sort of the tile's 2^nlog keys (nlog <= SB_LOG); full == 0: the half-cleaners of strides SB/2 .. 1 that finish a
// merge phase whose wider strides ran in global memory
__global__ void __launch_bounds__(ST) swd_sort_tile_k(float* __restrict__ x, long long M, int nlog, int full) {
  __shared__ float s[SB];
  float* seg = x + (size_t)blockIdx.y * M;
  const long long base = (long long)blockIdx.x * SB;
  const int n = 1 << nlog, tid = threadIdx.x;
  for (int i = tid; i < n; i += ST) s[i] = base + i < M ? seg[base + i] : INFINITY;
  __syncthreads();
  for (int k = full ? 1 : nlog; k <= nlog; ++k) {
    int j = 1 << (k - 1);
    if (full) {  // first step of the merge of two sorted runs of 2^(k-1): run i against the mirror of its neighbour
      for (int p = tid; p < n / 2; p += ST) {
        const int o = p & (j - 1), b = (p >> (k - 1)) << k;
        swd_cas(s, b + o, b + 2 * j - 1 - o);
      }
      __syncthreads();
      j >>= 1;
    }
    for (; j >= 1; j >>= 1) {
      for (int p = tid; p < n / 2; p += ST) {
        const int i = 2 * p - (p & (j - 1));
        swd_cas(s, i, i + j);
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n; i += ST)
    if (base + i < M) seg[base + i] = s[i];
}

// one compare-exchange step in global memory: flip != 0: the mirrored first step of the merge into runs of 2^k; else the
// half-cleaner of stride j.  pairs whose upper index is >= M hold a virtual +inf there and are skipped.
__global__ void __launch_bounds__(256) swd_sort_global_k(float* __restrict__ x, long long M, long long npairs, int k, long long j,
                                                         int flip) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npairs) return;
  float* seg = x + (size_t)blockIdx.y * M;
  long long lo, hi;
  if (flip) {
    const long long h = 1ll << (k - 1), o = p & (h - 1), b = (p >> (k - 1)) << k;
    lo = b + o;
    hi = b + 2 * h - 1 - o;
  } else {
    lo = 2 * p - (p & (j - 1));
    hi = lo + j;
  }
  if (hi >= M) return;
  const float a = seg[lo], b2 = seg[hi];
  if (a > b2) {
    seg[lo] = b2;
    seg[hi] = a;
  }
}

// ------------------------------------------------------------------ distance
constexpr int DIST_MAX_BLOCKS = 2048;

__global__ void __launch_bounds__(256) swd_absdiff_part_k(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                                          double* __restrict__ part) {
  __shared__ double red[256];
  double acc = 0.0;
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) acc += (double)fabsf(a[i] - b[i]);
  acc = mg_block_sum_f64(acc, red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256) swd_absdiff_fin_k(const double* __restrict__ part, int nparts, double count,
                                                         float* __restrict__ out) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[i];
  acc = mg_block_sum_f64(acc, red);
  if (threadIdx.x == 0) out[0] = (float)(acc / count);
}

int swd_dist_blocks(long long n) {  // a function of n alone: the grouping of the sum, and so its bits, never depend on the machine
  const long long b = (n + 256 * 8 - 1) / (256 * 8);
  return (int)(b < 1 ? 1 : b > DIST_MAX_BLOCKS ? DIST_MAX_BLOCKS : b);
}

}  // namespace

extern "C" int mg_swd_pyr_down(const float* x, float* out, int NC, int H, int W, mg_stream_t stream) {
  MG_CHECK_ARG(x && out && NC > 0, "mg_swd_pyr_down: bad arguments");
  MG_CHECK_ARG(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "mg_swd_pyr_down: even sides >= 4 expected, got %dx%d", H, W);
  const size_t total = (size_t)NC * (H / 2) * (W / 2);
  MG_CHECK_ARG(total < (1ull << 39), "mg_swd_pyr_down: batch too large");
  hipLaunchKernelGGL(swd_down_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, H, W, total);
  MG_CHECK_LAUNCH("mg_swd_pyr_down");
  return MG_OK;
}

extern "C" int mg_swd_pyr_lap(const float* x, const float* coarse, float* out, int NC, int H, int W, mg_stream_t stream) {
  MG_CHECK_ARG(x && coarse && out && NC > 0, "mg_swd_pyr_lap: bad arguments");
  MG_CHECK_ARG(H >= 4 && W >= 4 && H % 2 == 0 && W % 2 == 0, "mg_swd_pyr_lap: even sides >= 4 expected, got %dx%d", H, W);
  const size_t total = (size_t)NC * H * W;
  MG_CHECK_ARG(total < (1ull << 39), "mg_swd_pyr_lap: batch too large");
  hipLaunchKernelGGL(swd_lap_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, coarse, out, H, W, total);
  MG_CHECK_LAUNCH("mg_swd_pyr_lap");
  return MG_OK;
}

extern "C" int mg_swd_gather(const float* level, const int32_t* centres, float* desc, double* stats, int N, int C, int H, int W, int P,
                             int patch, int64_t row0, int64_t rows_total, mg_stream_t stream) {
  MG_CHECK_ARG(level && centres && desc && stats && N > 0 && C > 0 && P > 0, "mg_swd_gather: bad arguments");
  MG_CHECK_ARG(patch >= 1 && (patch & 1) && patch <= H && patch <= W, "mg_swd_gather: odd patch size <= %dx%d expected, got %d", H, W,
               patch);
  MG_CHECK_ARG(row0 >= 0 && row0 % P == 0 && row0 + (int64_t)N * P <= rows_total,
               "mg_swd_gather: rows %lld .. %lld do not fit a buffer of %lld rows (row offset: a multiple of %d)", (long long)row0,
               (long long)(row0 + (int64_t)N * P), (long long)rows_total, P);
  MG_CHECK_ARG((int64_t)P * patch * patch < (1ll << 30), "mg_swd_gather: too many patches per image");
  hipLaunchKernelGGL(swd_gather_k, dim3(N), dim3(256), 0, (hipStream_t)stream, level, centres, desc, stats, C, H, W, P, patch,
                     (size_t)row0);
  MG_CHECK_LAUNCH("mg_swd_gather");
  return MG_OK;
}

extern "C" int mg_swd_stats_finish(const double* stats, float* norm, int64_t images, int C, int64_t per_image, mg_stream_t stream) {
  MG_CHECK_ARG(stats && norm && images > 0 && C > 0 && per_image > 0, "mg_swd_stats_finish: bad arguments");
  hipLaunchKernelGGL(swd_stats_finish_k, dim3(C), dim3(256), 0, (hipStream_t)stream, stats, norm, (long long)images, C,
                     (double)images * (double)per_image);
  MG_CHECK_LAUNCH("mg_swd_stats_finish");
  return MG_OK;
}

extern "C" int mg_swd_project(const float* desc, const float* norm, const float* dirs, float* out, int64_t M, int C, int patch, int D,
                              mg_stream_t stream) {
  MG_CHECK_ARG(desc && norm && dirs && out && M > 0 && C > 0 && patch > 0 && D > 0, "mg_swd_project: bad arguments");
  const int K = C * patch * patch;
  const size_t lds = ((size_t)(PJ_DT + PJ_BM + 2) * K) * sizeof(float);
  MG_CHECK_ARG(lds <= 160 * 1024, "mg_swd_project: descriptors of %d numbers need more than 160 KB of LDS", K);
  const int64_t tiles = (M + PJ_BM - 1) / PJ_BM;
  MG_CHECK_ARG(tiles < (1ll << 31), "mg_swd_project: too many descriptors");
  static MgPerDevice once;
  if (mg_first_use_on_device(once))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&swd_project_k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  const int per_cu = lds <= 80 * 1024 ? 2 : 1;
  const int64_t cap = (int64_t)mg_cu_count() * per_cu;  // a workgroup keeps its directions in LDS over all the tiles it takes
  hipLaunchKernelGGL(swd_project_k, dim3((unsigned)(tiles < cap ? tiles : cap), (unsigned)((D + PJ_DT - 1) / PJ_DT)), dim3(256), lds,
                     (hipStream_t)stream, desc, norm, dirs, out, (long long)M, K, patch * patch, D, (int)tiles);
  MG_CHECK_LAUNCH("mg_swd_project");
  return MG_OK;
}

extern "C" int mg_swd_sort_segments(float* x, int S, int64_t M, mg_stream_t stream) {
  MG_CHECK_ARG(x && S > 0 && M > 0, "mg_swd_sort_segments: bad arguments");
  MG_CHECK_ARG(S <= 65535 && M <= (1ll << 30), "mg_swd_sort_segments: at most 65535 segments of 2^30 keys");
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((M + SB - 1) / SB);
  const int nlog = M >= SB ? SB_LOG : (mg_ilog2((int)M) < 1 ? 1 : mg_ilog2((int)M));
  hipLaunchKernelGGL(swd_sort_tile_k, dim3(tiles, S), dim3(ST), 0, s, x, (long long)M, nlog, 1);
  for (int k = SB_LOG + 1; (1ll << (k - 1)) < M; ++k) {
    const long long npairs = (((long long)M + (1ll << k) - 1) >> k) << (k - 1);  // pairs of the padded length
    const dim3 grid((unsigned)((npairs + 255) / 256), S);
    hipLaunchKernelGGL(swd_sort_global_k, grid, dim3(256), 0, s, x, (long long)M, npairs, k, 0ll, 1);
    for (long long j = 1ll << (k - 2); j >= SB; j >>= 1)
      hipLaunchKernelGGL(swd_sort_global_k, grid, dim3(256), 0, s, x, (long long)M, npairs, k, j, 0);
    hipLaunchKernelGGL(swd_sort_tile_k, dim3(tiles, S), dim3(ST), 0, s, x, (long long)M, SB_LOG, 0);
  }
  MG_CHECK_LAUNCH("mg_swd_sort_segments");
  return MG_OK;
}

extern "C" size_t mg_swd_distance_ws_bytes(int64_t n) { return (size_t)swd_dist_blocks(n) * sizeof(double); }

extern "C" int mg_swd_distance(const float* a, const float* b, int64_t n, float* out, void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(a && b && out && ws && n > 0, "mg_swd_distance: bad arguments");
  if (ws_bytes < mg_swd_distance_ws_bytes(n)) {
    mg_set_error("mg_swd_distance: workspace too small");
    return MG_EWORKSPACE;
  }
  const int blocks = swd_dist_blocks(n);
  double* part = reinterpret_cast<double*>(ws);
  hipLaunchKernelGGL(swd_absdiff_part_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a, b, (long long)n, part);
  hipLaunchKernelGGL(swd_absdiff_fin_k, dim3(1), dim3(256), 0, (hipStream_t)stream, part, blocks, (double)n, out);
  MG_CHECK_LAUNCH("mg_swd_distance");
  return MG_OK;
}
