// Mel power spectrogram of waveforms and pooled log rows of it: the kernels behind mel_ops.mel_power,
// mel_ops.logmel_pool, audio.mel_spectrogram and metrics.WaveLogMel.
//
//   X[k,t]  = the value of mg_stft_1024 (stft.hip): reflect padding by 512, periodic Hann / sqrt(384), k = 0 .. 511
//   p[k,t]  = re re + im im                                             float32, three roundings
//   s[m,t]  = sum over k in [lo[m], hi[m]) of weight[m,k] p[k,t]        float32, ascending k, product and sum rounded apart
//   out[b W + n, m P + j] = (float)(sum of log((double)s[m,t] + floor) over the win / P frames of pool j of window n, / (win / P))
//
// mel_power_k is stft1024_kernel's frame pipeline (stft_frame.h, fft512.h): persistent workgroups of 8 waves, a tile of 16
// consecutive frames of one row, one wave = 2 frames, each left as 512 bins in its own LDS column, the next frame's samples
// requested one frame ahead.  The spectrum stops there: after the tile's barrier thread (m, f) walks band m down column f and the 16
// frames of a band leave as one 64-byte run along t.  A bin's power is taken again by every band that holds it (two, for triangular
// filters): three operations against an LDS read.  Nothing is accumulated across workgroups: no atomics, no workspace.
//
// The band limits arrive as HOST arrays, are checked against 512 on the host and passed to the kernel by value: no LDS or weight
// index that the kernel forms depends on device memory.
#include <cmath>

#include "fft512.h"
#include "mg_common.h"
#include "stft_frame.h"

namespace {

constexpr int FPB = NWAVE * FPW;    // frames per tile
constexpr size_t MEL_LDS = (size_t)(TW_FLOATS + NFFT + FPB * XSTR * 2) * sizeof(float);
constexpr int MS_MAX_BANDS = 256;   // band limits passed by value: 2 KB of kernel arguments
constexpr int MS_BANDS_PER_PASS = 64 * NWAVE / FPB;   // bands the workgroup sums at a time

struct MsBands {
  int lo[MS_MAX_BANDS];
  int hi[MS_MAX_BANDS];
};

__global__ void __launch_bounds__(64 * NWAVE) mel_power_k(const float* __restrict__ wave_, const float* __restrict__ weight,
                                                          const MsBands bands, float* __restrict__ out, long long L,
                                                          long long row_stride, int T, int M, int tiles_per_row, int ntiles) {
  using Src = PcmSrc<0, 1>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  c2* tw = reinterpret_cast<c2*>(smem);                       // tw[k], k < 512
  c2* tw1 = tw + NB;                                           // tw1[r * 8 + k]
  c2* tw2 = tw1 + 64;                                          // tw2[r * 64 + j]
  float* win = smem + TW_FLOATS;                               // Hann / sqrt(sum w^2)
  c2* xbuf = reinterpret_cast<c2*>(win + NFFT);                // [FPB][XSTR] one column per frame of the tile

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int m = tid; m < NFFT; m += 64 * NWAVE) {
    const float c = fft512_fill_tables(tw, tw1, tw2, m);
    win[m] = stft_window_entry(c);
  }
  __syncthreads();

  // frame `slot` of tile `tile` (a tile past the last one reads as zeros); a row that starts at an odd sample takes its interior
  // frames sample by sample
  auto load_frame = [&](int tile, int slot, c2 (&x)[8]) {
    const int b = tile < ntiles ? tile / tiles_per_row : 0;
    const int t = tile < ntiles ? (tile - b * tiles_per_row) * FPB + slot : T;
    const long long off = (long long)b * row_stride;
    stft_load_frame<Src>(wave_ + off, L, T, t, lane, (off & 1) == 0, x);
  };

  c2 xn[8];  // the frame in flight
  load_frame(blockIdx.x, wv * FPW, xn);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / tiles_per_row, t0 = (tile - b * tiles_per_row) * FPB;
#pragma unroll 1
    for (int f = 0; f < FPW; ++f) {
      const int fl = wv * FPW + f;  // frame slot in the tile
      c2* xb = xbuf + fl * XSTR;
      c2 v[8];
      stft_apply_window(xn, win, lane, v);
      // the next frame of this tile is requested now and arrives under this frame's FFT (past the row's end it reads as zeros)
      if (f + 1 < FPW) load_frame(tile, fl + 1, xn);
      fft512_wave(v, xb, tw1, tw2, lane);
      stft_untangle(v, xb, tw, lane);
    }
    __syncthreads();
    // band sums: 16 neighbouring lanes hold the 16 frames of one band (columns 2 slots apart: no bank conflict among them)
    {
      const int f = tid & (FPB - 1), t = t0 + f;
      const c2* col = xbuf + f * XSTR;
      if (t < T) {
        for (int m = tid / FPB; m < M; m += MS_BANDS_PER_PASS) {
          const int lo = bands.lo[m], hi = bands.hi[m];
          const float* wrow = weight + (size_t)m * NB;
          float s = 0.f;
          for (int k = lo; k < hi; ++k) {
            const c2 z = col[k];
            const float rr = z.x * z.x, ii = z.y * z.y;
            const float p = rr + ii;
            const float wp = wrow[k] * p;
            s = s + wp;
          }
          out[((size_t)b * M + m) * (size_t)T + t] = s;
        }
      }
    }
    // The first frame of the workgroup's next tile is requested here, not under the last FFT: 16 registers that are not live
    // across the band sums are what lets two workgroups share a CU (126 registers against 144), and the other workgroup's FFTs
    // cover the latency that this one then waits for.
    load_frame(tile + (int)gridDim.x, wv * FPW, xn);
    __syncthreads();
  }
}

// one thread per number of out: a chain of win / P float64 additions in ascending t, fixed by the shape alone
__global__ void __launch_bounds__(256) logmel_pool_k(const float* __restrict__ power, float* __restrict__ out, long long total, int M,
                                                     int T, int W, int hop, int P, int pw, double floor_) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % P);
  const long long r = i / P;
  const int m = (int)(r % M);
  const long long bn = r / M;   // b W + n
  const int n = (int)(bn % W);
  const long long b = bn / W;
  const float* p = power + ((size_t)b * M + m) * (size_t)T + (size_t)n * hop + (size_t)j * pw;
  double a = log((double)p[0] + floor_);
  for (int t = 1; t < pw; ++t) a += log((double)p[t] + floor_);
  out[i] = (float)(a / (double)pw);
}

}  // namespace

extern "C" int mg_mel_power(const float* wave, int64_t rows, int64_t length, int64_t row_stride, const float* weight, const int32_t* lo,
                            const int32_t* hi, int bands, float* out, mg_stream_t stream) {
  MG_CHECK_ARG(wave && weight && lo && hi && out, "mg_mel_power: bad arguments");
  MG_CHECK_ARG(rows >= 1 && row_stride >= length, "mg_mel_power: rows >= 1 and row_stride >= length expected, got %lld and %lld < %lld",
               (long long)rows, (long long)row_stride, (long long)length);
  MG_CHECK_ARG(length > NFFT / 2, "mg_mel_power: reflect padding needs length > 512 (got %lld)", (long long)length);
  MG_CHECK_ARG(length / HOP + 1 < (1ll << 30), "mg_mel_power: too many frames");
  MG_CHECK_ARG(bands >= 1 && bands <= MS_MAX_BANDS, "mg_mel_power: bands in 1 .. %d expected, got %d", MS_MAX_BANDS, bands);
  MsBands b;
  for (int m = 0; m < MS_MAX_BANDS; ++m) {
    b.lo[m] = m < bands ? lo[m] : 0;
    b.hi[m] = m < bands ? hi[m] : 0;
    MG_CHECK_ARG(0 <= b.lo[m] && b.lo[m] <= b.hi[m] && b.hi[m] <= NB, "mg_mel_power: band %d: 0 <= lo <= hi <= %d expected, got %d, %d", m,
                 NB, b.lo[m], b.hi[m]);
  }
  const int T = (int)(length / HOP) + 1;
  const long long tiles_per_row = (T + FPB - 1) / FPB;
  MG_CHECK_ARG(rows * tiles_per_row < (1ll << 30), "mg_mel_power: %lld rows of %d frames are more than one launch takes", (long long)rows,
               T);
  const int ntiles = (int)(rows * tiles_per_row);
  const int n_cu = mg_cu_count();
  static MgPerDevice once;
  if (mg_first_use_on_device(once))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mel_power_k), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  // persistent over the tiles: as many workgroups as are resident at once (78 KB of LDS allow two per CU, the registers decide)
  int per_cu = 1;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&mel_power_k), 64 * NWAVE, MEL_LDS) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  if (per_cu > 2) per_cu = 2;
  const int blocks = ntiles < per_cu * n_cu ? ntiles : per_cu * n_cu;
  hipLaunchKernelGGL(mel_power_k, dim3(blocks), dim3(64 * NWAVE), MEL_LDS, (hipStream_t)stream, wave, weight, b, out, (long long)length,
                     (long long)row_stride, T, bands, (int)tiles_per_row, ntiles);
  MG_CHECK_LAUNCH("mg_mel_power");
  return MG_OK;
}

extern "C" int mg_logmel_pool(const float* power, int64_t rows, int bands, int64_t frames, int win, int hop, int pools, double floor,
                              float* out, mg_stream_t stream) {
  MG_CHECK_ARG(power && out, "mg_logmel_pool: bad arguments");
  MG_CHECK_ARG(rows >= 1 && bands >= 1 && bands <= MS_MAX_BANDS && frames >= 1 && frames < (1ll << 30),
               "mg_logmel_pool: rows >= 1, bands in 1 .. %d and frames in 1 .. 2^30 expected, got %lld, %d, %lld", MS_MAX_BANDS,
               (long long)rows, bands, (long long)frames);
  MG_CHECK_ARG(win >= 1 && hop >= 1 && win <= frames, "mg_logmel_pool: windows of 1 .. %lld frames and hop >= 1 expected, got %d, %d",
               (long long)frames, win, hop);
  MG_CHECK_ARG(pools >= 1 && win % pools == 0, "mg_logmel_pool: a pool count that divides win = %d expected, got %d", win, pools);
  MG_CHECK_ARG(floor > 0.0 && std::isfinite(floor), "mg_logmel_pool: a finite floor > 0 expected");
  const long long W = (frames - win) / hop + 1;
  const long long total = rows * W * bands * pools;
  MG_CHECK_ARG(rows * W < (1ll << 31) && total < (1ll << 39), "mg_logmel_pool: %lld windows are more than one launch takes",
               (long long)(rows * W));
  hipLaunchKernelGGL(logmel_pool_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, power, out, total, bands,
                     (int)frames, (int)W, hop, pools, win / pools, floor);
  MG_CHECK_LAUNCH("mg_logmel_pool");
  return MG_OK;
}
