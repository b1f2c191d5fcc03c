// FLAC encoding (RFC 9639) on the device: what torchaudio.save does for a .flac path (the reference's audio/functions.py:139,
// th_audio.save).  The host prepends "fLaC" and STREAMINFO (musicgan_amd/ops.py flac_encode) and hashes the quantised PCM for its
// MD5; everything else -- quantisation, analysis, bit accounting, packing and the CRCs -- runs here.
//
// Pipeline, every step a launch on the caller's stream, nothing read back in between:
//   1. quantise: (channels, samples) float32 / float64 / int16 with a row stride -> planar int32 and the interleaved little-endian
//      PCM for the MD5; non-finite values are counted and the first one's index kept.  A second tiny launch fills the fp64 Tukey
//      window tables.
//   2. analyse (one workgroup of 4 waves per frame): per signal (the channels; for stereo L, R, M, S) wasted bits, CONSTANT, fp64
//      autocorrelation of the windowed block (lags 0..12), Levinson-Durbin in one lane, then every FIXED 0-4 and LPC 1-12
//      candidate: exact integer residuals, per-partition sums, Rice parameters and partition order chosen by estimate, then the
//      exact bit count of that coding.  The cheapest (VERBATIM when nothing beats it) is kept; stereo picks the cheapest channel
//      assignment.  A compact descriptor per frame is written; residuals are not stored.
//   3. offsets (one workgroup): exclusive scan of the frame byte sizes; total and min / max frame size into the status.
//   4. pack (one workgroup per frame): the header with its CRC-8, then one subframe at a time staged in LDS (residuals recomputed,
//      their bit offsets from a workgroup prefix sum, only the stop bit and the k low bits written), flushed to the zeroed output
//      with atomicOr on the two edge words a neighbour may share.
//   5. crc (one wave per frame): the lane-parallel CRC-16 of flac_core.h over the packed frame, written into its last two bytes.
#include "mg_common.h"

#include "flac_core.h"

namespace {

constexpr int BLOCK = 4096;         // fixed block size
constexpr int MAXO = 12;            // highest LPC order tried
constexpr int NT = 256;             // threads of the analyse / pack workgroups
constexpr int PER = BLOCK / NT;     // samples per thread (16)
constexpr int MAXP = 8;             // highest partition order
constexpr int STAGE_WORDS = 3208;   // one subframe: <= 8 + 25 * 4096 bits (VERBATIM of a side channel) + 31 bits of alignment
constexpr int CRC_GRID_MAX = 256 * 16;

// status words (int64) at the start of the workspace
enum { E_TOTAL = 0, E_MIN_FRAME, E_MAX_FRAME, E_NONFINITE, E_FIRST_BAD, E_ERR, E_COUNT = 16 };
enum { T_CONSTANT = 0, T_VERBATIM = 1, T_FIXED = 2, T_LPC = 3 };

struct EncSub {
  int32_t type, order, prec, shift, wasted, porder, method, sbps;  // sbps: bits of the signal before the wasted bits come off
  int32_t cval;
  int32_t coef[MAXO];
  uint32_t bits;                                                   // exact size of the subframe in bits
  uint8_t k[1 << MAXP];                                            // Rice parameter per partition
};

struct EncFrame {
  uint32_t bytes, assign, bs, hbytes;  // assign: the header's channel code (channels - 1, or 8 / 9 / 10)
  EncSub sub[flac::MAX_CH];
};

struct Layout {
  int64_t nframes;
  size_t win, offs, frames, total;
};

Layout layout(int64_t samples) {
  Layout l;
  l.nframes = (samples + BLOCK - 1) / BLOCK;
  l.win = E_COUNT * 8;
  l.offs = l.win + 2 * BLOCK * sizeof(double);
  l.frames = l.offs + ((size_t)(l.nframes + 1) * 8 + 255) / 256 * 256;
  l.total = l.frames + (size_t)l.nframes * sizeof(EncFrame);
  return l;
}

__host__ __device__ inline int rate_code(int rate, int* extra, int* ebits) {
  *extra = 0;
  *ebits = 0;
  switch (rate) {
    case 88200: return 1;
    case 176400: return 2;
    case 192000: return 3;
    case 8000: return 4;
    case 16000: return 5;
    case 22050: return 6;
    case 24000: return 7;
    case 32000: return 8;
    case 44100: return 9;
    case 48000: return 10;
    case 96000: return 11;
    default: break;
  }
  if (rate % 1000 == 0 && rate / 1000 < 256) return *extra = rate / 1000, *ebits = 8, 12;
  if (rate < 65536) return *extra = rate, *ebits = 16, 13;
  if (rate % 10 == 0 && rate / 10 < 65536) return *extra = rate / 10, *ebits = 16, 14;
  return 0;  // from STREAMINFO
}

// frame header bytes (CRC-8 included) into h[16] (LDS in the kernels); returns their count
__device__ inline int build_header(uint8_t* h, int64_t number, int bs, int rate, int bits, int assign) {
  int bcode, bextra = 0, bbits = 0;
  if (bs == 192) bcode = 1;
  else if (bs == 576 || bs == 1152 || bs == 2304 || bs == 4608) bcode = 2 + (bs == 1152) + 2 * (bs == 2304) + 3 * (bs == 4608);
  else if (bs >= 256 && (bs & (bs - 1)) == 0 && bs <= 32768) {
    bcode = 8;
    while ((256 << (bcode - 8)) != bs) ++bcode;
  } else if (bs <= 256) bcode = 6, bextra = bs - 1, bbits = 8;
  else bcode = 7, bextra = bs - 1, bbits = 16;
  int rextra, rbits;
  const int rcode = rate_code(rate, &rextra, &rbits);
  const int scode = bits == 16 ? 4 : 6;
  int n = 0;
  h[n++] = 0xFF;
  h[n++] = 0xF8;  // fixed blocking
  h[n++] = (uint8_t)(bcode << 4 | rcode);
  h[n++] = (uint8_t)(assign << 4 | scode << 1);
  const uint32_t v = (uint32_t)number;  // frame numbers stay below 2^31 (36-bit sample counts / 4096)
  if (v < 0x80) h[n++] = (uint8_t)v;
  else {
    int extra = v < (1u << 11) ? 1 : v < (1u << 16) ? 2 : v < (1u << 21) ? 3 : v < (1u << 26) ? 4 : 5;
    h[n++] = (uint8_t)(((0xFF00u >> (extra + 1)) & 0xFF) | (v >> (6 * extra)));
    for (int k = extra - 1; k >= 0; --k) h[n++] = (uint8_t)(0x80 | ((v >> (6 * k)) & 0x3F));
  }
  if (bbits == 16) h[n++] = (uint8_t)(bextra >> 8);
  if (bbits) h[n++] = (uint8_t)bextra;
  if (rbits == 16) h[n++] = (uint8_t)(rextra >> 8);
  if (rbits) h[n++] = (uint8_t)rextra;
  h[n] = flac::crc8(h, n);
  return n + 1;
}

__device__ inline int32_t signal_sample(const int32_t* __restrict__ q, int64_t N, int assign_sig, int64_t pos) {
  // assign_sig: 0..7 a channel; 8 mid; 9 side (stereo)
  if (assign_sig < 8) return q[assign_sig * N + pos];
  const int32_t L = q[pos], R = q[N + pos];
  return assign_sig == 8 ? (L + R) >> 1 : L - R;
}

__device__ __forceinline__ int32_t fixed_coef(int order, int j) {  // (-1)^j C(order, j + 1)
  if (j >= order) return 0;
  int c = 1;
  for (int m = 0; m <= j; ++m) c = c * (order - m) / (m + 1);
  return (j & 1) ? -c : c;
}

__device__ inline uint32_t zigzag(int64_t r) { return r >= 0 ? (uint32_t)(2 * r) : (uint32_t)(-2 * r - 1); }

// residual of sample i: s[i] - ((sum_j c[j] s[i-1-j]) >> shift), exact; 32-bit sums when they cannot overflow (the decoder's rule)
template <int NO, bool WIDE>
__device__ __forceinline__ int64_t residual(const int32_t* s, int i, const int32_t* c, int shift) {
  if (WIDE) {
    int64_t acc = 0;
#pragma unroll
    for (int j = 0; j < NO; ++j) acc += (int64_t)c[j] * s[i - 1 - j];
    return (int64_t)s[i] - (acc >> shift);
  }
  int32_t acc = 0;
#pragma unroll
  for (int j = 0; j < NO; ++j) acc += c[j] * s[i - 1 - j];
  return (int64_t)s[i] - (int64_t)(acc >> shift);
}

__device__ inline bool lpc_wide(int sb, int prec, int order) {
  int lg = 0;
  while ((1 << lg) < order) ++lg;
  return sb + prec + lg > 32;
}

// residual of sample i >= order of a FIXED (type 2) or LPC (type 3) subframe over the signal s (LDS)
__device__ __forceinline__ int64_t any_residual(const int32_t* s, int i, int type, int order, const int32_t* c, int shift, int sb, int prec) {
  if (type == T_FIXED || !lpc_wide(sb, prec, order)) {
    if (order <= 4) return residual<4, false>(s, i, c, shift);
    if (order <= 8) return residual<8, false>(s, i, c, shift);
    return residual<12, false>(s, i, c, shift);
  }
  if (order <= 4) return residual<4, true>(s, i, c, shift);
  if (order <= 8) return residual<8, true>(s, i, c, shift);
  return residual<12, true>(s, i, c, shift);
}

// (k, estimated bits) of a Rice partition of n values summing to S: libFLAC's estimate (k + 1) n + (S >> k) around log2(S / n)
__device__ inline uint32_t pick_k(uint32_t n, uint64_t S, uint32_t* cost) {
  if (n == 0) {
    *cost = 0;
    return 0;
  }
  const float mean = (float)S / (float)n;  // floor(log2(mean)) to within one: the neighbours are tried
  const int k0 = mean >= 1.0f ? (int)floorf(log2f(mean)) : 0;
  uint32_t bestk = 0;
  uint64_t best = ~0ull;
  for (int k = k0 - 1; k <= k0 + 1; ++k) {
    if (k < 0 || k > 30) continue;
    const uint64_t c = (uint64_t)n * (k + 1) + (S >> k);
    if (c < best) best = c, bestk = (uint32_t)k;
  }
  *cost = best > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)best;
  return bestk;
}

__device__ inline double wave_sumd(double v) {
  for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// ---------------------------------------------------------------- 1. quantise
template <typename T>
__global__ void __launch_bounds__(256) flac_enc_quantise_k(const T* __restrict__ x, int64_t row_stride, int channels, int64_t N,
                                                          int bits, int32_t* __restrict__ q, uint8_t* __restrict__ pcm,
                                                          int64_t* __restrict__ st) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int nb = bits == 16 ? 2 : 3;
  for (int c = 0; c < channels; ++c) {
    const T v = x[c * row_stride + i];
    int32_t s;
    if constexpr (std::is_same<T, int16_t>::value) {
      s = v;
    } else {
      const T scale = (T)(1 << (bits - 1));
      if (!isfinite(v)) {
        atomicAdd(reinterpret_cast<unsigned long long*>(st + E_NONFINITE), 1ull);
        atomicMin(reinterpret_cast<unsigned long long*>(st + E_FIRST_BAD), (unsigned long long)(c * N + i));
        s = 0;
      } else {
        T r = rint(v * scale);  // exact scaling by a power of two, then round half to even
        r = r < -scale ? -scale : r;
        r = r > scale - 1 ? scale - 1 : r;
        s = (int32_t)r;
      }
    }
    q[c * N + i] = s;
    uint8_t* o = pcm + (i * channels + c) * nb;
    o[0] = (uint8_t)s;
    o[1] = (uint8_t)(s >> 8);
    if (nb == 3) o[2] = (uint8_t)(s >> 16);
  }
}

__global__ void flac_enc_init_k(int64_t* __restrict__ st) {
  const int i = threadIdx.x;
  if (i < E_COUNT) st[i] = i == E_FIRST_BAD ? INT64_MAX : 0;
}

// Tukey(0.5) windows: table 0 for a block of 4096, table 1 for the last block's length
__global__ void __launch_bounds__(256) flac_enc_window_k(double* __restrict__ win, int last_bs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * BLOCK) return;
  const int t = i / BLOCK, n = i % BLOCK, N = t ? last_bs : BLOCK;
  double w = 0.0;
  if (n < N) {
    if (N <= 1) w = 1.0;
    else {
      const double a = 0.5, x = (double)n / (N - 1);
      if (x < a / 2) w = 0.5 * (1.0 - cospi(2.0 * x / a));
      else if (x > 1.0 - a / 2) w = 0.5 * (1.0 - cospi(2.0 * (1.0 - x) / a));
      else w = 1.0;
    }
  }
  win[i] = w;
}

// ---------------------------------------------------------------- 2. analyse
constexpr int NCAND = 5 + MAXO;          // FIXED 0-4, LPC 1-MAXO
constexpr int KL = (2 << MAXP) - 1;      // Rice parameters of every partition of every order, heap layout: order p at 2^p - 1

struct AnShared {
  int32_t s[BLOCK + MAXO];               // s[MAXO + i]: sample i of the current signal (wasted bits removed); s[0, MAXO) zero
  uint64_t sums[NCAND][1 << MAXP];       // per candidate: sum of zigzag residuals per finest partition
  uint64_t xbits[NCAND];                 // exact residual bits of the chosen Rice coding
  uint32_t lvl_cost[NCAND][MAXP + 1], lvl_maxk[NCAND][MAXP + 1];  // estimated bits / largest parameter per partition order
  uint8_t kl[NCAND][KL];
  int32_t bp[NCAND], meth[NCAND];        // chosen partition order, Rice method
  double acf[4][MAXO + 1];
  int32_t qc[MAXO + 1][MAXO];            // quantised coefficients of LPC order m (row m)
  int32_t qshift[MAXO + 1];
  int lpc_ok[MAXO + 1];
  double lev_r[MAXO + 1], lev_a[MAXO + 1];  // Levinson-Durbin (one lane)
  uint8_t hdr[16];
  uint32_t red_or, red_diff, ovf;        // ovf: bit c set when candidate c has a residual outside 32 bits
  int best;
  EncSub sig[flac::MAX_CH];
};

// zigzag residuals of samples i0 .. i0 + PER - 1 from the thread's register window xr[m] = sample i0 - MAXO + m (every index a
// constant after unrolling).  MODE 0: 24-bit multiplies (operands within 24 bits, sums within 32), 1: 32-bit, 2: 64-bit sums.
template <int NO, int MODE>
__device__ __forceinline__ void residuals16(const int32_t* xr, int i0, int bs, int order, const int32_t* c, int shift, uint32_t* u,
                                            uint32_t* ovf) {
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int i = i0 + j;
    int64_t r;
    if (MODE == 2) {
      int64_t acc = 0;
#pragma unroll
      for (int m = 0; m < NO; ++m) acc += (int64_t)c[m] * xr[MAXO + j - 1 - m];
      r = (int64_t)xr[MAXO + j] - (acc >> shift);
    } else {
      int32_t acc = 0;
#pragma unroll
      for (int m = 0; m < NO; ++m) acc += MODE == 0 ? __mul24(c[m], xr[MAXO + j - 1 - m]) : c[m] * xr[MAXO + j - 1 - m];
      r = (int64_t)xr[MAXO + j] - (int64_t)(acc >> shift);
    }
    u[j] = 0;
    if (i >= order && i < bs) {
      if (r < INT32_MIN || r > INT32_MAX) *ovf = 1;
      else u[j] = zigzag(r);
    }
  }
}

__device__ __forceinline__ int cand_order(int cand) { return cand < 5 ? cand : cand - 4; }

template <int NO>
__device__ __forceinline__ void residuals_mode(int mode, const int32_t* xr, int i0, int bs, int order, const int32_t* c, int shift,
                                               uint32_t* u, uint32_t* ovf) {
  if (mode == 0) residuals16<NO, 0>(xr, i0, bs, order, c, shift, u, ovf);
  else if (mode == 1) residuals16<NO, 1>(xr, i0, bs, order, c, shift, u, ovf);
  else residuals16<NO, 2>(xr, i0, bs, order, c, shift, u, ovf);
}

// zigzag residuals of this thread's samples [16 t, 16 t + 16) for candidate `cand`
__device__ __forceinline__ void cand_residuals(const AnShared& sh, const int32_t* xr, int cand, int i0, int bs, int sb, int prec,
                                               uint32_t* u, uint32_t* ovf) {
  const int order = cand_order(cand);
  int32_t c[MAXO];
  int shift = 0;
  if (cand < 5) {
    const int32_t f1 = order, f2 = -(order * (order - 1) / 2), f3 = order * (order - 1) * (order - 2) / 6, f4 = order == 4 ? -1 : 0;
    c[0] = f1, c[1] = f2, c[2] = f3, c[3] = f4;
#pragma unroll
    for (int j = 4; j < MAXO; ++j) c[j] = 0;
  } else {
#pragma unroll
    for (int j = 0; j < MAXO; ++j) c[j] = sh.qc[order][j];
    shift = sh.qshift[order];
  }
  const bool narrow = cand < 5 || !lpc_wide(sb, prec, order);
  const int mode = narrow ? (sb <= 24 ? 0 : 1) : 2;  // uniform
  if (order <= 4) residuals_mode<4>(mode, xr, i0, bs, order, c, shift, u, ovf);
  else if (order <= 8) residuals_mode<8>(mode, xr, i0, bs, order, c, shift, u, ovf);
  else residuals_mode<12>(mode, xr, i0, bs, order, c, shift, u, ovf);
}

// Rice parameter and estimated bits of a partition of order p, index j, residual sum S (the partition's residual count follows)
__device__ __forceinline__ void level_part(AnShared& sh, int cand, int p, int j, uint64_t S, int bs, int order, uint32_t* cost,
                                           uint32_t* maxk) {
  uint32_t c;
  const uint32_t k = pick_k((uint32_t)((bs >> p) - (j == 0 ? order : 0)), S, &c);
  sh.kl[cand][(1 << p) - 1 + j] = (uint8_t)k;
  *cost += c;
  *maxk = max(*maxk, k);
}

// one signal of a frame -> sh.sig[slot].  All candidates are carried together, so the workgroup meets a handful of barriers per
// signal: A residual sums (all threads, every candidate), B partition search (one wave per candidate), C partition order per
// candidate, D exact residual bits (all threads), E the cheapest coding.
__device__ __forceinline__ void analyse_signal(AnShared& sh, const int32_t* __restrict__ q, int64_t N, int64_t first, int bs, int sig, int sbps,
                               const double* __restrict__ win, int slot) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int32_t* s = sh.s + MAXO;  // s[-MAXO, 0) reads as 0
  if (t < MAXO) sh.s[t] = 0;
  if (t == 0) sh.red_or = 0, sh.red_diff = 0, sh.ovf = 0;
  for (int k = t; k < NCAND * (1 << MAXP); k += NT) (&sh.sums[0][0])[k] = 0;
  for (int k = t; k < NCAND * (MAXP + 1); k += NT) (&sh.lvl_cost[0][0])[k] = 0, (&sh.lvl_maxk[0][0])[k] = 0;
  if (t < NCAND) sh.xbits[t] = 0;
  __syncthreads();
  uint32_t lor = 0;
  for (int j = 0; j < PER; ++j) {
    const int i = t * PER + j;
    if (i < bs) {
      const int32_t v = signal_sample(q, N, sig, first + i);
      s[i] = v;
      lor |= (uint32_t)v;
    }
  }
  if (lor) atomicOr(&sh.red_or, lor);
  __syncthreads();
  uint32_t ldiff = 0;
  const int32_t s0 = s[0];
  for (int j = 0; j < PER; ++j) {
    const int i = t * PER + j;
    if (i < bs && s[i] != s0) ldiff = 1;
  }
  if (ldiff) atomicOr(&sh.red_diff, 1u);
  __syncthreads();
  EncSub& out = sh.sig[slot];
  if (!sh.red_diff) {  // CONSTANT (uniform branch)
    if (t == 0) {
      out.type = T_CONSTANT, out.order = 0, out.prec = 0, out.shift = 0, out.wasted = 0, out.porder = 0, out.method = 0;
      out.sbps = sbps, out.cval = s0, out.bits = 8 + sbps;
    }
    __syncthreads();
    return;
  }
  const int wasted = min(__builtin_ctz(sh.red_or), sbps - 1);
  const int sb = sbps - wasted;
  if (wasted)
    for (int j = 0; j < PER; ++j) {
      const int i = t * PER + j;
      if (i < bs) s[i] >>= wasted;
    }
  // autocorrelation of the windowed block, lags 0..MAXO, in fp64
  double acc[MAXO + 1];
#pragma unroll
  for (int l = 0; l <= MAXO; ++l) acc[l] = 0.0;
  __syncthreads();
  {
    double xw[MAXO + 1];  // windowed samples i .. i + MAXO, slid along this thread's PER samples
#pragma unroll
    for (int l = 0; l <= MAXO; ++l) {
      const int i = t * PER + l;
      xw[l] = i < bs ? (double)s[i] * win[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
#pragma unroll
      for (int l = 0; l <= MAXO; ++l) acc[l] = fma(xw[0], xw[l], acc[l]);
#pragma unroll
      for (int l = 0; l < MAXO; ++l) xw[l] = xw[l + 1];
      const int i = t * PER + j + MAXO + 1;
      xw[MAXO] = i < bs ? (double)s[i] * win[i] : 0.0;
    }
  }
#pragma unroll
  for (int l = 0; l <= MAXO; ++l) {
    const double v = wave_sumd(acc[l]);
    if (lane == 0) sh.acf[w][l] = v;
  }
  __syncthreads();
  const int prec = sb <= 17 ? 12 : 15;
  if (t == 0) {  // Levinson-Durbin and coefficient quantisation in one lane; R and a in LDS, the inner loops issue their loads together
    double* R = sh.lev_r;
    double* a = sh.lev_a;
#pragma unroll
    for (int l = 0; l <= MAXO; ++l) R[l] = ((sh.acf[0][l] + sh.acf[1][l]) + sh.acf[2][l]) + sh.acf[3][l], a[l] = 0.0;
    double err = R[0];
    const int lim = (1 << (prec - 1)) - 1;
#pragma unroll 1
    for (int m = 1; m <= MAXO; ++m) {
      sh.lpc_ok[m] = 0;
      if (!(m < bs && err > 0.0)) continue;
      double r = R[m];
#pragma unroll
      for (int j = 1; j < MAXO; ++j)
        if (j < m) r -= a[j] * R[m - j];
      const double k = r / err;
      double na[MAXO];
#pragma unroll
      for (int j = 1; j < MAXO; ++j) na[j] = j < m ? a[j] - k * a[m - j] : 0.0;
#pragma unroll
      for (int j = 1; j < MAXO; ++j)
        if (j < m) a[j] = na[j];
      a[m] = k;
      err *= 1.0 - k * k;
      if (!(err == err)) {  // NaN: stop here
        err = -1.0;
        continue;
      }
      double cmax = 0.0;
#pragma unroll
      for (int j = 1; j <= MAXO; ++j)
        if (j <= m) cmax = fmax(cmax, fabs(a[j]));
      int shift = 15;
      while (shift > 0 && cmax * (double)(1 << shift) > (double)lim) --shift;
      double e = 0.0;
#pragma unroll
      for (int j = 0; j < MAXO; ++j) {
        int32_t qv = 0;
        if (j < m) {
          const double v = a[j + 1] * (double)(1 << shift) + e;
          const double r2 = fmin(fmax(rint(v), (double)(-lim - 1)), (double)lim);
          e = v - r2;
          qv = (int32_t)r2;
        }
        sh.qc[m][j] = qv;
      }
      sh.qshift[m] = shift;
      sh.lpc_ok[m] = 1;
    }
  }
  __syncthreads();
  int P = 0;
  while (P < MAXP && (bs & ((2 << P) - 1)) == 0) ++P;
  const int pnP = bs >> P;
  const int i0 = t * PER;
  int32_t xr[MAXO + PER];  // samples i0 - MAXO .. i0 + PER - 1 (entries past the block are never used as residuals or history)
#pragma unroll
  for (int m = 0; m < MAXO + PER; ++m) xr[m] = s[i0 - MAXO + m];
  // A: residual sums per finest partition, every candidate
  for (int cand = 0; cand < NCAND; ++cand) {
    const int order = cand_order(cand);
    if (order >= bs || (cand >= 5 && !sh.lpc_ok[order])) continue;  // uniform
    uint32_t u[PER], ovf = 0;
    cand_residuals(sh, xr, cand, i0, bs, sb, prec, u, &ovf);
    if (ovf) atomicOr(&sh.ovf, 1u << cand);
    if (pnP == PER) {
      uint64_t a = 0;
#pragma unroll
      for (int j = 0; j < PER; ++j) a += u[j];
      sh.sums[cand][t] = a;
    } else if (i0 < bs) {
      uint64_t a = 0;
      int part = i0 / pnP;
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        if (i0 + j < bs) {
          const int pj = (i0 + j) / pnP;
          if (pj != part) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&sh.sums[cand][part]), (unsigned long long)a);
            a = 0;
            part = pj;
          }
          a += u[j];
        }
      }
      atomicAdd(reinterpret_cast<unsigned long long*>(&sh.sums[cand][part]), (unsigned long long)a);
    }
  }
  __syncthreads();
  // B: one wave per candidate; lane l holds finest partitions 4l..4l+3, the coarser orders by pairwise sums and then shuffles
  for (int cand = w; cand < NCAND; cand += 4) {
    const int order = cand_order(cand);
    if (order >= bs || (cand >= 5 && !sh.lpc_ok[order])) continue;  // uniform in the wave
    const int NP = 1 << P;
    uint64_t a4[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) a4[m] = 4 * lane + m < NP ? sh.sums[cand][4 * lane + m] : 0;
    uint32_t cost = 0, mk = 0;
    if ((bs >> P) >= order) {  // order P
#pragma unroll
      for (int m = 0; m < 4; ++m)
        if (4 * lane + m < NP) level_part(sh, cand, P, 4 * lane + m, a4[m], bs, order, &cost, &mk);
      atomicAdd(&sh.lvl_cost[cand][P], cost);
      atomicMax(&sh.lvl_maxk[cand][P], mk);
    }
    const uint64_t b0 = a4[0] + a4[1], b1 = a4[2] + a4[3];
    if (P >= 1 && (bs >> (P - 1)) >= order) {  // order P - 1: partitions 2l, 2l + 1
      cost = 0, mk = 0;
      if (2 * lane < (NP >> 1)) level_part(sh, cand, P - 1, 2 * lane, b0, bs, order, &cost, &mk);
      if (2 * lane + 1 < (NP >> 1)) level_part(sh, cand, P - 1, 2 * lane + 1, b1, bs, order, &cost, &mk);
      atomicAdd(&sh.lvl_cost[cand][P - 1], cost);
      atomicMax(&sh.lvl_maxk[cand][P - 1], mk);
    }
    uint64_t sum = b0 + b1;  // order P - 2: partition l
    for (int p = P - 2; p >= 0; --p) {
      const int d = P - 2 - p;  // lanes per partition: 2^d
      if (d > 0) sum += __shfl_xor(sum, 1 << (d - 1));
      if ((bs >> p) >= order) {
        cost = 0, mk = 0;
        if (lane < (NP >> 2) && (lane & ((1 << d) - 1)) == 0) level_part(sh, cand, p, lane >> d, sum, bs, order, &cost, &mk);
        if (cost) atomicAdd(&sh.lvl_cost[cand][p], cost);
        if (mk) atomicMax(&sh.lvl_maxk[cand][p], mk);
      }
    }
  }
  __syncthreads();
  // C: the partition order of each candidate (one thread each)
  if (t < NCAND) {
    const int order = cand_order(t);
    int bp = 0, meth = 0;
    uint64_t bcost = ~0ull;
    if (order < bs && (t < 5 || sh.lpc_ok[order]))
      for (int p = 0; p <= P; ++p) {
        if ((bs >> p) < order) continue;
        const int mth = sh.lvl_maxk[t][p] >= 15;
        const uint64_t c = (uint64_t)sh.lvl_cost[t][p] + (uint64_t)(1 << p) * (mth ? 5 : 4);
        if (c < bcost) bcost = c, bp = p, meth = mth;
      }
    sh.bp[t] = bp;
    sh.meth[t] = meth;
  }
  __syncthreads();
  // D: exact residual bits of each candidate's chosen coding
  for (int cand = 0; cand < NCAND; ++cand) {
    const int order = cand_order(cand);
    if (order >= bs || (cand >= 5 && !sh.lpc_ok[order])) continue;  // uniform
    uint32_t u[PER], ovf = 0;
    cand_residuals(sh, xr, cand, i0, bs, sb, prec, u, &ovf);
    const int bp = sh.bp[cand];
    const uint8_t* kp = &sh.kl[cand][(1 << bp) - 1];
    uint64_t xb = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int i = i0 + j;
      if (i >= order && i < bs) {
        const uint32_t k = kp[(pnP == PER ? t : i / pnP) >> (P - bp)];
        xb += (u[j] >> k) + k + 1;
      }
    }
    if (xb) atomicAdd(reinterpret_cast<unsigned long long*>(&sh.xbits[cand]), (unsigned long long)xb);
  }
  __syncthreads();
  // E: the cheapest coding, VERBATIM unless something beats it
  if (t == 0) {
    uint64_t best_bits = 8 + wasted + (uint64_t)bs * sb;
    int best = -1;
    for (int cand = 0; cand < NCAND; ++cand) {
      const int order = cand_order(cand);
      if (order >= bs || (cand >= 5 && !sh.lpc_ok[order]) || ((sh.ovf >> cand) & 1)) continue;
      const uint64_t total = 8 + wasted + (uint64_t)order * sb + (cand >= 5 ? 9 + (uint64_t)order * prec : 0) + 6 +
                             (uint64_t)(1 << sh.bp[cand]) * (sh.meth[cand] ? 5 : 4) + sh.xbits[cand];
      if (total < best_bits) best_bits = total, best = cand;
    }
    const int order = best < 0 ? 0 : cand_order(best);
    out.type = best < 0 ? T_VERBATIM : best < 5 ? T_FIXED : T_LPC;
    out.order = order;
    out.prec = best >= 5 ? prec : 0;
    out.shift = best >= 5 ? sh.qshift[order] : 0;
    out.wasted = wasted, out.porder = best < 0 ? 0 : sh.bp[best], out.method = best < 0 ? 0 : sh.meth[best];
    out.sbps = sbps, out.cval = 0, out.bits = (uint32_t)best_bits;
    for (int j = 0; j < MAXO; ++j) out.coef[j] = best >= 5 ? sh.qc[order][j] : (best >= 0 ? fixed_coef(order, j) : 0);
    sh.best = best;
  }
  __syncthreads();
  const int best = sh.best;
  if (best >= 0 && t < (1 << sh.bp[best])) out.k[t] = sh.kl[best][(1 << sh.bp[best]) - 1 + t];
  __syncthreads();
}

__global__ void __launch_bounds__(NT, 2) flac_enc_analyse_k(const int32_t* __restrict__ q, int channels, int64_t N, int bits, int rate,
                                                        const double* __restrict__ win, EncFrame* __restrict__ frames,
                                                        int64_t nframes) {
  __shared__ AnShared sh;
  const int t = threadIdx.x;
  for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
    const int64_t first = f * BLOCK;
    const int bs = (int)min((int64_t)BLOCK, N - first);
    const double* wn = win + (bs == BLOCK ? 0 : BLOCK);
    const bool stereo = channels == 2;
    const int nsig = stereo ? 4 : channels;
    for (int k = 0; k < nsig; ++k) analyse_signal(sh, q, N, first, bs, stereo && k >= 2 ? 8 + (k - 2) : k, bits + (stereo && k == 3), wn, k);
    EncFrame& F = frames[f];
    // channel assignment: independent, left/side, side/right, mid/side (ties: the first)
    int assign = channels - 1, a = 0, b = 1;
    if (stereo) {
      const uint32_t L = sh.sig[0].bits, R = sh.sig[1].bits, M = sh.sig[2].bits, S = sh.sig[3].bits;
      uint32_t best = L + R;
      if (L + S < best) best = L + S, assign = 8, a = 0, b = 3;
      if (S + R < best) best = S + R, assign = 9, a = 3, b = 1;
      if (M + S < best) best = M + S, assign = 10, a = 2, b = 3;
    }
    uint64_t sbits = 0;
    for (int c = 0; c < channels; ++c) {
      const int src = stereo ? (c == 0 ? a : b) : c;
      sbits += sh.sig[src].bits;
      const uint32_t* from = reinterpret_cast<const uint32_t*>(&sh.sig[src]);
      uint32_t* to = reinterpret_cast<uint32_t*>(&F.sub[c]);
      for (int j = t; j < (int)(sizeof(EncSub) / 4); j += NT) to[j] = from[j];
    }
    if (t == 0) {
      const int hb = build_header(sh.hdr, f, bs, rate, bits, assign);
      F.bytes = (uint32_t)((hb * 8 + sbits + 7) / 8 + 2);
      F.assign = (uint32_t)assign;
      F.bs = (uint32_t)bs;
      F.hbytes = (uint32_t)hb;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- 3. offsets
__global__ void __launch_bounds__(1024) flac_enc_offsets_k(const EncFrame* __restrict__ frames, int64_t nframes,
                                                         int64_t* __restrict__ offs, int64_t* __restrict__ st) {
  __shared__ uint64_t s[1024];
  __shared__ uint64_t carry;
  __shared__ uint32_t mn, mx;
  const int t = threadIdx.x;
  if (t == 0) carry = 0, mn = 0xFFFFFFFFu, mx = 0;
  __syncthreads();
  for (int64_t b = 0; b < nframes; b += 1024) {
    const uint32_t v = b + t < nframes ? frames[b + t].bytes : 0;
    if (b + t < nframes) atomicMin(&mn, v), atomicMax(&mx, v);
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const uint64_t a = t >= d ? s[t - d] : 0;
      __syncthreads();
      s[t] += a;
      __syncthreads();
    }
    const uint64_t c0 = carry;
    if (b + t < nframes) offs[b + t] = (int64_t)(c0 + s[t] - v);
    __syncthreads();
    if (t == 0) carry = c0 + s[1023];
    __syncthreads();
  }
  if (t == 0) {
    offs[nframes] = (int64_t)carry;
    st[E_TOTAL] = (int64_t)carry;
    st[E_MIN_FRAME] = nframes ? mn : 0;
    st[E_MAX_FRAME] = mx;
  }
}

// ---------------------------------------------------------------- 4. pack
struct PkShared {
  int32_t s[BLOCK + MAXO];
  uint32_t stage[STAGE_WORDS];
  uint32_t scan[NT];
  uint8_t hdr[16];
  uint32_t err;
};

// n <= 32 bits of v (MSB first) at bit `pos` of the staging words
__device__ inline void put_bits(PkShared& sh, uint32_t pos, uint32_t v, int n) {
  if (n == 0) return;
  const uint32_t j = pos >> 5;
  const int sft = pos & 31;
  if (j + 1 >= STAGE_WORDS) {
    sh.err = 1;
    return;
  }
  v = n == 32 ? v : v & ((1u << n) - 1);
  if (sft + n <= 32) atomicOr(&sh.stage[j], v << (32 - sft - n));
  else {
    atomicOr(&sh.stage[j], v >> (sft + n - 32));
    atomicOr(&sh.stage[j + 1], v << (64 - sft - n));
  }
}

__device__ inline uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xFF00) | ((x << 8) & 0xFF0000) | (x << 24); }

__global__ void __launch_bounds__(NT) flac_enc_pack_k(const int32_t* __restrict__ q, int channels, int64_t N, int bits, int rate,
                                                    const EncFrame* __restrict__ frames, const int64_t* __restrict__ offs,
                                                    int64_t nframes, uint32_t* __restrict__ out, int64_t out_words,
                                                    int64_t* __restrict__ st) {
  __shared__ PkShared sh;
  const int t = threadIdx.x;
  int32_t* s = sh.s + MAXO;
  if (t < MAXO) sh.s[t] = 0;
  if (t == 0) sh.err = 0;
  for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
    const EncFrame& F = frames[f];
    const int bs = (int)F.bs, assign = (int)F.assign;
    const int64_t off = offs[f], first = f * BLOCK;
    if (t == 0) {
      uint8_t* h = sh.hdr;
      const int hb = build_header(h, f, bs, rate, bits, assign);
      if (hb != (int)F.hbytes) sh.err = 1;
      for (int j = 0; j < hb; ++j) {
        const int64_t o = off + j;
        if ((o >> 2) < out_words) atomicOr(&out[o >> 2], (uint32_t)h[j] << (8 * (o & 3)));
      }
    }
    int64_t bitpos = (off + F.hbytes) * 8;
    for (int c = 0; c < channels; ++c) {
      const EncSub& d = F.sub[c];
      const int type = d.type, order = d.order, wasted = d.wasted, sb = d.sbps - wasted, prec = d.prec, shift = d.shift;
      const int p = d.porder, pbits = d.method ? 5 : 4, pn = bs >> p;
      int sig = c;
      if (assign == 8) sig = c == 0 ? 0 : 9;
      else if (assign == 9) sig = c == 0 ? 9 : 1;
      else if (assign == 10) sig = c == 0 ? 8 : 9;
      for (int j = 0; j < PER; ++j) {
        const int i = t * PER + j;
        if (i < bs) s[i] = signal_sample(q, N, sig, first + i) >> wasted;
      }
      for (int j = t; j < STAGE_WORDS; j += NT) sh.stage[j] = 0;
      __syncthreads();
      const uint32_t o = (uint32_t)(bitpos & 31);
      const int tcode = type == T_CONSTANT ? 0 : type == T_VERBATIM ? 1 : type == T_FIXED ? 8 + order : 31 + order;
      const uint32_t hb = 8 + wasted;
      uint32_t end = 0;  // bits written, as counted here
      if (t == 0) {
        put_bits(sh, o, (uint32_t)(tcode << 1 | (wasted > 0)), 8);
        if (wasted) put_bits(sh, o + 8 + wasted - 1, 1, 1);
        if (type == T_CONSTANT) put_bits(sh, o + 8, (uint32_t)d.cval, d.sbps);
      }
      if (type == T_CONSTANT) {
        end = 8 + d.sbps;
      } else if (type == T_VERBATIM) {
        for (int j = 0; j < PER; ++j) {
          const int i = t * PER + j;
          if (i < bs) put_bits(sh, o + hb + (uint32_t)i * sb, (uint32_t)s[i], sb);
        }
        end = hb + (uint32_t)bs * sb;
      } else {
        if (t < order) put_bits(sh, o + hb + (uint32_t)t * sb, (uint32_t)s[t], sb);
        uint32_t rel = hb + (uint32_t)order * sb;
        if (type == T_LPC) {
          if (t == 0) {
            put_bits(sh, o + rel, (uint32_t)(prec - 1), 4);
            put_bits(sh, o + rel + 4, (uint32_t)shift, 5);
          }
          if (t < order) put_bits(sh, o + rel + 9 + (uint32_t)t * prec, (uint32_t)d.coef[t], prec);
          rel += 9 + (uint32_t)order * prec;
        }
        if (t == 0) {
          put_bits(sh, o + rel, (uint32_t)d.method, 2);
          put_bits(sh, o + rel + 2, (uint32_t)p, 4);
        }
        rel += 6;
        int32_t c12[MAXO];
#pragma unroll
        for (int j = 0; j < MAXO; ++j) c12[j] = d.coef[j];
        uint32_t u[PER], len[PER], tot = 0;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int i = t * PER + j;
          u[j] = 0;
          len[j] = 0;
          if (i < bs) {
            if (i % pn == 0) len[j] += pbits;
            if (i >= order) {
              const int64_t r = any_residual(s, i, type, order, c12, shift, sb, prec);
              u[j] = zigzag(r);
              const uint32_t k = d.k[i / pn];
              len[j] += (u[j] >> k) + k + 1;
            }
          }
          tot += len[j];
        }
        // workgroup exclusive prefix of the per-thread totals
        sh.scan[t] = tot;
        __syncthreads();
        for (int dd = 1; dd < NT; dd <<= 1) {
          const uint32_t a = t >= dd ? sh.scan[t - dd] : 0;
          __syncthreads();
          sh.scan[t] += a;
          __syncthreads();
        }
        uint32_t pos = rel + sh.scan[t] - tot;
        end = rel + sh.scan[NT - 1];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int i = t * PER + j;
          if (i < bs) {
            uint32_t at = pos;
            if (i % pn == 0) {
              put_bits(sh, o + at, d.k[i / pn], pbits);
              at += pbits;
            }
            if (i >= order) {
              const uint32_t k = d.k[i / pn];
              const uint32_t qq = u[j] >> k;
              put_bits(sh, o + at + qq, (1u << k) | (u[j] & ((1u << k) - 1)), (int)k + 1);
            }
          }
          pos += len[j];
        }
      }
      if (t == 0 && end != d.bits) sh.err = 1;
      __syncthreads();
      // flush: interior words are this subframe's alone, the two edge words may be shared with a neighbour
      const int64_t W0 = bitpos >> 5;
      const int64_t nw = ((int64_t)o + d.bits + 31) >> 5;
      for (int64_t j = t; j < nw; j += NT) {
        const int64_t gw = W0 + j;
        if (gw >= out_words || j >= STAGE_WORDS) {
          sh.err = 1;
          continue;
        }
        const uint32_t v = bswap32(sh.stage[j]);
        if (j == 0 || j == nw - 1) {
          if (v) atomicOr(&out[gw], v);
        } else {
          out[gw] = v;
        }
      }
      bitpos += d.bits;
      __syncthreads();
    }
    if (t == 0 && (bitpos + 7) / 8 + 2 != offs[f + 1]) sh.err = 1;
  }
  __syncthreads();
  if (t == 0 && sh.err) atomicOr(reinterpret_cast<unsigned long long*>(st + E_ERR), 1ull);
}

// ---------------------------------------------------------------- 5. CRC-16
__global__ void __launch_bounds__(64) flac_enc_crc_k(uint8_t* __restrict__ out, int64_t out_bytes, const int64_t* __restrict__ offs,
                                                   int64_t nframes) {
  __shared__ uint16_t table[256];
  __shared__ uint32_t xpow[65];
  __shared__ uint32_t part[64];
  const int lane = threadIdx.x;
  flac::crc16_setup(table, xpow, lane);
  __syncthreads();
  flac::Job jb = {};
  jb.d = out;
  jb.crc_table = table;
  jb.xpow = xpow;
  for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
    const int64_t start = offs[f], end = offs[f + 1] - 2;
    if (end + 2 > out_bytes || end <= start) continue;  // (the sizes are bounded by construction; never write past the output)
    part[lane] = flac::frame_crc_part(jb, start, end, lane, 64);
    __syncthreads();
    if (lane == 0) {
      uint32_t crc = 0;
      for (int l = 0; l < 64; ++l) crc ^= part[l];
      out[end] = (uint8_t)(crc >> 8);
      out[end + 1] = (uint8_t)crc;
    }
    __syncthreads();
  }
}

int check_args(const char* who, int channels, int64_t samples, int bits) {
  MG_CHECK_ARG(channels >= 1 && channels <= flac::MAX_CH && samples >= 1 && samples < (1ll << 36) && (bits == 16 || bits == 24),
               "%s: bad arguments (channels %d, samples %lld, bits %d)", who, channels, (long long)samples, bits);
  return MG_OK;
}

}  // namespace

extern "C" size_t mg_flac_enc_ws_bytes(int64_t samples, int channels) {
  if (samples < 1 || channels < 1 || channels > flac::MAX_CH) return 0;
  return layout(samples).total;
}

extern "C" size_t mg_flac_enc_max_bytes(int64_t samples, int channels, int bits) {
  if (samples < 0 || channels < 1 || channels > flac::MAX_CH || (bits != 16 && bits != 24)) return 0;
  // "fLaC" + STREAMINFO, then per frame: a header of at most 16 bytes, every subframe no larger than VERBATIM (8 + bs * bits), the
  // byte padding and the CRC-16
  size_t total = 42;
  for (int64_t first = 0; first < samples; first += BLOCK) {
    const int64_t bs = samples - first < BLOCK ? samples - first : BLOCK;
    total += 16 + ((size_t)channels * (8 + (size_t)bs * bits) + 7) / 8 + 2;
  }
  return total;
}

extern "C" int mg_flac_enc_quantise(const void* x, int kind, int64_t row_stride, int channels, int64_t samples, int bits,
                                    int32_t* planar, void* pcm, void* ws, size_t ws_bytes, mg_stream_t stream) {
  const int rc = check_args("mg_flac_enc_quantise", channels, samples, bits);
  if (rc) return rc;
  MG_CHECK_ARG(x && planar && pcm && ws && row_stride >= samples && kind >= 0 && kind <= 2 && (kind != 2 || bits == 16),
               "mg_flac_enc_quantise: bad arguments (kind %d, stride %lld)", kind, (long long)row_stride);
  const Layout l = layout(samples);
  MG_CHECK_ARG(ws_bytes >= l.total, "mg_flac_enc_quantise: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = static_cast<uint8_t*>(ws);
  int64_t* st = reinterpret_cast<int64_t*>(w);
  flac_enc_init_k<<<1, 64, 0, s>>>(st);
  const unsigned grid = (unsigned)((samples + 255) / 256);
  uint8_t* p = static_cast<uint8_t*>(pcm);
  if (kind == 0) flac_enc_quantise_k<float><<<grid, 256, 0, s>>>(static_cast<const float*>(x), row_stride, channels, samples, bits, planar, p, st);
  else if (kind == 1) flac_enc_quantise_k<double><<<grid, 256, 0, s>>>(static_cast<const double*>(x), row_stride, channels, samples, bits, planar, p, st);
  else flac_enc_quantise_k<int16_t><<<grid, 256, 0, s>>>(static_cast<const int16_t*>(x), row_stride, channels, samples, bits, planar, p, st);
  const int64_t last = samples - (l.nframes - 1) * BLOCK;
  flac_enc_window_k<<<2 * BLOCK / 256, 256, 0, s>>>(reinterpret_cast<double*>(w + l.win), (int)last);
  MG_CHECK_LAUNCH("mg_flac_enc_quantise");
  return MG_OK;
}

extern "C" int mg_flac_enc_frames(const int32_t* planar, int channels, int64_t samples, int bits, int sample_rate, void* ws,
                                  size_t ws_bytes, void* out, size_t out_bytes, mg_stream_t stream) {
  const int rc = check_args("mg_flac_enc_frames", channels, samples, bits);
  if (rc) return rc;
  const Layout l = layout(samples);
  MG_CHECK_ARG(planar && ws && out && ((uintptr_t)out & 3) == 0 && sample_rate >= 1 && sample_rate < (1 << 20),
               "mg_flac_enc_frames: bad arguments (rate %d)", sample_rate);
  MG_CHECK_ARG(ws_bytes >= l.total, "mg_flac_enc_frames: workspace of %zu bytes, %zu needed", ws_bytes, l.total);
  MG_CHECK_ARG(out_bytes + 42 >= mg_flac_enc_max_bytes(samples, channels, bits),
               "mg_flac_enc_frames: output of %zu bytes, %zu needed", out_bytes, mg_flac_enc_max_bytes(samples, channels, bits) - 42);
  hipStream_t s = (hipStream_t)stream;
  uint8_t* w = static_cast<uint8_t*>(ws);
  int64_t* st = reinterpret_cast<int64_t*>(w);
  const double* win = reinterpret_cast<const double*>(w + l.win);
  int64_t* offs = reinterpret_cast<int64_t*>(w + l.offs);
  EncFrame* frames = reinterpret_cast<EncFrame*>(w + l.frames);
  const unsigned grid = (unsigned)(l.nframes < (1 << 20) ? l.nframes : (1 << 20));
  flac_enc_analyse_k<<<grid, NT, 0, s>>>(planar, channels, samples, bits, sample_rate, win, frames, l.nframes);
  flac_enc_offsets_k<<<1, 1024, 0, s>>>(frames, l.nframes, offs, st);
  flac_enc_pack_k<<<grid, NT, 0, s>>>(planar, channels, samples, bits, sample_rate, frames, offs, l.nframes,
                                     static_cast<uint32_t*>(out), (int64_t)(out_bytes / 4), st);
  const unsigned cgrid = (unsigned)(l.nframes < CRC_GRID_MAX ? l.nframes : CRC_GRID_MAX);
  flac_enc_crc_k<<<cgrid, 64, 0, s>>>(static_cast<uint8_t*>(out), (int64_t)out_bytes, offs, l.nframes);
  MG_CHECK_LAUNCH("mg_flac_enc_frames");
  return MG_OK;
}
