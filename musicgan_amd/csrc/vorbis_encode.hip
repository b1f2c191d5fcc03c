// Ogg Vorbis encoding (Vorbis I specification) on the device: what torchaudio.save writes for a .ogg path (the reference's
// audio/functions.py:139).  The host builds the setup once per channel count (musicgan_amd/audio/vorbis_encode.py: codebooks,
// floor 1, residue 2, coupling) and passes its tables; the header pages are written there too.  This file writes the audio pages.
//
// Long blocks only (n = 2048, hop 1024).  Block k covers input samples [1024 k - 1024, 1024 k + 1024), zero outside [0, N).
// Phases, each a launch on the caller's stream, nothing read back in between (`phases` selects them, for timing):
//   1. analysis (one workgroup per packet and channel): window, fold and DCT-IV through a 512-point complex FFT in LDS (the
//      decoder's IMDCT structure run forwards); the floor posts from the largest |X| around each post (but never more than
//      MASK_DB below the block's largest), S dB below it; the floor
//      curve rendered as the decoder renders it (integer lines over the posts it draws) and q = rint(X / F) against it; posts
//      raised where |q| would pass QMAX.  A channel whose q are all 0 marks its floor unused.  (A first launch finds the first
//      NaN or infinity of float input.)
//   2. count (one workgroup per packet): square-polar coupling of the quantised pair, the class of every partition, the length
//      of every codeword in writing order -> the packet's bytes.
//   3. layout (one workgroup): packet offsets, Ogg lacing segments, page starts (every 255 segments and every 4096 bytes of
//      payload), page offsets; the status.
//   4. pack (one workgroup per packet): the codewords again, an exclusive scan of their lengths, each lane ORs its run of
//      codewords into the packet's 32-bit words (integer atomics only where lanes meet).
//   5. pages (one workgroup per page): header, lacing values, body gathered from the packets, CRC-32 from lane-parallel partial
//      CRCs shifted into place with a GF(2) multiply.
// Every sum has a fixed order and no float atomics are used: the same input gives the same bytes on every run.
#include "fft_radix2.h"
#include "mg_common.h"
#include "ogg_crc.h"

namespace {

constexpr int MAX_CH = 8;
constexpr int N2 = 1024;          // coefficients per block, and the hop
constexpr int FFT_H = 512;        // complex FFT points of the DCT-IV
constexpr int MAX_POSTS = 65;
constexpr int FL_STRIDE = 66;     // int16 per (packet, channel): Y0, Y1, val[2..], used flag at [65]
constexpr int PSIZE = 16;
constexpr int NCLASS = 6;
constexpr int QMAX = 131;
constexpr int CASCADE = 17;
constexpr int MAX_ITER = 24, FORCE_ITER = 16;
constexpr float MASK_GAIN = 0.1f;  // 10^(-MASK_DB / 20), MASK_DB = 20 (audio/vorbis_encode.py)
constexpr int A_THREADS = 256, P_THREADS = 256, L_THREADS = 512, G_THREADS = 256;
constexpr int PAGE_SEGS = 255, PAGE_BYTES = 4096;
constexpr uint32_t SERIAL = 0x4D47414Eu;  // audio/vorbis_encode.py SERIAL

// int32 table (audio/vorbis_encode.py TI_*)
constexpr int TI_BOOK = 0, TI_NPOSTS = 8, TI_NCODES = 9, TI_X = 16, TI_LO = 81, TI_HI = 146, TI_ORD = 211, TI_BIN = 276,
              TI_CODES = 276 + N2;
// float32 table (TF_*)
constexpr int TF_SLOPE = 0, TF_PRE = N2, TF_POST = 2 * N2, TF_FFT = 3 * N2, TF_DB = 3 * N2 + N2 / 2;
enum { B_Y = 0, B_CLS = 1, B_VQ = 2, B_COARSE = 6, B_FINE = 7 };

// status (int64): [0] first non-finite input value (channel * N + sample), [1] first coefficient out of range
// ((packet * channels + channel) * 1024 + bin), -1 none; [2] packet bytes, [3] audio page bytes, [4] pages, [5] page table full,
// [6] a packet longer than max_packet_bytes (-1 none; both are internal errors: nothing written is meaningful)
enum { S_NONFINITE = 0, S_RANGE, S_PAYLOAD, S_TOTAL, S_PAGES, S_OVERFLOW, S_TOOLONG };

__host__ __device__ inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

struct Layout {
  size_t q, fl, pbytes, plog, ppay, pseg, pgseg, pgoff, payload, total;
};

__host__ __device__ inline int64_t packets_of(int64_t n) { return (n + N2 - 1) / N2 + 1; }
__host__ __device__ inline int64_t pay_stride(int64_t maxpk) { return (maxpk + 3) / 4 * 4; }
__host__ __device__ inline int64_t max_segments(int64_t n, int64_t maxpk) { return packets_of(n) * (maxpk / 255 + 1); }
__host__ __device__ inline int64_t max_pages(int64_t n, int64_t maxpk) {
  return max_segments(n, maxpk) / PAGE_SEGS + packets_of(n) * maxpk / PAGE_BYTES + 2;
}

Layout layout(int64_t n, int ch, int64_t maxpk) {
  const int64_t P = packets_of(n), G = max_pages(n, maxpk);
  Layout l;
  l.q = 256;
  l.fl = l.q + al((size_t)P * ch * N2 * 2);
  l.pbytes = l.fl + al((size_t)P * ch * FL_STRIDE * 2);
  l.plog = l.pbytes + al((size_t)P * 4);
  l.ppay = l.plog + al((size_t)(P + 1) * 8);
  l.pseg = l.ppay + al((size_t)(P + 1) * 8);
  l.pgseg = l.pseg + al((size_t)(P + 1) * 8);
  l.pgoff = l.pgseg + al((size_t)(G + 1) * 8);
  l.payload = l.pgoff + al((size_t)(G + 1) * 8);
  l.total = l.payload + al((size_t)P * pay_stride(maxpk));
  return l;
}

struct Ws {
  int64_t* status;
  int16_t* q;
  int16_t* fl;
  int32_t* pbytes;
  int64_t *plog, *ppay, *pseg, *pgseg, *pgoff;
  uint8_t* payload;
};

struct Input {
  const void* x;
  int kind;  // 0 float32, 1 float64, 2 int16
  int64_t stride, n;
  int ch;
};

__device__ __forceinline__ float sample(const Input& in, int c, int64_t i) {
  if (i < 0 || i >= in.n) return 0.f;
  const int64_t o = (int64_t)c * in.stride + i;
  if (in.kind == 0) return static_cast<const float*>(in.x)[o];
  if (in.kind == 1) return (float)static_cast<const double*>(in.x)[o];
  return (float)static_cast<const int16_t*>(in.x)[o] * (1.f / 32768.f);
}

// ------------------------------------------------------------------ 0. status reset, non-finite input
__global__ void __launch_bounds__(64) venc_reset_k(int64_t* __restrict__ status) {
  if (threadIdx.x < 16) status[threadIdx.x] = -1;
}

__global__ void __launch_bounds__(256) venc_check_k(Input in, int64_t* __restrict__ status) {
  const int64_t total = (int64_t)in.ch * in.n;
  for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (int64_t)gridDim.x * 256) {
    const int c = (int)(k / in.n);
    const int64_t i = k - (int64_t)c * in.n;
    const int64_t o = (int64_t)c * in.stride + i;
    const bool ok = in.kind == 0 ? isfinite(static_cast<const float*>(in.x)[o]) : isfinite(static_cast<const double*>(in.x)[o]);
    if (!ok) atomicMin(reinterpret_cast<unsigned long long*>(status + S_NONFINITE), (unsigned long long)k);
  }
}

// ------------------------------------------------------------------ 1. analysis, floor, quantisation
__device__ __forceinline__ float window(const float* slope, int i) { return i < N2 ? slope[i] : slope[2 * N2 - 1 - i]; }

__global__ void __launch_bounds__(A_THREADS) venc_analysis_k(Input in, const int32_t* __restrict__ ti, const float* __restrict__ tf,
                                                             float s_db, Ws ws) {
  __shared__ float u[N2];
  __shared__ float X[N2];
  __shared__ float2 buf[FFT_H];
  __shared__ int imax[MAX_POSTS];
  __shared__ int Y[MAX_POSTS], val[MAX_POSTS], st2[MAX_POSTS], tgt[MAX_POSTS];
  __shared__ int rx[MAX_POSTS + 1], ry[MAX_POSTS + 1];
  __shared__ int nr, viol, nonzero, first_bad;
  const int t = threadIdx.x;
  const int ch = in.ch;
  const int64_t p = blockIdx.x / ch;
  const int c = (int)(blockIdx.x - p * ch);
  const int np = ti[TI_NPOSTS];
  const float* slope = tf + TF_SLOPE;
  const int64_t base = (p - 1) * N2;
  // window and fold: the 2048 windowed samples z folded to the 1024 inputs u of the DCT-IV (the transpose of the decoder's
  // unfold)
  for (int m = t; m < N2; m += A_THREADS) {
    float v;
    if (m < N2 / 2) {
      const int i0 = 3 * N2 / 2 - 1 - m, i1 = 3 * N2 / 2 + m;
      v = -window(slope, i0) * sample(in, c, base + i0) - window(slope, i1) * sample(in, c, base + i1);
    } else {
      const int i0 = m - N2 / 2, i1 = 3 * N2 / 2 - 1 - m;
      v = window(slope, i0) * sample(in, c, base + i0) - window(slope, i1) * sample(in, c, base + i1);
    }
    u[m] = v;
  }
  if (t < MAX_POSTS) imax[t] = 0;
  if (t == 0) viol = 0, nonzero = 0, first_bad = N2;
  __syncthreads();
  // DCT-IV, scaled by 1/512 (= 4 / n)
  dct4_lds(u, X, buf, N2, reinterpret_cast<const float2*>(tf + TF_PRE), reinterpret_cast<const float2*>(tf + TF_POST),
           reinterpret_cast<const float2*>(tf + TF_FFT), 1.f / 512.f, t, A_THREADS);
  __syncthreads();
  // largest |X| between each pair of neighbouring posts (non-negative floats order as their bits)
  for (int b = t; b < N2; b += A_THREADS) atomicMax(&imax[ti[TI_BIN + b]], __float_as_int(fabsf(X[b])));
  __syncthreads();
  const float L0 = logf(1.0649863e-7f), LS = logf(1.0649863f);
  if (t < np) {  // post t's starting Y: S dB below the largest |X| on either side of it
    const int rk = [&] {
      for (int r = 0; r < np; ++r)
        if (ti[TI_ORD + r] == t) return r;
      return 0;
    }();
    float peak = 0.f;  // the block's largest |X| (fixed order)
    for (int r = 0; r < np - 1; ++r) peak = fmaxf(peak, __int_as_float(imax[r]));
    // masking range: a region more than MASK_DB below the block's peak is coded as if it were MASK_DB below it
    const float env = fmaxf(fmaxf(__int_as_float(rk > 0 ? imax[rk - 1] : 0), __int_as_float(rk < np - 1 ? imax[rk] : 0)),
                            peak * MASK_GAIN);
    float y = env > 0.f ? ceilf((logf(env) - s_db * 0.115129255f - L0) / (2.f * LS)) : 0.f;
    y = fminf(fmaxf(y, 0.f), 127.f);  // (a NaN becomes 0 or 127; the input check reports it)
    Y[t] = (int)y;
    tgt[t] = 0;
  }
  __syncthreads();
  const float* db = tf + TF_DB;
  int qv[N2 / A_THREADS];
  for (int it = 0;; ++it) {
    // the decoder's floor 1 synthesis: predicted values, val, and which posts it draws
    if (t < np) st2[t] = t < 2;
    __syncthreads();
    if (t >= 2 && t < np) {
      const int lo = ti[TI_LO + t], hi = ti[TI_HI + t];
      const int x0 = ti[TI_X + lo], x1 = ti[TI_X + hi], y0 = Y[lo], y1 = Y[hi];
      const int dy = y1 - y0, adx = x1 - x0;
      const int off = abs(dy) * (ti[TI_X + t] - x0) / adx;
      const int pred = dy < 0 ? y0 - off : y0 + off;
      const int hiroom = 128 - pred, loroom = pred;
      const int room = 2 * (hiroom < loroom ? hiroom : loroom);
      const int f = Y[t], d = f - pred;
      int v;
      if (d >= 0 && 2 * d < room) v = 2 * d;
      else if (d < 0 && -2 * d - 1 < room) v = -2 * d - 1;
      else v = hiroom > loroom ? f : 127 - f;
      val[t] = v;
      if (v) st2[t] = st2[lo] = st2[hi] = 1;
    }
    __syncthreads();
    if (t == 0) {
      int k = 0;
      for (int r = 0; r < np; ++r) {
        const int i = ti[TI_ORD + r];
        if (st2[i]) rx[k] = ti[TI_X + i], ry[k] = 2 * Y[i], ++k;
      }
      nr = k;
    }
    __syncthreads();
    // the curve at each bin (the decoder's render_line in closed form) and q = rint(X / F)
#pragma unroll
    for (int k = 0; k < N2 / A_THREADS; ++k) {
      const int b = t + k * A_THREADS;
      int lo = 0, hi = nr - 1;  // the last drawn post at or before b
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rx[mid] <= b) lo = mid;
        else hi = mid - 1;
      }
      const int x0 = rx[lo], y0 = ry[lo], x1 = rx[lo + 1], y1 = ry[lo + 1];
      const int dy = y1 - y0, adx = x1 - x0, m = b - x0;
      const int cur = dy < 0 ? y0 - (m * -dy) / adx : y0 + (m * dy) / adx;
      const float F = db[cur];
      const float r = X[b] / F;
      if (!(fabsf(r) < (float)QMAX + 0.5f)) {
        qv[k] = 0;
        float need = ceilf((logf(fabsf(X[b]) / ((float)QMAX + 0.5f)) - L0) / LS) + 1.f;
        need = fminf(fmaxf(need, 0.f), 254.f);  // (NaN: 254)
        const int ty = ((int)need + 1) / 2;
        const int rk = ti[TI_BIN + b];
        atomicMax(&tgt[ti[TI_ORD + rk]], ty);
        atomicMax(&tgt[ti[TI_ORD + rk + 1]], ty);
        viol = 1;
        atomicMin(&first_bad, b);
      } else {
        qv[k] = (int)rintf(r);
      }
    }
    __syncthreads();
    const int v = viol;
    if (v == 0 || it == MAX_ITER) break;
    __syncthreads();
    if (t == 0) viol = 0, first_bad = N2;
    if (t < np) Y[t] = it + 1 >= FORCE_ITER ? 127 : max(Y[t], tgt[t]);
    __syncthreads();
  }
  if (t == 0 && viol)
    atomicMin(reinterpret_cast<unsigned long long*>(ws.status + S_RANGE),
              (unsigned long long)(blockIdx.x * (int64_t)N2 + first_bad));
  int16_t* q = ws.q + (int64_t)blockIdx.x * N2;
  bool any = false;
#pragma unroll
  for (int k = 0; k < N2 / A_THREADS; ++k) {
    q[t + k * A_THREADS] = (int16_t)qv[k];
    any |= qv[k] != 0;
  }
  if (any) nonzero = 1;
  __syncthreads();
  int16_t* fl = ws.fl + (int64_t)blockIdx.x * FL_STRIDE;
  if (t < np) fl[t] = (int16_t)(t < 2 ? Y[t] : val[t]);
  if (t == 0) fl[FL_STRIDE - 1] = (int16_t)nonzero;
}

// ------------------------------------------------------------------ 2 / 4. codewords of a packet in writing order
struct PacketLds {
  int16_t v[MAX_CH * N2];  // the residue vector, channels interleaved (residue 2), pair 0 / 1 coupled
  uint8_t cls[MAX_CH * N2 / PSIZE];
  int16_t fv[MAX_CH][FL_STRIDE];
  int any_used;
  int64_t part[P_THREADS / 64];
};

__device__ __forceinline__ int class_dims(int cl) { return cl == 1 ? 4 : 2; }
__device__ __forceinline__ int class_nval(int cl) { return cl == 1 ? 3 : cl == 2 ? 5 : cl == 3 ? 9 : 17; }

__device__ void load_packet(PacketLds& L, const Ws& ws, int64_t p, int ch) {
  const int t = threadIdx.x;
  for (int k = t; k < ch * N2; k += P_THREADS) {
    const int c = k / N2, i = k - c * N2;
    L.v[i * ch + c] = ws.q[(p * ch + c) * N2 + i];
  }
  for (int k = t; k < ch * FL_STRIDE; k += P_THREADS) L.fv[k / FL_STRIDE][k % FL_STRIDE] = ws.fl[p * ch * FL_STRIDE + k];
  __syncthreads();
  if (ch == 2) {  // square polar: the exact inverse of the decoder's four sign quadrants
    for (int i = t; i < N2; i += P_THREADS) {
      const int l = L.v[2 * i], r = L.v[2 * i + 1];
      int m, a;
      if (abs(l) > abs(r)) m = l, a = l > 0 ? l - r : r - l;
      else m = r, a = r > 0 ? l - r : r - l;
      L.v[2 * i] = (int16_t)m;
      L.v[2 * i + 1] = (int16_t)a;
    }
  }
  if (t == 0) {
    int a = 0;
    for (int c = 0; c < ch; ++c) a |= L.fv[c][FL_STRIDE - 1];
    L.any_used = a;
  }
  __syncthreads();
  const int parts = ch * N2 / PSIZE;
  for (int pt = t; pt < parts; pt += P_THREADS) {
    int mx = 0;
    for (int j = 0; j < PSIZE; ++j) mx = max(mx, abs((int)L.v[pt * PSIZE + j]));
    L.cls[pt] = (uint8_t)(mx == 0 ? 0 : mx <= 1 ? 1 : mx <= 2 ? 2 : mx <= 4 ? 3 : mx <= 8 ? 4 : 5);
  }
  __syncthreads();
}

__device__ __forceinline__ int units_of(int ch, int np) {
  const int parts = ch * N2 / PSIZE;
  return 1 + ch * (np + 1) + parts / 2 * (1 + 2 * PSIZE) + parts * PSIZE;
}

// codeword u of the packet: its bits (first bit to write at bit 0) and length
__device__ __forceinline__ uint32_t unit(const PacketLds& L, const int32_t* __restrict__ ti, int ch, int np, int u, int& len) {
  const int32_t* codes = ti + TI_CODES;
  const int32_t* lens = codes + ti[TI_NCODES];
  if (u == 0) {  // audio packet, mode 1 (long), previous and next windows long
    len = 4;
    return 0xEu;
  }
  const int fu = np + 1;
  if (u < 1 + ch * fu) {
    const int c = (u - 1) / fu, off = (u - 1) - c * fu;
    const bool used = L.fv[c][FL_STRIDE - 1] != 0;
    if (off == 0) {
      len = 1;
      return used ? 1u : 0u;
    }
    if (!used) {
      len = 0;
      return 0u;
    }
    if (off <= 2) {
      len = 7;
      return (uint32_t)L.fv[c][off - 1];
    }
    const int e = ti[TI_BOOK + B_Y] + L.fv[c][off - 1];
    len = lens[e];
    return (uint32_t)codes[e];
  }
  len = 0;
  if (!L.any_used) return 0u;
  const int parts = ch * N2 / PSIZE;
  const int r0 = 1 + ch * fu, r1 = r0 + parts / 2 * (1 + 2 * PSIZE);
  int pt, j, pass;
  if (u < r1) {
    const int g = (u - r0) / (1 + 2 * PSIZE), k = (u - r0) - g * (1 + 2 * PSIZE);
    if (k == 0) {
      const int e = ti[TI_BOOK + B_CLS] + L.cls[2 * g] * NCLASS + L.cls[2 * g + 1];
      len = lens[e];
      return (uint32_t)codes[e];
    }
    pt = 2 * g + (k - 1) / PSIZE;
    j = (k - 1) % PSIZE;
    pass = 0;
  } else {
    pt = (u - r1) / PSIZE;
    j = (u - r1) % PSIZE;
    pass = 1;
  }
  const int cl = L.cls[pt];
  const int16_t* v = L.v + pt * PSIZE;
  int e;
  if (cl == 0) return 0u;
  if (cl == 5) {
    const int x = v[j];
    const int k = (x + (x >= 0 ? CASCADE / 2 : -(CASCADE / 2))) / CASCADE;
    e = pass == 0 ? ti[TI_BOOK + B_COARSE] + k + 15 : ti[TI_BOOK + B_FINE] + (x - k * CASCADE) + CASCADE / 2;
  } else {
    const int d = class_dims(cl), nv = class_nval(cl), h = nv / 2;
    if (pass == 1 || j >= PSIZE / d) return 0u;
    e = 0;
    for (int dd = d - 1; dd >= 0; --dd) e = e * nv + (v[j * d + dd] + h);
    e += ti[TI_BOOK + B_VQ + cl - 1];
  }
  len = lens[e];
  return (uint32_t)codes[e];
}

__device__ int64_t block_sum(int64_t v, int64_t* part) {  // P_THREADS lanes; every lane gets the total
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t tot = 0;
  for (int k = 0; k < P_THREADS / 64; ++k) tot += part[k];
  __syncthreads();
  return tot;
}

__global__ void __launch_bounds__(P_THREADS) venc_count_k(const int32_t* __restrict__ ti, int ch, int64_t maxpk, Ws ws) {
  __shared__ PacketLds L;
  const int64_t p = blockIdx.x;
  const int np = ti[TI_NPOSTS];
  load_packet(L, ws, p, ch);
  const int U = units_of(ch, np);
  const int per = (U + P_THREADS - 1) / P_THREADS;
  const int a = threadIdx.x * per, b = min(a + per, U);
  int64_t bits = 0;
  for (int u = a; u < b; ++u) {
    int len;
    unit(L, ti, ch, np, u, len);
    bits += len;
  }
  const int64_t tot = block_sum(bits, L.part);
  if (threadIdx.x == 0) {
    const int64_t nb = (tot + 7) / 8;
    if (nb > maxpk) ws.status[S_TOOLONG] = p;  // (the packer then writes nothing for it)
    ws.pbytes[p] = (int32_t)(nb < maxpk ? nb : maxpk);
  }
}

__global__ void __launch_bounds__(P_THREADS) venc_pack_k(const int32_t* __restrict__ ti, int ch, Ws ws) {
  __shared__ PacketLds L;
  __shared__ int64_t pre[P_THREADS];
  __shared__ int64_t total;
  const int64_t p = blockIdx.x;
  const int t = threadIdx.x;
  const int np = ti[TI_NPOSTS];
  uint32_t* words = reinterpret_cast<uint32_t*>(ws.payload + ws.ppay[p]);
  const int nw = (ws.pbytes[p] + 3) / 4;
  for (int k = t; k < nw; k += P_THREADS) words[k] = 0u;
  load_packet(L, ws, p, ch);  // (its barriers also order the zeroing before the ORs below)
  const int U = units_of(ch, np);
  const int per = (U + P_THREADS - 1) / P_THREADS;
  const int a = t * per, b = min(a + per, U);
  int64_t bits = 0;
  for (int u = a; u < b; ++u) {
    int len;
    unit(L, ti, ch, np, u, len);
    bits += len;
  }
  pre[t] = bits;
  __syncthreads();
  if (t == 0) {  // exclusive scan of the lanes' bit counts (fixed order)
    int64_t s = 0;
    for (int k = 0; k < P_THREADS; ++k) {
      const int64_t v = pre[k];
      pre[k] = s;
      s += v;
    }
    total = s;
  }
  __syncthreads();
  if ((total + 7) / 8 > ws.pbytes[p]) return;  // longer than the bound (status[6] is set)
  int64_t pos = pre[t];
  int64_t word = pos >> 5;
  int fill = (int)(pos & 31);
  uint64_t acc = 0;
  for (int u = a; u < b; ++u) {
    int len;
    const uint32_t code = unit(L, ti, ch, np, u, len);
    if (!len) continue;
    acc |= (uint64_t)code << fill;
    fill += len;
    if (fill >= 32) {
      atomicOr(words + word, (uint32_t)acc);
      acc >>= 32;
      fill -= 32;
      ++word;
    }
  }
  if (fill > 0) atomicOr(words + word, (uint32_t)acc);
}

// ------------------------------------------------------------------ 3. layout (one workgroup)
__device__ int64_t scan_excl(int64_t v, int64_t* sh, int64_t& total) {  // L_THREADS lanes, fixed order
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  int64_t x = v;
  for (int s = 1; s < 64; s <<= 1) {
    const int64_t y = __shfl_up(x, s, 64);
    if (lane >= s) x += y;
  }
  if (lane == 63) sh[wv] = x;
  __syncthreads();
  int64_t before = 0, tot = 0;
  for (int k = 0; k < L_THREADS / 64; ++k) {
    if (k < wv) before += sh[k];
    tot += sh[k];
  }
  __syncthreads();
  total = tot;
  return before + x - v;
}

__device__ __forceinline__ int64_t packet_of_seg(const int64_t* pseg, int64_t P, int64_t s) {  // the last p with pseg[p] <= s
  int64_t lo = 0, hi = P - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pseg[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ int64_t seg_start(const Ws& ws, int64_t P, int64_t s) {  // payload byte where segment s starts
  if (s >= ws.pseg[P]) return ws.plog[P];
  const int64_t pk = packet_of_seg(ws.pseg, P, s);
  return ws.plog[pk] + 255 * (s - ws.pseg[pk]);
}

__global__ void __launch_bounds__(L_THREADS) venc_layout_k(Ws ws, int64_t P, int64_t max_pg) {
  __shared__ int64_t sh[L_THREADS / 64];
  const int t = threadIdx.x;
  int64_t clog = 0, cpay = 0, cseg = 0;
  for (int64_t b = 0; b < P; b += L_THREADS) {
    const int64_t p = b + t;
    const int64_t n = p < P ? ws.pbytes[p] : 0;
    int64_t t0, t1, t2;
    const int64_t e0 = scan_excl(n, sh, t0);
    const int64_t e1 = scan_excl((n + 3) / 4 * 4, sh, t1);
    const int64_t e2 = scan_excl(p < P ? n / 255 + 1 : 0, sh, t2);
    if (p < P) ws.plog[p] = clog + e0, ws.ppay[p] = cpay + e1, ws.pseg[p] = cseg + e2;
    clog += t0, cpay += t1, cseg += t2;
  }
  if (t == 0) ws.plog[P] = clog, ws.ppay[P] = cpay, ws.pseg[P] = cseg;
  __syncthreads();
  const int64_t S = cseg;
  int64_t npg = 0;
  for (int64_t b = 0; b < S; b += L_THREADS) {
    const int64_t s = b + t;
    int f = 0;
    if (s < S) f = s == 0 || s % PAGE_SEGS == 0 || seg_start(ws, P, s) / PAGE_BYTES != seg_start(ws, P, s - 1) / PAGE_BYTES;
    int64_t tot;
    const int64_t e = scan_excl(f, sh, tot);
    if (f && npg + e < max_pg) ws.pgseg[npg + e] = s;
    npg += tot;
  }
  const int overflow = npg > max_pg;
  if (overflow) npg = max_pg;
  if (t == 0) ws.pgseg[npg] = S;
  __syncthreads();
  int64_t off = 0;
  for (int64_t b = 0; b < npg; b += L_THREADS) {
    const int64_t j = b + t;
    int64_t size = 0;
    if (j < npg) {
      const int64_t s0 = ws.pgseg[j], s1 = ws.pgseg[j + 1];
      size = 27 + (s1 - s0) + seg_start(ws, P, s1) - seg_start(ws, P, s0);
    }
    int64_t tot;
    const int64_t e = scan_excl(size, sh, tot);
    if (j < npg) ws.pgoff[j] = off + e;
    off += tot;
  }
  if (t == 0) {
    ws.pgoff[npg] = off;
    ws.status[S_PAYLOAD] = clog;
    ws.status[S_TOTAL] = off;
    ws.status[S_PAGES] = npg;
    ws.status[S_OVERFLOW] = overflow;
  }
}

// ------------------------------------------------------------------ 5. pages
__global__ void __launch_bounds__(G_THREADS) venc_pages_k(Ws ws, int64_t P, int64_t n, int first_seq, uint8_t* __restrict__ out) {
  __shared__ uint32_t T[256];
  __shared__ uint32_t part[G_THREADS / 64];
  const int64_t j = blockIdx.x;
  const int64_t npg = ws.status[S_PAGES];
  if (j >= npg) return;
  const int t = threadIdx.x;
  const int64_t s0 = ws.pgseg[j], s1 = ws.pgseg[j + 1], ns = s1 - s0;
  const int64_t b0 = seg_start(ws, P, s0), b1 = seg_start(ws, P, s1);
  uint8_t* o = out + ws.pgoff[j];
  const int64_t pk0 = packet_of_seg(ws.pseg, P, s0), pk1 = packet_of_seg(ws.pseg, P, s1 - 1);
  if (t == 0) {
    int64_t gran = -1;  // the end of the last packet completed on the page
    if (s1 - 1 == ws.pseg[pk1 + 1] - 1) gran = pk1;
    else if (ws.pseg[pk1] > s0) gran = pk1 - 1;
    if (gran >= 0) gran = gran * N2 < n ? gran * N2 : n;
    const int flags = (ws.pseg[pk0] != s0 ? 1 : 0) | (j == npg - 1 ? 4 : 0);
    const uint8_t h[27] = {'O', 'g', 'g', 'S', 0, (uint8_t)flags, (uint8_t)gran, (uint8_t)(gran >> 8), (uint8_t)(gran >> 16),
                           (uint8_t)(gran >> 24), (uint8_t)(gran >> 32), (uint8_t)(gran >> 40), (uint8_t)(gran >> 48),
                           (uint8_t)(gran >> 56), (uint8_t)SERIAL, (uint8_t)(SERIAL >> 8), (uint8_t)(SERIAL >> 16),
                           (uint8_t)(SERIAL >> 24), (uint8_t)(j + first_seq), (uint8_t)((j + first_seq) >> 8),
                           (uint8_t)((j + first_seq) >> 16), (uint8_t)((j + first_seq) >> 24), 0, 0, 0, 0, (uint8_t)ns};
    for (int k = 0; k < 27; ++k) o[k] = h[k];
  }
  for (int64_t s = s0 + t; s < s1; s += G_THREADS) {
    const int64_t pk = packet_of_seg(ws.pseg, P, s);
    const int64_t rest = ws.pbytes[pk] - 255 * (s - ws.pseg[pk]);
    o[27 + (s - s0)] = (uint8_t)(rest < 255 ? rest : 255);
  }
  for (int64_t b = b0 + t; b < b1; b += G_THREADS) {
    int64_t lo = pk0, hi = pk1;  // the packet holding payload byte b
    while (lo < hi) {
      const int64_t mid = (lo + hi + 1) >> 1;
      if (ws.plog[mid] <= b) lo = mid;
      else hi = mid - 1;
    }
    o[27 + ns + (b - b0)] = ws.payload[ws.ppay[lo] + (b - ws.plog[lo])];
  }
  __threadfence_block();  // the page as the other threads wrote it
  const uint32_t x = ogg::page_crc_block<G_THREADS>(o, 27 + ns + (b1 - b0), t, T, part);
  if (t == 0) {
    o[22] = (uint8_t)x, o[23] = (uint8_t)(x >> 8), o[24] = (uint8_t)(x >> 16), o[25] = (uint8_t)(x >> 24);
  }
}

}  // namespace

extern "C" size_t mg_vorbis_enc_ws_bytes(int64_t samples, int channels, int64_t max_packet_bytes) {
  if (samples < 1 || channels < 1 || channels > MAX_CH || max_packet_bytes < 1) return 0;
  return layout(samples, channels, max_packet_bytes).total;
}

extern "C" size_t mg_vorbis_enc_max_bytes(int64_t samples, int channels, int64_t max_packet_bytes) {
  if (samples < 1 || channels < 1 || channels > MAX_CH || max_packet_bytes < 1) return 0;
  return (size_t)(packets_of(samples) * max_packet_bytes + max_segments(samples, max_packet_bytes) +
                  27 * max_pages(samples, max_packet_bytes));
}

extern "C" int mg_vorbis_encode(const void* x, int kind, int64_t row_stride, int channels, int64_t samples, float s_db,
                                const int32_t* tables, const float* ftables, int64_t max_packet_bytes, int first_seq, void* ws,
                                size_t ws_bytes, void* out, size_t out_bytes, int phases, mg_stream_t stream) {
  MG_CHECK_ARG(x && tables && ftables && ws && out && samples >= 1, "mg_vorbis_encode: null or empty argument");
  MG_CHECK_ARG(channels >= 1 && channels <= MAX_CH, "mg_vorbis_encode: %d channels (1-%d)", channels, MAX_CH);
  MG_CHECK_ARG(kind >= 0 && kind <= 2, "mg_vorbis_encode: sample kind %d", kind);
  MG_CHECK_ARG(channels == 1 || row_stride >= samples, "mg_vorbis_encode: row stride %lld", (long long)row_stride);
  MG_CHECK_ARG(max_packet_bytes >= 1 && ws_bytes >= mg_vorbis_enc_ws_bytes(samples, channels, max_packet_bytes),
               "mg_vorbis_encode: workspace of %zu bytes too small", ws_bytes);
  MG_CHECK_ARG(out_bytes >= mg_vorbis_enc_max_bytes(samples, channels, max_packet_bytes),
               "mg_vorbis_encode: output of %zu bytes too small", out_bytes);
  const int64_t P = packets_of(samples), G = max_pages(samples, max_packet_bytes);
  MG_CHECK_ARG(P * channels < (1ll << 31) && G < (1ll << 31), "mg_vorbis_encode: input too long");
  const Layout l = layout(samples, channels, max_packet_bytes);
  uint8_t* w = static_cast<uint8_t*>(ws);
  Ws W{reinterpret_cast<int64_t*>(w), reinterpret_cast<int16_t*>(w + l.q), reinterpret_cast<int16_t*>(w + l.fl),
       reinterpret_cast<int32_t*>(w + l.pbytes), reinterpret_cast<int64_t*>(w + l.plog), reinterpret_cast<int64_t*>(w + l.ppay),
       reinterpret_cast<int64_t*>(w + l.pseg), reinterpret_cast<int64_t*>(w + l.pgseg), reinterpret_cast<int64_t*>(w + l.pgoff),
       w + l.payload};
  hipStream_t s = (hipStream_t)stream;
  const Input in{x, kind, channels == 1 ? samples : row_stride, samples, channels};
  if (phases & 1) {
    venc_reset_k<<<1, 64, 0, s>>>(W.status);
    if (kind != 2) {
      const int64_t total = (int64_t)channels * samples;
      const int64_t g = (total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096;
      venc_check_k<<<(unsigned)g, 256, 0, s>>>(in, W.status);
    }
    venc_analysis_k<<<(unsigned)(P * channels), A_THREADS, 0, s>>>(in, tables, ftables, s_db, W);
  }
  if (phases & 2) venc_count_k<<<(unsigned)P, P_THREADS, 0, s>>>(tables, channels, max_packet_bytes, W);
  if (phases & 4) venc_layout_k<<<1, L_THREADS, 0, s>>>(W, P, G);
  if (phases & 8) venc_pack_k<<<(unsigned)P, P_THREADS, 0, s>>>(tables, channels, W);
  if (phases & 16) venc_pages_k<<<(unsigned)G, G_THREADS, 0, s>>>(W, P, samples, first_seq, static_cast<uint8_t*>(out));
  MG_CHECK_LAUNCH("mg_vorbis_encode");
  return MG_OK;
}
