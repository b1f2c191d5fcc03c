// Harmonic / percussive separation by median filtering (Fitzgerald 2010, with librosa's soft masks and margins) of a spectrum
// X (512, T) of the 1024 / 256 STFT, and the overlap-add re-timing that the transient-preserving time stretch (Driedger, Mueller,
// Ewert 2014) gives the percussive part.  Definitions: DESIGN.md, "Harmonic / percussive separation".
//
//   S = |X| in float32 with torch's bits (sleef_f32.h),
//   H[k, t] = median S[k, t - (Lh-1)/2 .. t + (Lh-1)/2],   P[k, t] = median S[k - (Lp-1)/2 .. k + (Lp-1)/2, t],
//   indices past an end reflected as scipy.ndimage's mode='reflect' does (hpss_select.h),
//   Mh = softmask(H, mh P),  Mp = softmask(P, mp H),  harmonic = X Mh,  percussive = X Mp.
//
// mg_hpss is ONE launch: a workgroup = a 64 x 64 tile of output bins, 256 threads, 16 bins per thread with lanes along time.  The
// magnitudes that the tile's windows cover are staged once in LDS as a cross: the tile's 64 rows with (Lh-1)/2 frames on either side
// [64][64 + Lh - 1], and its 64 frames with (Lp-1)/2 rows on either side [64 + Lp - 1][64] (the centre is computed once and stored in
// both); at most 2 x 64 x 126 floats and the reflected index tables = 65 520 bytes.  X is read once per bin plus the halo, every
// output is written once.  A median is a selection among the staged bit patterns (non-negative floats order as unsigned integers),
// so it carries no rounding, and an output bin depends on its own windows alone: the same bits in every run and for every tiling.
// A window is held in registers and its middle key selected by a comparator network with literal indices (hpss_select.h: no scratch
// memory): 32 inputs for lengths up to 31, 64 beyond, shorter windows padded with as many smallest as largest keys; Lh = Lp = 31, the
// default, has an instantiation of its own without the padding.  No atomics, no workspace, no synchronisation: capturable.
//
// mg_ola_stretch is a gather: two reads and two window products per output sample, nothing accumulated across threads.
#include "mg_common.h"
#include "sleef_f32.h"
#include "hpss_select.h"

#include <cmath>
#include <cstdint>

namespace {

constexpr int NB = 512;     // frequency rows
constexpr int TILE = 64;    // output rows and frames per workgroup (hpss_ops.TILE)
constexpr int MAX_L = 63;   // longest median window
constexpr float TINY = 1.17549435e-38f;   // 2^-126, numpy's float32 `tiny`: librosa's threshold for an empty bin

typedef long long i64;

enum { POWER_ONE = 1, POWER_TWO = 2, POWER_INF = 0 };

__device__ __forceinline__ float softmask(float a, float b, int pmode, bool split) {
  if (pmode == POWER_INF) return a > b ? 1.f : 0.f;
  const float z = fmaxf(a, b);
  if (z < TINY) return split ? 0.5f : 0.f;
  float u = a / z, v = b / z;
  if (pmode == POWER_TWO) {
    u = u * u;
    v = v * v;
  }
  return u / (u + v);
}

// the middle key of p[0], p[STRIDE], .., p[(L-1) STRIDE] through the network of N inputs; FULL: L == N - 1, no padding
template <int N, int STRIDE, bool FULL>
__device__ __forceinline__ uint32_t window_median(const uint32_t* p, int L) {
  uint32_t a[N];
  if constexpr (FULL) {
#pragma unroll
    for (int j = 0; j < N - 1; ++j) a[j] = p[j * STRIDE];
  } else {
    const int pad = (N - 1 - L) / 2;
#pragma unroll
    for (int j = 0; j < N - 1; ++j) {
      const int i = j - pad;   // position in the window
      uint32_t v = i < 0 ? hpss::KEY_MIN : hpss::KEY_MAX;
      if (i >= 0 && i < L) v = p[i * STRIDE];
      a[j] = v;
    }
  }
  return hpss::median<N>(a);
}

// NH, NP: inputs of the two selection networks (window lengths up to NH - 1, NP - 1); L31: both window lengths are 31, known at
// compile time; else lh / lp are what the arguments say
template <int NH, int NP, bool L31>
__global__ void __launch_bounds__(256) hpss_tile(const float2* __restrict__ X, float2* __restrict__ harm, float2* __restrict__ perc,
                                                 float* __restrict__ H, float* __restrict__ P, float* __restrict__ Mh,
                                                 float* __restrict__ Mp, i64 T, int lh_arg, int lp_arg, int pmode, float mh, float mp) {
  extern __shared__ uint32_t lds[];
  const int lh = L31 ? 31 : lh_arg, lp = L31 ? 31 : lp_arg;
  const int hh = (lh - 1) / 2, hp = (lp - 1) / 2;
  const int WH = TILE + lh - 1, WP = TILE + lp - 1;
  uint32_t* Sh = lds;                      // [TILE][WH]: the tile's rows, frames t0 - hh .. t0 + 63 + hh
  uint32_t* Sp = lds + TILE * WH;          // [WP][TILE]: rows k0 - hp .. k0 + 63 + hp, the tile's frames
  int* tcol = reinterpret_cast<int*>(Sp + WP * TILE);   // [WH] reflected frame of every staged column
  int* krow = tcol + WH;                                // [WP] reflected row of every staged row
  const int tid = threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * TILE;
  const int k0 = blockIdx.y * TILE;

  for (int i = tid; i < WH; i += 256) tcol[i] = (int)hpss::reflect(t0 - hh + i, T);
  for (int i = tid; i < WP; i += 256) krow[i] = (int)hpss::reflect((i64)k0 - hp + i, NB);
  __syncthreads();

  for (int e = tid; e < TILE * WH; e += 256) {
    const int r = e / WH, c = e - r * WH;
    const float2 z = X[(size_t)(k0 + r) * (size_t)T + (size_t)tcol[c]];
    const uint32_t m = __builtin_bit_cast(uint32_t, slf::hypotf_u05(z.x, z.y));
    Sh[e] = m;
    if (c >= hh && c < hh + TILE) Sp[(hp + r) * TILE + (c - hh)] = m;
  }
  for (int e = tid; e < (lp - 1) * TILE; e += 256) {
    const int rr = e >> 6, c = e & 63;
    const int r = rr < hp ? rr : rr + TILE;
    const float2 z = X[(size_t)krow[r] * (size_t)T + (size_t)tcol[hh + c]];
    Sp[r * TILE + c] = __builtin_bit_cast(uint32_t, slf::hypotf_u05(z.x, z.y));
  }
  __syncthreads();

  const int t = tid & 63;
  const i64 gt = t0 + t;
  if (gt >= T) return;
  const bool split = mh == 1.f && mp == 1.f;
  for (int i = 0; i < TILE / 4; ++i) {
    const int k = (tid >> 6) + 4 * i;
    uint32_t hm, pm;
    hm = window_median<NH, 1, L31>(Sh + k * WH + t, lh);
    pm = window_median<NP, TILE, L31>(Sp + k * TILE + t, lp);
    const float hv = __builtin_bit_cast(float, hm), pv = __builtin_bit_cast(float, pm);
    const float m_h = softmask(hv, mh * pv, pmode, split), m_p = softmask(pv, mp * hv, pmode, split);
    const size_t at = (size_t)(k0 + k) * (size_t)T + (size_t)gt;
    const float2 z = X[at];
    if (harm) harm[at] = float2{z.x * m_h, z.y * m_h};
    if (perc) perc[at] = float2{z.x * m_p, z.y * m_p};
    if (H) H[at] = hv;
    if (P) P[at] = pv;
    if (Mh) Mh[at] = m_h;
    if (Mp) Mp[at] = m_p;
  }
}

constexpr int OLA_HOP = 256;      // hop = threads per workgroup: thread j owns the window values w[j] and w[j + 256]
constexpr int OLA_FRAMES = 8;     // output hops per workgroup

// y[256 m + j] = w[j] x[a_m + j] + w[j + 256] x[a_{m-1} + j + 256],  a_m = (256 m p) / q,  a_{-1} = -256,  x = 0 outside [0, L)
__global__ void __launch_bounds__(OLA_HOP) ola_stretch(const float* __restrict__ x, float* __restrict__ y, i64 L, i64 n_out, i64 p,
                                                       i64 q) {
  const int j = threadIdx.x;
  // 1/2 (1 - cos(2 pi i / 512)) in float64, rounded once
  const float w0 = (float)(0.5 * (1.0 - cospi((double)j / 256.0)));
  const float w1 = (float)(0.5 * (1.0 - cospi((double)(j + OLA_HOP) / 256.0)));
  for (int f = 0; f < OLA_FRAMES; ++f) {
    const i64 m = (i64)blockIdx.x * OLA_FRAMES + f;
    const i64 n = m * OLA_HOP + j;
    if (n >= n_out) return;
    const i64 a = (OLA_HOP * m * p) / q;
    const i64 b = m == 0 ? -(i64)OLA_HOP : (OLA_HOP * (m - 1) * p) / q;
    const i64 i0 = a + j, i1 = b + j + OLA_HOP;
    const float x0 = (i0 >= 0 && i0 < L) ? x[i0] : 0.f;
    const float x1 = (i1 >= 0 && i1 < L) ? x[i1] : 0.f;
    y[n] = w0 * x0 + w1 * x1;
  }
}

bool odd_length(int l) { return l >= 3 && l <= MAX_L && (l & 1); }

}  // namespace

extern "C" int mg_hpss(const float* x_c64, float* harm_c64, float* perc_c64, float* H, float* P, float* mask_h, float* mask_p,
                       int64_t frames, int lh, int lp, float power, float margin_h, float margin_p, mg_stream_t stream) {
  MG_CHECK_ARG(x_c64 && (harm_c64 || perc_c64 || H || P || mask_h || mask_p), "mg_hpss: the spectrum and at least one output expected");
  MG_CHECK_ARG(frames >= 1 && frames < ((int64_t)1 << 31) - 2 * TILE, "mg_hpss: 1 .. 2^31 - 129 frames expected, got %lld",
               (long long)frames);
  MG_CHECK_ARG(odd_length(lh) && odd_length(lp), "mg_hpss: odd kernel lengths in [3, %d] expected, got %d and %d", MAX_L, lh, lp);
  MG_CHECK_ARG(power == 1.f || power == 2.f || power == INFINITY, "mg_hpss: power must be 1, 2 or infinity, got %g", (double)power);
  MG_CHECK_ARG(margin_h >= 1.f && margin_p >= 1.f && std::isfinite(margin_h) && std::isfinite(margin_p),
               "mg_hpss: finite margins >= 1 expected, got %g and %g", (double)margin_h, (double)margin_p);
  MG_CHECK_ARG((reinterpret_cast<uintptr_t>(x_c64) | reinterpret_cast<uintptr_t>(harm_c64) | reinterpret_cast<uintptr_t>(perc_c64)) % 8 == 0 &&
               (reinterpret_cast<uintptr_t>(H) | reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(mask_h) |
                reinterpret_cast<uintptr_t>(mask_p)) % 4 == 0,
               "mg_hpss: the spectra must be 8-byte aligned, the float arrays 4-byte aligned");
  const int pmode = power == 1.f ? POWER_ONE : (power == 2.f ? POWER_TWO : POWER_INF);
  const int WH = TILE + lh - 1, WP = TILE + lp - 1;
  const size_t lds_bytes = ((size_t)TILE * WH + (size_t)WP * TILE + WH + WP) * 4;   // <= 65 520
  const dim3 grid((unsigned)((frames + TILE - 1) / TILE), NB / TILE), block(256);
  hipStream_t s = (hipStream_t)stream;
  const float2* X = reinterpret_cast<const float2*>(x_c64);
  float2* oh = reinterpret_cast<float2*>(harm_c64);
  float2* op = reinterpret_cast<float2*>(perc_c64);
#define MG_HPSS_LAUNCH(NH, NP, L31)                                                                                              \
  hipLaunchKernelGGL((hpss_tile<NH, NP, L31>), grid, block, lds_bytes, s, X, oh, op, H, P, mask_h, mask_p, (i64)frames, lh, lp, pmode, \
                     margin_h, margin_p)
  if (lh == 31 && lp == 31) MG_HPSS_LAUNCH(32, 32, true);
  else if (lh <= 31 && lp <= 31) MG_HPSS_LAUNCH(32, 32, false);
  else if (lh <= 31) MG_HPSS_LAUNCH(32, 64, false);
  else if (lp <= 31) MG_HPSS_LAUNCH(64, 32, false);
  else MG_HPSS_LAUNCH(64, 64, false);
#undef MG_HPSS_LAUNCH
  MG_CHECK_LAUNCH("mg_hpss");
  return MG_OK;
}

extern "C" int mg_ola_stretch(const float* x, int64_t length, float* y, int64_t out_length, int p, int q, mg_stream_t stream) {
  MG_CHECK_ARG(x && length >= 1 && out_length >= 0 && (y || out_length == 0), "mg_ola_stretch: bad arguments");
  MG_CHECK_ARG(p >= 1 && q >= 1 && (i64)p <= 8 * (i64)q && (i64)q <= 8 * (i64)p, "mg_ola_stretch: the rate p / q must lie in [1/8, 8], got %d / %d",
               p, q);
  // 256 m p <= out_length p stays inside 64 bits, the grid inside 2^31 workgroups
  MG_CHECK_ARG(length < ((int64_t)1 << 40) && out_length < ((int64_t)1 << 40) &&
               (unsigned __int128)out_length * (unsigned)p < ((unsigned __int128)1 << 62),
               "mg_ola_stretch: lengths below 2^40 samples and out_length * p below 2^62 expected, got %lld and %lld at p = %d",
               (long long)length, (long long)out_length, p);
  if (out_length == 0) return MG_OK;
  const i64 hops = (out_length + OLA_HOP - 1) / OLA_HOP;
  hipLaunchKernelGGL(ola_stretch, dim3((unsigned)((hops + OLA_FRAMES - 1) / OLA_FRAMES)), dim3(OLA_HOP), 0, (hipStream_t)stream, x, y,
                     (i64)length, (i64)out_length, (i64)p, (i64)q);
  MG_CHECK_LAUNCH("mg_ola_stretch");
  return MG_OK;
}
