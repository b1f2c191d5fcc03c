// Phase vocoder for the 1024 / 256 STFT (definition and the mod-2 pi argument: DESIGN.md, "Phase vocoder"): re-time a spectrum
// X (512, T) by the rational rate p / q.  Output frame t reads the input frames i0 = (t p) / q and i0 + 1 (X is zero from frame T on),
//   mag = alpha |X[i0+1]| + (1 - alpha) |X[i0]|,  alpha = ((t p) mod q) / q,
//   dev = wrap(arg X[i0+1] - arg X[i0] - (k mod 4) pi/2),
//   out = mag e^{i theta} i^(k t mod 4),  theta = arg X[k, 0] + sum_{j < t} dev[k, j].
// The advance pi k / 2 per frame is never summed: modulo 2 pi it is a whole number of quarter turns, applied exactly as a swap of
// the real and imaginary parts.  |X| and arg X are float32 with torch's bits (sleef_f32.h); everything between them and the final
// sine / cosine is float64; the sums have a fixed order (no atomics, no workgroup waits for another).
//
// Four launches on the caller's stream:
//   pv_polar      (|X|, arg X) of every input bin that an output frame reads, ONCE, into the workspace (8 B read + 8 B written per
//                 input bin).  The ~130 vector instructions of the SLEEF restatement per bin are what bounds codec_row_pass; the two
//                 passes below both need the angles, so recomputing them there would pay that twice per output bin and pass.
//   pv_tile_sums  a workgroup = one row x TILE output frames, one frame per thread: the float64 sum of the tile's deviations
//   pv_row_scan   a workgroup = one row: exclusive prefix of its tile sums, in place
//   pv_finish     the tiles again: prefix inside the tile + the carried-in prefix, reduction mod 2 pi, sine / cosine, the store
// Lanes run along time in every launch, so loads and stores are contiguous runs of the frequency-major layout.
#include "mg_common.h"
#include "sleef_f32.h"

#include <cstdint>

namespace {

constexpr int NB = 512;     // frequency rows
constexpr int TILE = 256;   // output frames per workgroup = threads per workgroup (pv_ops.TIME_TILE)
constexpr double PI_2 = 1.5707963267948966, TWO_PI = 6.283185307179586, INV_TWO_PI = 0.15915494309189535, TWO_OVER_PI = 0.6366197723675814;

typedef long long i64;

__device__ __forceinline__ double pv_wrap(double x) { return x - TWO_PI * rint(x * INV_TWO_PI); }

// Inclusive prefix sum over the 256 threads of a workgroup in a fixed order: a shuffle scan inside each wave, the wave totals
// through LDS.  Returns this thread's inclusive prefix; `excl` its exclusive one, `total` the sum of all 256.
__device__ __forceinline__ double pv_block_scan(double v, double* red, double& excl, double& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double u = __shfl_up(v, d);
    if (lane >= d) v += u;
  }
  double before = __shfl_up(v, 1);
  if (lane == 0) before = 0.0;
  if (lane == 63) red[wave] = v;
  __syncthreads();
  double off = 0.0;
  for (int w = 0; w < wave; ++w) off += red[w];
  total = ((red[0] + red[1]) + red[2]) + red[3];
  excl = off + before;
  return off + v;
}

// sparse != 0 (p >= 2 q: the pairs (i0, i0 + 1) of different output frames are disjoint): thread = one member of one pair, 2 n in
// all; else thread = one input frame.  Frames that no output frame reads are neither computed nor written.
__global__ void __launch_bounds__(256) pv_polar(const float2* __restrict__ X, float2* __restrict__ P, i64 T, i64 n, i64 p, i64 q,
                                                int sparse) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  i64 i = idx;
  if (sparse) {
    if (idx >= 2 * n) return;
    i = ((idx >> 1) * p) / q + (idx & 1);
  }
  if (i >= T) return;
  const size_t at = (size_t)blockIdx.y * (size_t)T + (size_t)i;
  const float2 z = X[at];
  float m, a;
  slf::abs_angle(z.x, z.y, m, a);
  P[at] = float2{m, a};
}

// what output frame t of row k reads: the magnitudes and the wrapped deviation (0 past the last frame)
__device__ __forceinline__ double pv_bin(const float2* __restrict__ Prow, i64 T, i64 n, i64 p, i64 q, int k, i64 t, float& m0, float& m1,
                                         double& alpha) {
  m0 = m1 = 0.f;
  alpha = 0.0;
  if (t >= n) return 0.0;
  const i64 tp = t * p, i0 = tp / q;  // i0 <= T - 1 for every t < n
  alpha = (double)(tp - i0 * q) / (double)q;
  const float2 a = Prow[i0];
  float2 b = float2{0.f, 0.f};
  if (i0 + 1 < T) b = Prow[i0 + 1];
  m0 = a.x;
  m1 = b.x;
  return pv_wrap(((double)b.y - (double)a.y) - (double)(k & 3) * PI_2);
}

__global__ void __launch_bounds__(256) pv_tile_sums(const float2* __restrict__ P, double* __restrict__ sums, i64 T, i64 n, i64 p, i64 q,
                                                    int ntiles) {
  __shared__ double red[4];
  const int k = blockIdx.y;
  const i64 t = (i64)blockIdx.x * TILE + threadIdx.x;
  float m0, m1;
  double alpha, excl, total;
  const double dev = pv_bin(P + (size_t)k * (size_t)T, T, n, p, q, k, t, m0, m1, alpha);
  pv_block_scan(dev, red, excl, total);
  if (threadIdx.x == 0) sums[(size_t)k * ntiles + blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) pv_row_scan(double* __restrict__ sums, int ntiles) {
  __shared__ double red[4];
  double* row = sums + (size_t)blockIdx.x * ntiles;
  double carry = 0.0;
  for (int c = 0; c < ntiles; c += 256) {
    const int j = c + (int)threadIdx.x;
    double excl, total;
    pv_block_scan(j < ntiles ? row[j] : 0.0, red, excl, total);
    if (j < ntiles) row[j] = carry + excl;
    carry += total;
    __syncthreads();  // `red` is written again by the next chunk
  }
}

// sine and cosine of |x| <= pi in float64: quadrant j = rint(2 x / pi), r = x - j pi/2 with pi/2 in two parts, then the polynomials of
// fdlibm's __kernel_sin / __kernel_cos on |r| <= pi/4 (Sun Microsystems, freely distributable; errors below 1 ulp)
__device__ __forceinline__ void pv_sincos(double x, int& quad, double& s, double& c) {
  const double j = rint(x * TWO_OVER_PI);
  const double r = (x - j * 1.57079632673412561417e+00) - j * 6.07710050650619224932e-11;
  const double z = r * r;
  const double ps = -1.66666666666666324348e-01 + z * (8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 +
                    z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10))));
  const double pc = 4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * (2.48015872894767294178e-05 +
                    z * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11))));
  s = r + r * z * ps;
  c = (1.0 - 0.5 * z) + z * z * pc;
  quad = (int)j;
}

__global__ void __launch_bounds__(256) pv_finish(const float2* __restrict__ P, const double* __restrict__ carry, float2* __restrict__ out,
                                                 i64 T, i64 n, i64 p, i64 q, int ntiles) {
  __shared__ double red[4];
  const int k = blockIdx.y;
  const i64 t = (i64)blockIdx.x * TILE + threadIdx.x;
  const float2* Prow = P + (size_t)k * (size_t)T;
  float m0, m1;
  double alpha, excl, total;
  const double dev = pv_bin(Prow, T, n, p, q, k, t, m0, m1, alpha);
  pv_block_scan(dev, red, excl, total);
  if (t >= n) return;
  const double theta = (double)Prow[0].y + (carry[(size_t)k * ntiles + blockIdx.x] + excl);
  const double mag = alpha * (double)m1 + (1.0 - alpha) * (double)m0;
  int quad;
  double s, c;
  pv_sincos(pv_wrap(theta), quad, s, c);
  const int turns = (quad + (k & 3) * (int)(t & 3)) & 3;  // e^{i r} i^turns
  const double re = (turns & 1) ? -s : c, im = (turns & 1) ? c : s;
  const double sign = (turns & 2) ? -1.0 : 1.0;
  out[(size_t)k * (size_t)n + (size_t)t] = float2{(float)(mag * (sign * re)), (float)(mag * (sign * im))};
}

// ---------------------------------------------------------------- identity phase locking ("Phase locking")
// Output frame t picks peaks of its interpolated magnitude; every bin k follows the peak P = P_t(k) nearest to it:
//   s_t[k] = s_{t-1}[P] + c_t(k),  c_t(k) = dev[P, t-1] + (arg X[k, i0] - arg X[P, i0]),  m4_t[k] = (m4_{t-1}[P] + P) mod 4,
//   out = mag e^{i wrap(s_t[k])} i^(m4_t[k]);  frame 0: s = arg X[k, 0], m4 = 0 (stored as the step P = k, c = arg X[k, 0], no turn).
// One frame is the map new[k] = old[P(k)] + c(k); such maps compose: (P2, c2) o (P1, c1) = (P1[P2], c1[P2] + c2).  Behind pv_polar:
//   pvl_prepare   a workgroup = LOCK_PREP output frames x 512 bins: the polar rows those frames read go through LDS (lanes along
//                 time on the way in, along frequency from there on); mag, the peaks, P, c, written time-major
//   pvl_tile_map  a workgroup = LOCK_TILE output frames: the composed map of the tile (P int16, c float64, quarter turns), ping-pong in LDS
//   pvl_carry     one workgroup, tile after tile: the state every tile starts from
//   pvl_finish    the tiles again from that state; sine / cosine; the stores go back to frequency-major through LDS
// Lanes are bins in all four; one barrier per frame; every sum has one order.
constexpr int LOCK_TILE = 256;  // output frames per workgroup of pvl_tile_map / pvl_finish (pv_ops.LOCK_TILE)
constexpr int LOCK_PREP = 4;    // output frames per workgroup of pvl_prepare (its LDS, 49 KB, lets three workgroups share a CU)
constexpr int LOCK_ITEMS = 2 * (LOCK_PREP + 1);  // staged polar columns: the pairs (i0, i0 + 1) of frames t0 - 1 .. t0 + LOCK_PREP - 1
constexpr int LOCK_PAD = NB + 1;                 // LDS row pitch of the staged columns
constexpr int LOCK_FLUSH = 16;                   // output frames that pvl_finish collects before it stores them

__global__ void __launch_bounds__(NB) pvl_prepare(const float2* __restrict__ Pol, short* __restrict__ pi, double* __restrict__ cs,
                                                  double* __restrict__ mags, i64 T, i64 n, i64 p, i64 q) {
  __shared__ float2 stage[LOCK_ITEMS * LOCK_PAD];
  __shared__ double magbuf[2][NB];
  __shared__ unsigned long long masks[2][NB / 64];
  __shared__ i64 i0s[LOCK_PREP + 1];
  __shared__ double alphas[LOCK_PREP + 1];
  const int k = threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * LOCK_PREP;
  if (k <= LOCK_PREP) {
    const i64 t = t0 - 1 + k;
    i64 i0 = -1;
    double alpha = 0.0;
    if (t >= 0 && t < n) {
      const i64 tp = t * p;
      i0 = tp / q;  // i0 <= T - 1 for every t < n
      alpha = (double)(tp - i0 * q) / (double)q;
    }
    i0s[k] = i0;
    alphas[k] = alpha;
  }
  __syncthreads();
  for (int idx = k; idx < NB * LOCK_ITEMS; idx += NB) {  // LOCK_ITEMS neighbouring lanes read one row's columns
    const int row = idx / LOCK_ITEMS, item = idx - row * LOCK_ITEMS;
    const i64 i0 = i0s[item >> 1], i = i0 + (item & 1);
    float2 v = float2{0.f, 0.f};  // frames T and T + 1 are zero (pv_polar never writes them)
    if (i0 >= 0 && i < T) v = Pol[(size_t)row * (size_t)T + (size_t)i];
    stage[item * LOCK_PAD + row] = v;
  }
  __syncthreads();
  const int wave = k >> 6, lane = k & 63;
  for (int f = 0; f < LOCK_PREP; ++f) {
    const i64 t = t0 + f;
    if (t >= n) break;
    const int b = f & 1;
    const float2 c0 = stage[(2 * f + 2) * LOCK_PAD + k], c1 = stage[(2 * f + 3) * LOCK_PAD + k];
    const double alpha = alphas[f + 1];
    const double mag = __dadd_rn(__dmul_rn(alpha, (double)c1.x), __dmul_rn(1.0 - alpha, (double)c0.x));
    magbuf[b][k] = mag;
    __syncthreads();
    bool peak = mag > 0.0;
    if (k >= 1) peak = peak && mag > magbuf[b][k - 1];
    if (k >= 2) peak = peak && mag > magbuf[b][k - 2];
    if (k + 1 < NB) peak = peak && mag >= magbuf[b][k + 1];
    if (k + 2 < NB) peak = peak && mag >= magbuf[b][k + 2];
    const unsigned long long mine = __ballot(peak);
    if (lane == 0) masks[b][wave] = mine;
    __syncthreads();
    int lo = -1, hi = -1;  // the nearest peak at or below k, at or above k
    unsigned long long m = mine & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    for (int w = wave; w >= 0; --w) {
      if (w != wave) m = masks[b][w];
      if (m) {
        lo = 64 * w + 63 - __clzll((long long)m);
        break;
      }
    }
    m = mine & (~0ull << lane);
    for (int w = wave; w < NB / 64; ++w) {
      if (w != wave) m = masks[b][w];
      if (m) {
        hi = 64 * w + __ffsll((long long)m) - 1;
        break;
      }
    }
    int P = k;  // no peak in the frame: the unlocked rule
    if (lo >= 0 && hi >= 0) P = (k - lo <= hi - k) ? lo : hi;  // a tie goes to the lower peak
    else if (lo >= 0) P = lo;
    else if (hi >= 0) P = hi;
    double c = (double)c0.y;  // frame 0: the state starts as arg X[k, 0]
    if (t > 0) {  // dev[P, t - 1] from the pair of frame t - 1
      const double dev = pv_wrap(((double)stage[(2 * f + 1) * LOCK_PAD + P].y - (double)stage[(2 * f) * LOCK_PAD + P].y) - (double)(P & 3) * PI_2);
      c = dev + ((double)c0.y - (double)stage[(2 * f + 2) * LOCK_PAD + P].y);
    }
    const size_t at = (size_t)t * NB + k;
    pi[at] = (short)(t > 0 ? P : k);
    cs[at] = c;
    mags[at] = mag;
  }
}

// the composed map of every tile but the last: state_end[k] = state_start[Pi[k]] + C[k], turns likewise
__global__ void __launch_bounds__(NB) pvl_tile_map(const short* __restrict__ pi, const double* __restrict__ cs, short* __restrict__ sumPi,
                                                   double* __restrict__ sumC, unsigned char* __restrict__ sumM, i64 n) {
  __shared__ double C[2][NB];
  __shared__ short Pi[2][NB];
  __shared__ unsigned char M[2][NB];
  const int k = threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * LOCK_TILE, t1 = (t0 + LOCK_TILE < n) ? t0 + LOCK_TILE : n;
  C[0][k] = 0.0;
  Pi[0][k] = (short)k;
  M[0][k] = 0;
  __syncthreads();
  size_t at = (size_t)t0 * NB + k;
  int P = pi[at], cur = 0;
  double c = cs[at];
  for (i64 t = t0; t < t1; ++t) {
    int Pn = 0;
    double cn = 0.0;
    if (t + 1 < t1) {  // the next frame's step is on its way while this one waits at the barrier
      Pn = pi[at + NB];
      cn = cs[at + NB];
    }
    C[cur ^ 1][k] = C[cur][P] + c;
    Pi[cur ^ 1][k] = Pi[cur][P];
    M[cur ^ 1][k] = (unsigned char)((M[cur][P] + (t > 0 ? P : 0)) & 3);
    __syncthreads();
    cur ^= 1;
    P = Pn;
    c = cn;
    at += NB;
  }
  const size_t o = (size_t)blockIdx.x * NB + k;
  sumPi[o] = Pi[cur][k];
  sumC[o] = C[cur][k];
  sumM[o] = M[cur][k];
}

__global__ void __launch_bounds__(NB) pvl_carry(const short* __restrict__ sumPi, const double* __restrict__ sumC,
                                                const unsigned char* __restrict__ sumM, double* __restrict__ startS,
                                                unsigned char* __restrict__ startM, int ntiles) {
  __shared__ double S[2][NB];
  __shared__ unsigned char M[2][NB];
  const int k = threadIdx.x;
  S[0][k] = 0.0;
  M[0][k] = 0;
  __syncthreads();
  int cur = 0;
  for (int j = 0; j < ntiles; ++j) {
    const size_t o = (size_t)j * NB + k;
    startS[o] = S[cur][k];
    startM[o] = M[cur][k];
    if (j + 1 == ntiles) break;  // the last tile has no summary
    const int P = sumPi[o];
    S[cur ^ 1][k] = S[cur][P] + sumC[o];
    M[cur ^ 1][k] = (unsigned char)((M[cur][P] + sumM[o]) & 3);
    __syncthreads();
    cur ^= 1;
  }
}

__global__ void __launch_bounds__(NB) pvl_finish(const short* __restrict__ pi, const double* __restrict__ cs, const double* __restrict__ mags,
                                                 const double* __restrict__ startS, const unsigned char* __restrict__ startM,
                                                 float2* __restrict__ out, i64 n) {
  __shared__ double S[2][NB];
  __shared__ unsigned char M[2][NB];
  __shared__ float2 rows[NB * (LOCK_FLUSH + 1)];
  const int k = threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * LOCK_TILE, t1 = (t0 + LOCK_TILE < n) ? t0 + LOCK_TILE : n;
  S[0][k] = startS[(size_t)blockIdx.x * NB + k];
  M[0][k] = startM[(size_t)blockIdx.x * NB + k];
  __syncthreads();
  size_t at = (size_t)t0 * NB + k;
  int P = pi[at], cur = 0;
  double c = cs[at], mag = mags[at];
  for (i64 t = t0; t < t1; ++t) {
    int Pn = 0;
    double cn = 0.0, magn = 0.0;
    if (t + 1 < t1) {
      Pn = pi[at + NB];
      cn = cs[at + NB];
      magn = mags[at + NB];
    }
    const double s = S[cur][P] + c;
    const int m4 = (M[cur][P] + (t > 0 ? P : 0)) & 3;
    S[cur ^ 1][k] = s;
    M[cur ^ 1][k] = (unsigned char)m4;
    int quad;
    double sn, cn2;
    pv_sincos(pv_wrap(s), quad, sn, cn2);
    const int turns = (quad + m4) & 3;  // e^{i r} i^turns
    const double re = (turns & 1) ? -sn : cn2, im = (turns & 1) ? cn2 : sn;
    const double sign = (turns & 2) ? -1.0 : 1.0;
    const int g = (int)(t - t0) % LOCK_FLUSH;
    rows[k * (LOCK_FLUSH + 1) + g] = float2{(float)(mag * (sign * re)), (float)(mag * (sign * im))};
    __syncthreads();
    if (g == LOCK_FLUSH - 1 || t + 1 == t1) {  // LOCK_FLUSH neighbouring lanes store one row's run of frames
      const i64 tb = t - g;
      for (int idx = k; idx < NB * LOCK_FLUSH; idx += NB) {
        const int row = idx / LOCK_FLUSH, gg = idx % LOCK_FLUSH;
        if (gg <= g) out[(size_t)row * (size_t)n + (size_t)(tb + gg)] = rows[row * (LOCK_FLUSH + 1) + gg];
      }
      __syncthreads();  // `rows` is written again by the next frame
    }
    cur ^= 1;
    P = Pn;
    c = cn;
    mag = magn;
    at += NB;
  }
}

// 0: fine; else the reason
const char* bad_rate(i64 frames, int p, int q) {
  if (p < 1 || q < 1) return "p and q must be at least 1";
  if ((i64)p > 8 * (i64)q || (i64)q > 8 * (i64)p) return "the rate p / q must lie in [1/8, 8]";
  if (frames < 1) return "at least one frame expected";
  if ((unsigned __int128)frames * (unsigned)p >= ((unsigned __int128)1 << 62)) return "frames * p must stay below 2^62";
  return nullptr;
}

size_t polar_bytes(i64 frames) { return (((size_t)NB * (size_t)frames * sizeof(float2)) + 15) / 16 * 16; }

// the locked vocoder's workspace behind the polar rows, widest elements first (every part a multiple of 16 bytes)
struct LockLayout {
  size_t c, mag, sumC, startS, pi, sumPi, sumM, startM, total;
  int ntiles;
};

LockLayout lock_layout(i64 frames, i64 n) {
  LockLayout L;
  L.ntiles = (int)((n + LOCK_TILE - 1) / LOCK_TILE);
  const size_t bins = (size_t)NB * (size_t)n, tiles = (size_t)NB * (size_t)L.ntiles;
  size_t at = polar_bytes(frames);
  L.c = at, at += bins * sizeof(double);
  L.mag = at, at += bins * sizeof(double);
  L.sumC = at, at += tiles * sizeof(double);
  L.startS = at, at += tiles * sizeof(double);
  L.pi = at, at += bins * sizeof(short);
  L.sumPi = at, at += tiles * sizeof(short);
  L.sumM = at, at += tiles;
  L.startM = at, at += tiles;
  L.total = at;
  return L;
}

}  // namespace

extern "C" int64_t mg_phase_vocoder_len(int64_t frames, int p, int q) {
  if (bad_rate(frames, p, q)) return -1;
  return (int64_t)(((unsigned __int128)frames * (unsigned)q + (unsigned)p - 1) / (unsigned)p);
}

extern "C" size_t mg_phase_vocoder_ws_bytes(int64_t frames, int p, int q) {
  const int64_t n = mg_phase_vocoder_len(frames, p, q);
  if (n < 1 || n >= ((int64_t)1 << 31) - TILE || frames >= ((int64_t)1 << 31)) return 0;
  return polar_bytes(frames) + (size_t)NB * (size_t)((n + TILE - 1) / TILE) * sizeof(double);
}

extern "C" int mg_phase_vocoder(const float* x_c64, float* out_c64, void* ws, size_t ws_bytes, int64_t frames, int p, int q,
                                mg_stream_t stream) {
  MG_CHECK_ARG(x_c64 && out_c64 && ws, "mg_phase_vocoder: bad arguments");
  const char* why = bad_rate(frames, p, q);
  MG_CHECK_ARG(!why, "mg_phase_vocoder: %s (got frames %lld, p %d, q %d)", why, (long long)frames, p, q);
  const i64 T = frames, n = mg_phase_vocoder_len(frames, p, q);
  MG_CHECK_ARG(T < ((i64)1 << 31) && n < ((i64)1 << 31) - TILE, "mg_phase_vocoder: input and output must stay below 2^31 frames");
  MG_CHECK_ARG((reinterpret_cast<uintptr_t>(x_c64) | reinterpret_cast<uintptr_t>(out_c64)) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(ws) % 16 == 0,
               "mg_phase_vocoder: the spectra must be 8-byte aligned, the workspace 16-byte aligned");
  if (ws_bytes < mg_phase_vocoder_ws_bytes(frames, p, q)) {
    mg_set_error("mg_phase_vocoder: workspace too small");
    return MG_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const float2* X = reinterpret_cast<const float2*>(x_c64);
  float2* P = reinterpret_cast<float2*>(ws);
  double* sums = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + polar_bytes(T));
  const int ntiles = (int)((n + TILE - 1) / TILE);
  const int sparse = (i64)p >= 2 * (i64)q;
  const i64 items = sparse ? 2 * n : T;
  hipLaunchKernelGGL(pv_polar, dim3((unsigned)((items + 255) / 256), NB), dim3(256), 0, s, X, P, T, n, (i64)p, (i64)q, sparse);
  MG_CHECK_LAUNCH("mg_phase_vocoder(polar)");
  hipLaunchKernelGGL(pv_tile_sums, dim3(ntiles, NB), dim3(TILE), 0, s, P, sums, T, n, (i64)p, (i64)q, ntiles);
  MG_CHECK_LAUNCH("mg_phase_vocoder(tile sums)");
  hipLaunchKernelGGL(pv_row_scan, dim3(NB), dim3(256), 0, s, sums, ntiles);
  MG_CHECK_LAUNCH("mg_phase_vocoder(row scan)");
  hipLaunchKernelGGL(pv_finish, dim3(ntiles, NB), dim3(TILE), 0, s, P, sums, reinterpret_cast<float2*>(out_c64), T, n, (i64)p, (i64)q,
                     ntiles);
  MG_CHECK_LAUNCH("mg_phase_vocoder(finish)");
  return MG_OK;
}

extern "C" size_t mg_phase_vocoder_locked_ws_bytes(int64_t frames, int p, int q) {
  const int64_t n = mg_phase_vocoder_len(frames, p, q);
  if (n < 1 || n >= ((int64_t)1 << 31) - TILE || frames >= ((int64_t)1 << 31)) return 0;
  return lock_layout(frames, n).total;
}

extern "C" int mg_phase_vocoder_locked(const float* x_c64, float* out_c64, void* ws, size_t ws_bytes, int64_t frames, int p, int q,
                                       mg_stream_t stream) {
  MG_CHECK_ARG(x_c64 && out_c64 && ws, "mg_phase_vocoder_locked: bad arguments");
  const char* why = bad_rate(frames, p, q);
  MG_CHECK_ARG(!why, "mg_phase_vocoder_locked: %s (got frames %lld, p %d, q %d)", why, (long long)frames, p, q);
  const i64 T = frames, n = mg_phase_vocoder_len(frames, p, q);
  MG_CHECK_ARG(T < ((i64)1 << 31) && n < ((i64)1 << 31) - TILE, "mg_phase_vocoder_locked: input and output must stay below 2^31 frames");
  MG_CHECK_ARG((reinterpret_cast<uintptr_t>(x_c64) | reinterpret_cast<uintptr_t>(out_c64)) % 8 == 0 &&
               reinterpret_cast<uintptr_t>(ws) % 16 == 0,
               "mg_phase_vocoder_locked: the spectra must be 8-byte aligned, the workspace 16-byte aligned");
  if (ws_bytes < mg_phase_vocoder_locked_ws_bytes(frames, p, q)) {
    mg_set_error("mg_phase_vocoder_locked: workspace too small");
    return MG_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const LockLayout L = lock_layout(T, n);
  char* base = reinterpret_cast<char*>(ws);
  float2* P = reinterpret_cast<float2*>(ws);
  double* cs = reinterpret_cast<double*>(base + L.c);
  double* mags = reinterpret_cast<double*>(base + L.mag);
  double* sumC = reinterpret_cast<double*>(base + L.sumC);
  double* startS = reinterpret_cast<double*>(base + L.startS);
  short* pi = reinterpret_cast<short*>(base + L.pi);
  short* sumPi = reinterpret_cast<short*>(base + L.sumPi);
  unsigned char* sumM = reinterpret_cast<unsigned char*>(base + L.sumM);
  unsigned char* startM = reinterpret_cast<unsigned char*>(base + L.startM);
  const int sparse = (i64)p >= 2 * (i64)q;
  const i64 items = sparse ? 2 * n : T;
  hipLaunchKernelGGL(pv_polar, dim3((unsigned)((items + 255) / 256), NB), dim3(256), 0, s, reinterpret_cast<const float2*>(x_c64), P, T,
                     n, (i64)p, (i64)q, sparse);
  MG_CHECK_LAUNCH("mg_phase_vocoder_locked(polar)");
  hipLaunchKernelGGL(pvl_prepare, dim3((unsigned)((n + LOCK_PREP - 1) / LOCK_PREP)), dim3(NB), 0, s, P, pi, cs, mags, T, n, (i64)p, (i64)q);
  MG_CHECK_LAUNCH("mg_phase_vocoder_locked(prepare)");
  if (L.ntiles > 1) {  // the last tile's map is needed by nobody
    hipLaunchKernelGGL(pvl_tile_map, dim3(L.ntiles - 1), dim3(NB), 0, s, pi, cs, sumPi, sumC, sumM, n);
    MG_CHECK_LAUNCH("mg_phase_vocoder_locked(tile map)");
  }
  hipLaunchKernelGGL(pvl_carry, dim3(1), dim3(NB), 0, s, sumPi, sumC, sumM, startS, startM, L.ntiles);
  MG_CHECK_LAUNCH("mg_phase_vocoder_locked(carry)");
  hipLaunchKernelGGL(pvl_finish, dim3(L.ntiles), dim3(NB), 0, s, pi, cs, mags, startS, startM, reinterpret_cast<float2*>(out_c64), n);
  MG_CHECK_LAUNCH("mg_phase_vocoder_locked(finish)");
  return MG_OK;
}
