// Look-ahead true-peak limiter of a waveform (C, L): one gain curve g for all channels that keeps every sample of x G g under a
// ceiling c (definition, steps 1 - 6: DESIGN.md, "True-peak limiter").  With the look-ahead A the file is taken as preceded by A
// silent samples; positions p = n + A >= 0 count from the first of them, and the tiles of the release run over p.
//   lim_env_k          m[n], float32: the largest of |x_c[n]| and of the 4x interpolation at 4n - 3 .. 4n + 3 over the channels.  A tile
//                      of samples and its halo go through LDS per channel, the four phases are summed in the order of resample_k
//                      (as true_peak_k does), so every interpolated value has the resampler's bits
//   lim_release_k<0>   a workgroup = TILE positions.  Hold: r is a falling function of m, so min r over a window is r of max m,
//                      and the window maximum is taken on the float32 m by van Herk / Gil-Werman (prefix maxima of blocks of A + 1
//                      from the left, from the right, one comparison of the two).  Release: d = max(1 - h, rho d) is a scan over
//                      pairs (a, v) with (a1, v1) o (a2, v2) = (a1 a2, max(a2 v1, v2)); a thread runs 8 positions from zero
//                      state, the 256 end states are scanned with the powers rho^8, rho^16, ..: V[tile] = the end state of the tile
//   lim_carry_k        one workgroup: V[tile] <- the state at the start of the tile (a thread's run of tiles, a serial pass over the
//                      256 runs, the runs again) -- the scheme of loud_carry_k
//   lim_release_k<1>   the tiles again from their true state: q[p] = 1 - d[p], float64
//   lim_out_k          a workgroup = TILE samples: the sums of q over n .. n + A (positions) as differences of a prefix sum that
//                      starts anew in every tile (at most TILE + A terms of at most 1), the minimum with r[n], x G g rounded once
// Every intermediate but m is float64.  No atomics, every scan and sum has one order: the same bits on every run.  The loops that
// stage global memory issue all of their loads at clamped addresses first and drop what lay outside afterwards: written as
// `cond ? p[i] : 0`, every load is branched around and waited for on its own.
#include <cmath>
#include <cstdint>

#include "mg_common.h"

namespace {

constexpr int TILE = 2048;     // samples (positions) per workgroup (lim_ops.TILE)
constexpr int THREADS = 256;
constexpr int MAXA = 2047;     // look-ahead at most: a window never spans more than two tiles
constexpr int MAXC = 8;
constexpr int NP = 4096;       // TILE + MAXA, rounded up to THREADS * RUN
constexpr int RUN = NP / THREADS;          // elements per thread of a block scan at most
constexpr int NPP = NP + NP / RUN;         // an LDS array of NP elements, one element of padding after every 16
constexpr int REL = TILE / THREADS;        // positions per thread of the release
constexpr int TAPS = 15, HALF = 7, PHASES = 4;
constexpr int XLOADS = (TILE + TAPS + THREADS - 1) / THREADS;  // loads per thread that stage a tile and its halo

typedef long long i64;
typedef float f32x2 __attribute__((ext_vector_type(2)));

// 16 elements at a stride of 17: the threads' runs start on distinct banks
__device__ __forceinline__ int pad(int i) { return i + i / RUN; }

// n brought into [0, len): the address of a load whose value is dropped where n lies outside
__device__ __forceinline__ i64 clampi(i64 n, i64 len) { return n < 0 ? 0 : (n < len ? n : len - 1); }

// the gain that brings G m under the ceiling, 1 where it is there already
__device__ __forceinline__ double required_gain(double G, double c, float m) {
  const double e = G * (double)m;
  return e > c ? c / e : 1.0;
}

struct MaxF {
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct AddD {
  __device__ __forceinline__ double operator()(double a, double b) const { return a + b; }
};

// a[pad(i)], i < N = run * 256, in place: the running `op` from the start of i's block to i, blocks of W from element 0 (REV: from i
// to the end of its block, scanned from the right; SEG == false: one block).  A thread owns `run` consecutive elements; the states
// at the ends of the runs are carried over the 256 threads by a scan of (a block started in the run, state).  Begins and ends with
// a barrier.
template <typename T, typename Op, bool REV, bool SEG>
__device__ __forceinline__ void block_scan(T* a, int run, int W, T ident, T* cv, int* cf, Op op) {
  const int t = threadIdx.x, N = run * THREADS;
  const int i0 = REV ? N - 1 - t * run : t * run, ph0 = SEG ? i0 % W : i0;  // ph: the place of i in its block
  T acc = ident;
  int flag = 0, first = run;
  for (int k = 0, i = i0, ph = ph0; k < run; ++k) {
    const bool start = SEG ? ph == (REV ? W - 1 : 0) : i == 0;
    if (start) {
      acc = a[pad(i)];
      if (!flag) first = k;
      flag = 1;
    } else {
      acc = op(acc, a[pad(i)]);
      a[pad(i)] = acc;
    }
    if (REV) {
      --i;
      ph = ph == 0 ? W - 1 : ph - 1;
    } else {
      ++i;
      ph = ph + 1 == W ? 0 : ph + 1;
    }
  }
  __syncthreads();
  cv[t] = acc;
  cf[t] = flag;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    T v = cv[t];
    int f = cf[t];
    if (t >= d) {
      if (!f) v = op(cv[t - d], v);
      f |= cf[t - d];
    }
    __syncthreads();
    cv[t] = v;
    cf[t] = f;
    __syncthreads();
  }
  if (t > 0) {
    const T carry = cv[t - 1];
    for (int k = 0; k < first; ++k) {
      const int i = REV ? i0 - k : i0 + k;
      a[pad(i)] = op(carry, a[pad(i)]);
    }
  }
  __syncthreads();
}

// m[n] = max over the channels of max(|x[n]|, |u[4n - 3 .. 4n + 3]|), u[4 s + p] = sum_j x[s - 7 + j] h[p][j] with x zero outside
// [0, L): the outputs of mg_resample_pcm(1 -> 4); u outside [0, 4 L) does not count.
__global__ void __launch_bounds__(THREADS) lim_env_k(const float* __restrict__ x, i64 row_stride, int C, i64 L,
                                                     const float* __restrict__ bank, float* __restrict__ m) {
  __shared__ float xs[TILE + TAPS];   // samples t0 - 8 .. t0 + TILE + 6: the windows of the samples t0 - 1 .. t0 + TILE - 1
  __shared__ float e0[TILE + 1];      // per sample t0 - 1 + j: max(|x|, |phase 0|) over the channels so far
  __shared__ float e1[TILE + 1];      //                        max(|phase 1|, |phase 2|, |phase 3|)
  const int tid = threadIdx.x;
  const i64 t0 = (i64)blockIdx.x * TILE;
  f32x2 h01[TAPS], h23[TAPS];  // phases 0 and 1, 2 and 3, side by side (uniform: scalar registers)
#pragma unroll
  for (int j = 0; j < TAPS; ++j) {
    h01[j] = f32x2{bank[j], bank[TAPS + j]};
    h23[j] = f32x2{bank[2 * TAPS + j], bank[3 * TAPS + j]};
  }
  for (int c = 0; c < C; ++c) {
    const float* __restrict__ xc = x + (i64)c * row_stride;
    if (c > 0) __syncthreads();  // xs is still being read
    float xr[XLOADS];  // every load goes out, at a clamped address, before the first is used (a branch around a load waits for it)
#pragma unroll
    for (int k = 0; k < XLOADS; ++k) {
      const int i = min(tid + k * THREADS, TILE + TAPS - 1);
      xr[k] = xc[clampi(t0 - HALF - 1 + i, L)];
    }
#pragma unroll
    for (int k = 0; k < XLOADS; ++k) {
      const int i = tid + k * THREADS;
      const i64 s = t0 - HALF - 1 + i;
      if (i < TILE + TAPS) xs[i] = (s >= 0 && s < L) ? xr[k] : 0.f;
    }
    __syncthreads();
    for (int j = tid; j < TILE + 1; j += THREADS) {
      const i64 s = t0 - 1 + j;
      float a = 0.f, b = 0.f;
      if (s >= 0 && s < L) {
        const float* w = xs + j;
        f32x2 a01 = f32x2{w[0], w[0]} * h01[0], a23 = f32x2{w[0], w[0]} * h23[0];
#pragma unroll
        for (int k = 1; k < TAPS; ++k) {
          const f32x2 xv = f32x2{w[k], w[k]};
          a01 = __builtin_elementwise_fma(xv, h01[k], a01);
          a23 = __builtin_elementwise_fma(xv, h23[k], a23);
        }
        a = fmaxf(fabsf(w[HALF]), fabsf(a01.x));
        b = fmaxf(fabsf(a01.y), fmaxf(fabsf(a23.x), fabsf(a23.y)));
      }
      if (c > 0) {  // the thread that wrote them
        a = fmaxf(a, e0[j]);
        b = fmaxf(b, e1[j]);
      }
      e0[j] = a;
      e1[j] = b;
    }
  }
  __syncthreads();
  for (int i = tid; i < TILE; i += THREADS) {
    const i64 n = t0 + i;
    if (n < L) m[n] = fmaxf(fmaxf(e0[i + 1], e1[i + 1]), e1[i]);
  }
}

// Positions p0 .. p0 + TILE - 1 of tile blockIdx.x; position p is sample n = p - A.  APPLY == false: V[tile] = the release state d
// at the end of the tile from zero state.  APPLY == true: V[tile] is the state at the start of the tile; q[p] = 1 - d[p], p < L + A.
// rho8 = rho^REL; run = the elements per thread of the scans, run * 256 >= TILE + A.
template <bool APPLY>
__global__ void __launch_bounds__(THREADS) lim_release_k(const float* __restrict__ m, i64 L, int A, int run,
                                                         const double* __restrict__ pregain, double c, double rho, double rho8,
                                                         double* __restrict__ V, double* __restrict__ q) {
  __shared__ double buf[NPP];  // two float arrays of NPP; then, once the hold is taken, TILE + THREADS float64 of q
  __shared__ float cvf[THREADS];
  __shared__ int cf[THREADS];
  __shared__ double sc[THREADS];
  float* pre = reinterpret_cast<float*>(buf);
  float* suf = pre + NPP;
  double* qs = buf;  // a thread's REL values at a stride of REL + 1
  const int tid = threadIdx.x;
  const i64 p0 = (i64)blockIdx.x * TILE;
  float mr[RUN];  // m over the samples p0 - A .. p0 + TILE - 1, the tile and its windows: all loads first, at clamped addresses
#pragma unroll
  for (int k = 0; k < RUN; ++k) mr[k] = m[clampi(p0 + min(tid + k * THREADS, TILE + A - 1) - A, L)];
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const int i = tid + k * THREADS;
    const i64 n = p0 + i - A;
    if (k < run) {
      const float v = (i < TILE + A && n >= 0 && n < L) ? mr[k] : 0.f;
      pre[pad(i)] = v;
      suf[pad(i)] = v;
    }
  }
  __syncthreads();
  block_scan<float, MaxF, false, true>(pre, run, A + 1, 0.f, cvf, cf, MaxF());
  block_scan<float, MaxF, true, true>(suf, run, A + 1, 0.f, cvf, cf, MaxF());
  const double G = pregain[0];
  double u[REL];  // 1 - h
#pragma unroll
  for (int k = 0; k < REL; ++k) {
    const int i = tid * REL + k;
    u[k] = 1.0 - required_gain(G, c, fmaxf(suf[pad(i)], pre[pad(i + A)]));
  }
  double v = 0.0;
  if constexpr (APPLY) {
    if (tid == 0) v = V[blockIdx.x];
  }
#pragma unroll
  for (int k = 0; k < REL; ++k) v = fmax(u[k], rho * v);
  sc[tid] = v;
  __syncthreads();  // pre and suf are read: qs may take their place
  double pw = rho8;  // rho^(REL d)
  for (int d = 1; d < THREADS; d <<= 1) {
    const double o = tid >= d ? sc[tid - d] : 0.0;
    __syncthreads();
    if (tid >= d) sc[tid] = fmax(sc[tid], pw * o);
    __syncthreads();
    pw *= pw;
  }
  if constexpr (!APPLY) {
    if (tid == THREADS - 1) V[blockIdx.x] = sc[THREADS - 1];
  } else {
    v = tid > 0 ? sc[tid - 1] : V[blockIdx.x];
#pragma unroll
    for (int k = 0; k < REL; ++k) {
      v = fmax(u[k], rho * v);
      qs[tid * (REL + 1) + k] = 1.0 - v;
    }
    __syncthreads();
    for (int i = tid; i < TILE; i += THREADS)
      if (p0 + i < L + A) q[p0 + i] = qs[i + i / REL];
  }
}

// V[k]: the zero-state end state of tile k on entry, the state at the start of tile k on return.  PT = rho^TILE, PP = PT^per; thread
// t owns the tiles t per .. (t + 1) per - 1 (a short or empty run sits at the end, where nothing follows).
__global__ void __launch_bounds__(THREADS) lim_carry_k(double* __restrict__ V, int nt, int per, double PT, double PP) {
  __shared__ double E[THREADS];
  const int t = threadIdx.x;
  const i64 lo = (i64)t * per;
  const i64 hi = lo + per < nt ? lo + per : nt;
  double v = 0.0;
  for (i64 k = lo; k < hi; ++k) v = fmax(V[k], PT * v);
  E[t] = v;
  __syncthreads();
  if (t == 0) {  // E[u] = the state at the start of thread u's run
    double c = 0.0;
    for (int u = 0; u < THREADS; ++u) {
      const double z = E[u];
      E[u] = c;
      c = fmax(z, PP * c);
    }
  }
  __syncthreads();
  v = E[t];
  for (i64 k = lo; k < hi; ++k) {
    const double z = V[k];
    V[k] = v;
    v = fmax(z, PT * v);
  }
}

// g[n] = min(r[n], (q[n] + .. + q[n + A]) / (A + 1)) over positions, out[c][n] = float32(double(x[c][n]) G g[n])
__global__ void __launch_bounds__(THREADS) lim_out_k(const float* __restrict__ x, i64 row_stride, int C, i64 L, int A, int run,
                                                     const float* __restrict__ m, const double* __restrict__ q,
                                                     const double* __restrict__ pregain, double c, float* __restrict__ out,
                                                     double* __restrict__ gain_out) {
  __shared__ double S[NPP];
  __shared__ double cv[THREADS];
  __shared__ int cf[THREADS];
  const int tid = threadIdx.x;
  const i64 n0 = (i64)blockIdx.x * TILE;
  double qr[RUN];  // all loads first, at clamped addresses
#pragma unroll
  for (int k = 0; k < RUN; ++k) qr[k] = q[clampi(n0 + min(tid + k * THREADS, TILE + A - 1), L + A)];
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    const int i = tid + k * THREADS;
    if (k < run) S[pad(i)] = (i < TILE + A && n0 + i < L + A) ? qr[k] : 0.0;
  }
  __syncthreads();
  block_scan<double, AddD, false, false>(S, run, 0, 0.0, cv, cf, AddD());  // one block: S[i] = q[n0] + .. + q[n0 + i]
  const double G = pregain[0], width = (double)(A + 1);
  float mr[REL];
#pragma unroll
  for (int k = 0; k < REL; ++k) mr[k] = m[clampi(n0 + tid + k * THREADS, L)];
  double g[REL];
#pragma unroll
  for (int k = 0; k < REL; ++k) {
    const int i = tid + k * THREADS;
    const double below = i > 0 ? S[pad(i - 1)] : 0.0;
    g[k] = fmin(required_gain(G, c, mr[k]), (S[pad(i + A)] - below) / width);
    if (gain_out && n0 + i < L) gain_out[n0 + i] = g[k];
  }
  for (int ch = 0; ch < C; ++ch) {
    const float* __restrict__ xc = x + (i64)ch * row_stride;
    float xr[REL];
#pragma unroll
    for (int k = 0; k < REL; ++k) xr[k] = xc[clampi(n0 + tid + k * THREADS, L)];
#pragma unroll
    for (int k = 0; k < REL; ++k) {
      const i64 n = n0 + tid + k * THREADS;
      if (n < L) out[(i64)ch * L + n] = (float)(((double)xr[k] * G) * g[k]);
    }
  }
}

// out = float32(double(y) min(1, c / peak))
__global__ void __launch_bounds__(THREADS) lim_trim_k(const float* __restrict__ y, float* __restrict__ out, i64 n,
                                                      const float* __restrict__ peak, double c) {
  const double t = fmin(1.0, c / (double)peak[0]);
  const i64 step = (i64)gridDim.x * THREADS;
  for (i64 i = (i64)blockIdx.x * THREADS + threadIdx.x; i < n; i += step) out[i] = (float)((double)y[i] * t);
}

// G = prev 10^((target - L_int) / 20), prev = 1 without one; the factor is 1 where L_int = -inf
__global__ void lim_pregain_k(const double* __restrict__ record, double target, const double* __restrict__ prev,
                              double* __restrict__ G) {
  const double l = record[0], p = prev ? prev[0] : 1.0;
  G[0] = l != -INFINITY ? p * pow(10.0, (target - l) / 20.0) : p;
}

size_t align16(size_t n) { return (n + 15) / 16 * 16; }

bool plan(int C, i64 L, int A, i64* nt) {
  if (C < 1 || C > MAXC || L < 0 || A < 0 || A > MAXA) return false;
  *nt = (L + A + TILE - 1) / TILE;
  return *nt < ((i64)1 << 31);
}

bool check_bank(const char* who, const void* bank, size_t bank_bytes) {
  int phases = 0, taps = 0;
  const size_t need = mg_resample_bank_size(1, 4, 6, 0.99, &phases, &taps);
  if (bank && phases == PHASES && taps == TAPS && bank_bytes >= need) return true;
  mg_set_error("%s: the bank of mg_resample_bank(1, 4, 6, 0.99) expected (%zu bytes, 4 x 15 taps)", who, need);
  return false;
}

}  // namespace

extern "C" int mg_limiter_tile(void) { return TILE; }

extern "C" size_t mg_limiter_ws_bytes(int C, int64_t L, int A) {
  i64 nt;
  if (!plan(C, L, A, &nt)) return 0;
  return align16((size_t)L * sizeof(float)) + align16((size_t)nt * sizeof(double)) + (size_t)(L + A) * sizeof(double) + 16;
}

extern "C" int mg_limiter_envelope(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes, float* m,
                                   mg_stream_t stream) {
  MG_CHECK_ARG(C >= 1 && C <= MAXC && L >= 0 && row_stride >= 0 && (C == 1 || row_stride >= L), "mg_limiter_envelope: bad arguments");
  if (!check_bank("mg_limiter_envelope", bank, bank_bytes)) return MG_EINVAL;
  if (L == 0) return MG_OK;
  const i64 tiles = (L + TILE - 1) / TILE;
  MG_CHECK_ARG(x && m && tiles < ((i64)1 << 31), "mg_limiter_envelope: null pointer or too many samples");
  hipLaunchKernelGGL(lim_env_k, dim3((unsigned)tiles), dim3(THREADS), 0, (hipStream_t)stream, x, (i64)row_stride, C, (i64)L,
                     reinterpret_cast<const float*>(bank), m);
  MG_CHECK_LAUNCH("mg_limiter_envelope");
  return MG_OK;
}

extern "C" int mg_limiter(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes,
                          const double* pregain, double ceiling, int A, double rho, float* out, double* gain_out, void* ws,
                          size_t ws_bytes, mg_stream_t stream) {
  i64 nt;
  MG_CHECK_ARG(plan(C, L, A, &nt), "mg_limiter: 1 .. %d channels, L >= 0 and a look-ahead of 0 .. %d samples expected (got %d, %lld, %d)",
               MAXC, MAXA, C, (long long)L, A);
  MG_CHECK_ARG(row_stride >= 0 && (C == 1 || row_stride >= L), "mg_limiter: bad row stride");
  MG_CHECK_ARG(std::isfinite(ceiling) && ceiling > 0.0 && rho > 0.0 && rho < 1.0,
               "mg_limiter: a positive finite ceiling and a release factor in (0, 1) expected (got %g, %g)", ceiling, rho);
  if (!check_bank("mg_limiter", bank, bank_bytes)) return MG_EINVAL;
  if (L == 0) return MG_OK;
  MG_CHECK_ARG(x && out && pregain && ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0 && reinterpret_cast<uintptr_t>(pregain) % 8 == 0 &&
                   reinterpret_cast<uintptr_t>(gain_out) % 8 == 0,
               "mg_limiter: null or misaligned pointer");
  if (ws_bytes < mg_limiter_ws_bytes(C, L, A)) {
    mg_set_error("mg_limiter: workspace too small");
    return MG_EWORKSPACE;
  }
  char* base = reinterpret_cast<char*>(ws);
  float* m = reinterpret_cast<float*>(base);
  double* V = reinterpret_cast<double*>(base + align16((size_t)L * sizeof(float)));
  double* q = reinterpret_cast<double*>(base + align16((size_t)L * sizeof(float)) + align16((size_t)nt * sizeof(double)));
  const int per = (int)((nt + THREADS - 1) / THREADS);
  const int run = (TILE + A + THREADS - 1) / THREADS;  // 8 .. 16 elements per thread of the scans over a tile and its halo
  double rho8 = rho;  // rho^REL by squaring (REL = 8)
  for (int i = REL; i > 1; i >>= 1) rho8 *= rho8;
  const double PT = std::pow(rho, (double)TILE), PP = std::pow(rho, (double)TILE * (double)per);
  const i64 tiles = (L + TILE - 1) / TILE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(lim_env_k, dim3((unsigned)tiles), dim3(THREADS), 0, s, x, (i64)row_stride, C, (i64)L,
                     reinterpret_cast<const float*>(bank), m);
  MG_CHECK_LAUNCH("mg_limiter(envelope)");
  hipLaunchKernelGGL(lim_release_k<false>, dim3((unsigned)nt), dim3(THREADS), 0, s, m, (i64)L, A, run, pregain, ceiling, rho, rho8, V, q);
  MG_CHECK_LAUNCH("mg_limiter(tile states)");
  hipLaunchKernelGGL(lim_carry_k, dim3(1), dim3(THREADS), 0, s, V, (int)nt, per, PT, PP);
  MG_CHECK_LAUNCH("mg_limiter(carry)");
  hipLaunchKernelGGL(lim_release_k<true>, dim3((unsigned)nt), dim3(THREADS), 0, s, m, (i64)L, A, run, pregain, ceiling, rho, rho8, V, q);
  MG_CHECK_LAUNCH("mg_limiter(release)");
  hipLaunchKernelGGL(lim_out_k, dim3((unsigned)tiles), dim3(THREADS), 0, s, x, (i64)row_stride, C, (i64)L, A, run, m, q, pregain,
                     ceiling, out, gain_out);
  MG_CHECK_LAUNCH("mg_limiter(output)");
  return MG_OK;
}

extern "C" int mg_limiter_trim(const float* y, float* out, int64_t n, const float* peak, double ceiling, mg_stream_t stream) {
  MG_CHECK_ARG(peak && n >= 0 && ((y && out) || n == 0) && std::isfinite(ceiling) && ceiling > 0.0, "mg_limiter_trim: bad arguments");
  if (n == 0) return MG_OK;
  i64 blocks = (n + 4 * THREADS - 1) / (4 * THREADS);  // four elements per thread
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(lim_trim_k, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, y, out, (i64)n, peak, ceiling);
  MG_CHECK_LAUNCH("mg_limiter_trim");
  return MG_OK;
}

extern "C" int mg_limiter_pregain(const double* record, double target, const double* prev, double* pregain, mg_stream_t stream) {
  MG_CHECK_ARG(record && pregain && std::isfinite(target), "mg_limiter_pregain: bad arguments");
  hipLaunchKernelGGL(lim_pregain_k, dim3(1), dim3(1), 0, (hipStream_t)stream, record, target, prev, pregain);
  MG_CHECK_LAUNCH("mg_limiter_pregain");
  return MG_OK;
}
