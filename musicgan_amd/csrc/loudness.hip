// Programme loudness (ITU-R BS.1770-4 / EBU R128) and true peak of a waveform (C, L), and the gain that brings it to a target
// (definitions and the chunked-state derivation: DESIGN.md, "Loudness").
//
// K-weighting is two biquads in cascade, a serial recurrence along the whole file.  Both run in transposed direct form II, so the
// filter is the linear system v' = A v + B x on the four states v = (s1, s2, t1, t2); everything about it is float64.  Each channel
// is cut into chunks of CHUNK samples and the state is carried across them by the affine map  v_end = A^CHUNK v_start + z,  z the
// end state of the chunk filtered from zero state:
//   loud_chunk_k<false>  a thread = one chunk: z of every chunk, in parallel                      (reads the signal once)
//   loud_carry_k         a workgroup = one channel: v_start of every chunk, in place of z.  Three levels of the same idea (a
//                        thread's run of chunks, 16 threads, 16 groups), each "scan from zero, carry, scan again from the carry"
//   loud_chunk_k<true>   the chunks again, each from its true v_start: the squares of the output summed per piece -- a piece is what
//                        one chunk holds of one 100 ms segment, numbered chunk + segment                (reads the signal again)
//   loud_segments_k      S[c][j] = the pieces of segment j in chunk order
// The filtered signal is never written.  A workgroup of 256 threads owns 256 consecutive chunks; the samples go through LDS in
// slices of 32 per chunk, loaded as 128-byte runs and read back one row per thread (row stride 33: conflict-free), so that no lane
// ever loads from HBM at a 4 KB stride.  No atomics, every sum has one order: the same bits on every run.
//
// loud_gate_k: the two gates over the 400 ms blocks, one workgroup, float64.  true_peak_k: the 4 x 15 polyphase bank of
// mg_resample_pcm(1 -> 4) applied from LDS, the 4x signal reduced to one maximum per workgroup and never written; the sums have the
// order of resample_k, so every interpolated value has its bits.  loud_gain_k / loud_scale_k: the gain, left in device memory, and
// the scaled waveform.
#include <cmath>
#include <cstdint>

#include "mg_common.h"

namespace {

constexpr int CHUNK = 1024;    // samples per chunk (loud_ops.CHUNK)
constexpr int ROWS = 256;      // chunks per workgroup = threads per workgroup
constexpr int SLICE = 32;      // samples of every chunk staged at a time
constexpr int MAXC = 8;        // channels at most
constexpr int TP_TILE = 2048;  // input samples per workgroup of true_peak_k
constexpr int TP_W = 7, TP_TAPS = 15, TP_PHASES = 4;

typedef long long i64;
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Coef {
  double b0, b1, b2, a1, a2;  // shelf
  double c0, c1, c2, d1, d2;  // high-pass
};
struct Mat4 {
  double m[16];
};
struct Weights {
  double g[MAXC];
};

// one sample through both stages (transposed direct form II); returns the K-weighted sample
__host__ __device__ __forceinline__ double kw_step(const Coef& k, double v[4], double x) {
  const double y1 = fma(k.b0, x, v[0]);
  v[0] = fma(-k.a1, y1, fma(k.b1, x, v[1]));
  v[1] = fma(-k.a2, y1, k.b2 * x);
  const double y2 = fma(k.c0, y1, v[2]);
  v[2] = fma(-k.d1, y2, fma(k.c1, y1, v[3]));
  v[3] = fma(-k.d2, y2, k.c2 * y1);
  return y2;
}

// v = M v + z
__device__ __forceinline__ void affine(const Mat4& M, double v[4], const double z[4]) {
  double r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
    r[i] = fma(M.m[4 * i + 3], v[3], fma(M.m[4 * i + 2], v[2], fma(M.m[4 * i + 1], v[1], fma(M.m[4 * i], v[0], z[i]))));
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = r[i];
}

// ENERGY == false: st[c][k] = end state of chunk k from zero state.  ENERGY == true: st[c][k] is the state at the start of chunk k;
// pieces[c][k + j] = sum of y^2 over the samples of chunk k in segment j, for every segment j < nseg that the chunk meets.
// N = nseg * seg samples per channel are filtered; nch = ceil(N / CHUNK).
template <bool ENERGY>
__global__ void __launch_bounds__(ROWS) loud_chunk_k(const float* __restrict__ x, i64 row_stride, i64 N, int nch, int seg, i64 nseg,
                                                     Coef kc, double* __restrict__ st, double* __restrict__ pieces) {
  __shared__ float tile[ROWS][SLICE + 1];
  const int tid = threadIdx.x, c = blockIdx.y;
  const i64 k0 = (i64)blockIdx.x * ROWS, k = k0 + tid;
  const float* __restrict__ xc = x + (i64)c * row_stride;
  const bool live = k < nch;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  double* stk = st + ((i64)c * nch + (live ? k : 0)) * 4;
  double* pc = nullptr;
  i64 j = 0;
  int rem = 0, cnt = 0;
  double acc = 0.0;
  if constexpr (ENERGY) {
    if (live) {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = stk[i];
    }
    const i64 p0 = k * CHUNK;
    j = p0 / seg;
    rem = (int)((j + 1) * seg - p0);
    pc = pieces + (i64)c * (nch + nseg) + k;
  }
  for (int t0 = 0; t0 < CHUNK; t0 += SLICE) {
    float ld[SLICE];
#pragma unroll
    for (int r = 0; r < SLICE; ++r) {
      const int idx = r * ROWS + tid, row = idx / SLICE, col = idx % SLICE;
      const i64 pos = (k0 + row) * CHUNK + t0 + col;
      ld[r] = pos < N ? xc[pos] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < SLICE; ++r) {
      const int idx = r * ROWS + tid;
      tile[idx / SLICE][idx % SLICE] = ld[r];
    }
    __syncthreads();
    if (live) {
#pragma unroll 4
      for (int t = 0; t < SLICE; ++t) {
        const double y = kw_step(kc, v, (double)tile[tid][t]);
        if constexpr (ENERGY) {
          acc = fma(y, y, acc);
          ++cnt;
          if (--rem == 0) {  // the segment ends with this sample
            if (j < nseg) pc[j] = acc;
            ++j;
            rem = seg;
            acc = 0.0;
            cnt = 0;
          }
        }
      }
    }
    __syncthreads();
  }
  if (!live) return;
  if constexpr (ENERGY) {
    if (cnt > 0 && j < nseg) pc[j] = acc;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) stk[i] = v[i];
  }
}

// st[c][k]: the zero-state end state of chunk k on entry, the state at the start of chunk k on return.  M = A^CHUNK, MP = M^per,
// MG = MP^16; thread t owns the chunks t per .. (t + 1) per - 1.  (A thread whose run is short or empty sits at the end of the
// channel, where nothing follows: MP stands for every thread's run.)
__global__ void __launch_bounds__(256) loud_carry_k(double* __restrict__ st, int nch, int per, Mat4 M, Mat4 MP, Mat4 MG) {
  __shared__ double E[256][4], G[16][4];
  const int t = threadIdx.x;
  double* s = st + (i64)blockIdx.x * nch * 4;
  const i64 lo = (i64)t * per;
  const i64 hi = lo + per < nch ? lo + per : nch;
  double v[4] = {0.0, 0.0, 0.0, 0.0}, z[4];
  for (i64 k = lo; k < hi; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = s[k * 4 + i];
    affine(M, v, z);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) E[t][i] = v[i];
  __syncthreads();
  if (t % 16 == 0) {  // the end state of 16 threads' runs from zero state
    double g[4] = {0.0, 0.0, 0.0, 0.0};
    for (int u = 0; u < 16; ++u) affine(MP, g, E[t + u]);
#pragma unroll
    for (int i = 0; i < 4; ++i) G[t / 16][i] = g[i];
  }
  __syncthreads();
  if (t == 0) {  // G[g] = the state at the start of group g
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for (int g = 0; g < 16; ++g) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        z[i] = G[g][i];
        G[g][i] = c[i];
      }
      affine(MG, c, z);
    }
  }
  __syncthreads();
  if (t % 16 == 0) {  // E[t] = the state at the start of thread t's run
    double c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = G[t / 16][i];
    for (int u = 0; u < 16; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        z[i] = E[t + u][i];
        E[t + u][i] = c[i];
      }
      affine(MP, c, z);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = E[t][i];
  for (i64 k = lo; k < hi; ++k) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      z[i] = s[k * 4 + i];
      s[k * 4 + i] = v[i];
    }
    affine(M, v, z);
  }
}

// S[c][j] = the pieces of segment j, in chunk order
__global__ void __launch_bounds__(256) loud_segments_k(const double* __restrict__ pieces, double* __restrict__ S, int nch, int seg,
                                                       i64 nseg) {
  const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
  if (j >= nseg) return;
  const int c = blockIdx.y;
  const double* pc = pieces + (i64)c * (nch + nseg) + j;
  const i64 klo = j * seg / CHUNK, khi = ((j + 1) * seg - 1) / CHUNK;
  double acc = pc[klo];
  for (i64 k = klo + 1; k <= khi; ++k) acc += pc[k];
  S[(i64)c * nseg + j] = acc;
}

// mean square of block i (segments i .. i + 3), weighted over the channels
__device__ __forceinline__ double block_z(const double* __restrict__ S, const Weights& w, int C, i64 nseg, double inv, i64 i) {
  double z = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* s = S + (i64)c * nseg + i;
    z += w.g[c] * (((s[0] + s[1]) + s[2]) + s[3]);
  }
  return z * inv;
}

// record = (integrated LUFS, momentary maximum, blocks above the absolute gate, blocks above both gates)
__global__ void __launch_bounds__(256) loud_gate_k(const double* __restrict__ S, Weights w, int C, i64 nseg, int seg,
                                                   double* __restrict__ record) {
  __shared__ double red[256];
  const double ninf = -INFINITY;
  const i64 nb = nseg - 3;
  if (nb < 1) {
    if (threadIdx.x == 0) {
      record[0] = ninf;
      record[1] = ninf;
      record[2] = 0.0;
      record[3] = 0.0;
    }
    return;
  }
  const double inv = 1.0 / (4.0 * (double)seg);
  double sum = 0.0, cnt = 0.0, top = ninf;
  for (i64 i = threadIdx.x; i < nb; i += 256) {
    const double z = block_z(S, w, C, nseg, inv, i);
    const double l = -0.691 + 10.0 * log10(z);
    top = fmax(top, l);
    if (l > -70.0) {
      sum += z;
      cnt += 1.0;
    }
  }
  sum = mg_block_sum_f64(sum, red);
  cnt = mg_block_sum_f64(cnt, red);
  top = mg_block_max_f64(top, red);
  if (cnt == 0.0) {
    if (threadIdx.x == 0) {
      record[0] = ninf;
      record[1] = top;
      record[2] = 0.0;
      record[3] = 0.0;
    }
    return;
  }
  const double gamma = -0.691 + 10.0 * log10(sum / cnt) - 10.0;
  double sum2 = 0.0, cnt2 = 0.0;
  for (i64 i = threadIdx.x; i < nb; i += 256) {
    const double z = block_z(S, w, C, nseg, inv, i);
    const double l = -0.691 + 10.0 * log10(z);
    if (l > -70.0 && l > gamma) {
      sum2 += z;
      cnt2 += 1.0;
    }
  }
  sum2 = mg_block_sum_f64(sum2, red);
  cnt2 = mg_block_sum_f64(cnt2, red);
  if (threadIdx.x == 0) {
    record[0] = cnt2 > 0.0 ? -0.691 + 10.0 * log10(sum2 / cnt2) : ninf;
    record[1] = top;
    record[2] = cnt;
    record[3] = cnt2;
  }
}

// part[c * tiles + tile] = max over the tile's samples T of max(|x[T]|, |u[4 T + p]|, p < 4),
// u[4 T + p] = sum_j x[T - 7 + j] h[p][j] with x zero outside [0, L): the outputs 4 T .. 4 T + 3 of mg_resample_pcm(1 -> 4).
__global__ void __launch_bounds__(256) true_peak_k(const float* __restrict__ x, i64 row_stride, i64 L, const float* __restrict__ bank,
                                                   float* __restrict__ part) {
  __shared__ float xs[TP_TILE + TP_TAPS - 1];
  __shared__ float red[4];
  const int tid = threadIdx.x, c = blockIdx.y;
  const i64 t0 = (i64)blockIdx.x * TP_TILE;
  const float* __restrict__ xc = x + (i64)c * row_stride;
  for (int i = tid; i < TP_TILE + TP_TAPS - 1; i += 256) {
    const i64 s = t0 - TP_W + i;
    xs[i] = (s >= 0 && s < L) ? xc[s] : 0.f;
  }
  f32x2 h01[TP_TAPS], h23[TP_TAPS];  // phases 0 and 1, 2 and 3, side by side (uniform: scalar registers)
#pragma unroll
  for (int j = 0; j < TP_TAPS; ++j) {
    h01[j] = f32x2{bank[j], bank[TP_TAPS + j]};
    h23[j] = f32x2{bank[2 * TP_TAPS + j], bank[3 * TP_TAPS + j]};
  }
  __syncthreads();
  float m = 0.f;
  for (int i = tid; i < TP_TILE; i += 256) {
    if (t0 + i >= L) break;
    const float* w = xs + i;
    f32x2 a01 = f32x2{w[0], w[0]} * h01[0], a23 = f32x2{w[0], w[0]} * h23[0];
#pragma unroll
    for (int j = 1; j < TP_TAPS; ++j) {
      const f32x2 xv = f32x2{w[j], w[j]};
      a01 = __builtin_elementwise_fma(xv, h01[j], a01);
      a23 = __builtin_elementwise_fma(xv, h23[j], a23);
    }
    m = fmaxf(m, fabsf(w[TP_W]));
    m = fmaxf(fmaxf(m, fabsf(a01.x)), fabsf(a01.y));
    m = fmaxf(fmaxf(m, fabsf(a23.x)), fabsf(a23.y));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) part[(i64)c * gridDim.x + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void __launch_bounds__(256) true_peak_final_k(const float* __restrict__ part, i64 n, float* __restrict__ out) {
  __shared__ float red[4];
  float m = 0.f;
  for (i64 i = threadIdx.x; i < n; i += 256) m = fmaxf(m, part[i]);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// gain = min(10^((target - L_int) / 20), 10^(ceiling / 20) / peak) in float64, rounded once; 1 where L_int = -inf
__global__ void loud_gain_k(const double* __restrict__ record, const float* __restrict__ peak, double target, double ceiling,
                            float* __restrict__ gain) {
  const double l = record[0];
  double g = 1.0;
  if (l != -INFINITY) g = fmin(pow(10.0, (target - l) / 20.0), pow(10.0, ceiling / 20.0) / (double)peak[0]);
  gain[0] = (float)g;
}

__global__ void __launch_bounds__(256) loud_scale_k(const float* __restrict__ x, float* __restrict__ out, i64 n,
                                                    const float* __restrict__ gain) {
  const float g = gain[0];
  const i64 step = (i64)gridDim.x * 256;
  for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += step) out[i] = x[i] * g;
}

void mat_mul(const Mat4& a, const Mat4& b, Mat4* out) {
  Mat4 r;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = 0.0;
      for (int k = 0; k < 4; ++k) s += a.m[4 * i + k] * b.m[4 * k + j];
      r.m[4 * i + j] = s;
    }
  *out = r;
}

void mat_pow(Mat4 a, long long e, Mat4* out) {
  Mat4 r = {};
  for (int i = 0; i < 4; ++i) r.m[5 * i] = 1.0;
  for (; e > 0; e >>= 1) {
    if (e & 1) mat_mul(r, a, &r);
    mat_mul(a, a, &a);
  }
  *out = r;
}

// A^CHUNK: column j = the state CHUNK silent samples after the unit state e_j
void chunk_matrix(const Coef& kc, Mat4* out) {
  for (int j = 0; j < 4; ++j) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    v[j] = 1.0;
    for (int t = 0; t < CHUNK; ++t) kw_step(kc, v, 0.0);
    for (int i = 0; i < 4; ++i) out->m[4 * i + j] = v[i];
  }
}

size_t state_bytes(int C, i64 nch) { return (size_t)C * (size_t)nch * 4 * sizeof(double); }

bool plan(int C, i64 L, int seg, i64* nseg, i64* nch) {
  if (C < 1 || C > MAXC || L < 0 || seg < 1) return false;
  *nseg = L / seg;
  *nch = (*nseg * seg + CHUNK - 1) / CHUNK;
  return *nch < ((i64)1 << 31) - ROWS && *nseg < ((i64)1 << 40);
}

}  // namespace

extern "C" int mg_loudness_chunk(void) { return CHUNK; }

extern "C" size_t mg_loudness_ws_bytes(int C, int64_t L, int seg) {
  i64 nseg, nch;
  if (!plan(C, L, seg, &nseg, &nch)) return 0;
  return state_bytes(C, nch) + (size_t)C * (size_t)(nch + nseg) * sizeof(double) + 16;
}

extern "C" int mg_loudness_energy(const float* x, int C, int64_t L, int64_t row_stride, int seg, const double* coef, double* S, void* ws,
                                  size_t ws_bytes, mg_stream_t stream) {
  i64 nseg, nch;
  MG_CHECK_ARG(plan(C, L, seg, &nseg, &nch), "mg_loudness_energy: 1 .. %d channels, L >= 0 and seg >= 1 expected (got %d, %lld, %d)",
               MAXC, C, (long long)L, seg);
  MG_CHECK_ARG(coef && row_stride >= 0 && (C == 1 || row_stride >= L), "mg_loudness_energy: bad arguments");
  for (int i = 0; i < 10; ++i) MG_CHECK_ARG(std::isfinite(coef[i]), "mg_loudness_energy: coefficient %d is not finite", i);
  if (nseg == 0) return MG_OK;
  MG_CHECK_ARG(x && S && ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0 && reinterpret_cast<uintptr_t>(S) % 8 == 0,
               "mg_loudness_energy: null or misaligned pointer");
  if (ws_bytes < mg_loudness_ws_bytes(C, L, seg)) {
    mg_set_error("mg_loudness_energy: workspace too small");
    return MG_EWORKSPACE;
  }
  const Coef kc = {coef[0], coef[1], coef[2], coef[3], coef[4], coef[5], coef[6], coef[7], coef[8], coef[9]};
  const int per = (int)((nch + 255) / 256);
  Mat4 M, MP, MG;
  chunk_matrix(kc, &M);
  mat_pow(M, per, &MP);
  mat_pow(MP, 16, &MG);
  double* st = reinterpret_cast<double*>(ws);
  double* pieces = st + (size_t)C * (size_t)nch * 4;
  const i64 N = nseg * seg;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((nch + ROWS - 1) / ROWS), (unsigned)C);
  hipLaunchKernelGGL(loud_chunk_k<false>, grid, dim3(ROWS), 0, s, x, (i64)row_stride, N, (int)nch, seg, nseg, kc, st, pieces);
  MG_CHECK_LAUNCH("mg_loudness_energy(chunk states)");
  hipLaunchKernelGGL(loud_carry_k, dim3(C), dim3(256), 0, s, st, (int)nch, per, M, MP, MG);
  MG_CHECK_LAUNCH("mg_loudness_energy(carry)");
  hipLaunchKernelGGL(loud_chunk_k<true>, grid, dim3(ROWS), 0, s, x, (i64)row_stride, N, (int)nch, seg, nseg, kc, st, pieces);
  MG_CHECK_LAUNCH("mg_loudness_energy(energies)");
  hipLaunchKernelGGL(loud_segments_k, dim3((unsigned)((nseg + 255) / 256), (unsigned)C), dim3(256), 0, s, pieces, S, (int)nch, seg, nseg);
  MG_CHECK_LAUNCH("mg_loudness_energy(segments)");
  return MG_OK;
}

extern "C" int mg_loudness_gate(const double* S, const double* weights, int C, int64_t nseg, int seg, double* record,
                                mg_stream_t stream) {
  MG_CHECK_ARG(C >= 1 && C <= MAXC && nseg >= 0 && seg >= 1 && weights && record && (S || nseg == 0),
               "mg_loudness_gate: bad arguments");
  Weights w = {};
  for (int c = 0; c < C; ++c) {
    MG_CHECK_ARG(std::isfinite(weights[c]) && weights[c] >= 0.0, "mg_loudness_gate: weight %d must be finite and not negative", c);
    w.g[c] = weights[c];
  }
  hipLaunchKernelGGL(loud_gate_k, dim3(1), dim3(256), 0, (hipStream_t)stream, S, w, C, (i64)nseg, seg, record);
  MG_CHECK_LAUNCH("mg_loudness_gate");
  return MG_OK;
}

extern "C" size_t mg_true_peak_ws_bytes(int C, int64_t L) {
  if (C < 1 || C > MAXC || L < 1) return 0;
  return (size_t)C * (size_t)((L + TP_TILE - 1) / TP_TILE) * sizeof(float);
}

extern "C" int mg_true_peak(const float* x, int C, int64_t L, int64_t row_stride, const void* bank, size_t bank_bytes, float* peak,
                            void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(x && bank && peak && ws && C >= 1 && C <= MAXC && L >= 1 && row_stride >= 0 && (C == 1 || row_stride >= L),
               "mg_true_peak: bad arguments");
  int phases = 0, taps = 0;
  const size_t need = mg_resample_bank_size(1, 4, 6, 0.99, &phases, &taps);
  MG_CHECK_ARG(phases == TP_PHASES && taps == TP_TAPS && bank_bytes >= need,
               "mg_true_peak: the bank of mg_resample_bank(1, 4, 6, 0.99) expected (%zu bytes, 4 x 15 taps)", need);
  const i64 tiles = (L + TP_TILE - 1) / TP_TILE;
  MG_CHECK_ARG(tiles < ((i64)1 << 31), "mg_true_peak: too many samples");
  if (ws_bytes < mg_true_peak_ws_bytes(C, L)) {
    mg_set_error("mg_true_peak: workspace too small");
    return MG_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  float* part = reinterpret_cast<float*>(ws);
  hipLaunchKernelGGL(true_peak_k, dim3((unsigned)tiles, (unsigned)C), dim3(256), 0, s, x, (i64)row_stride, (i64)L,
                     reinterpret_cast<const float*>(bank), part);
  MG_CHECK_LAUNCH("mg_true_peak(tiles)");
  hipLaunchKernelGGL(true_peak_final_k, dim3(1), dim3(256), 0, s, part, tiles * C, peak);
  MG_CHECK_LAUNCH("mg_true_peak(final)");
  return MG_OK;
}

extern "C" int mg_loudness_normalize(const float* x, float* out, int64_t n, const double* record, const float* peak, double target,
                                     double ceiling, float* gain, mg_stream_t stream) {
  MG_CHECK_ARG(record && peak && gain && n >= 0 && ((x && out) || n == 0), "mg_loudness_normalize: bad arguments");
  MG_CHECK_ARG(std::isfinite(target) && std::isfinite(ceiling), "mg_loudness_normalize: target and ceiling must be finite");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(loud_gain_k, dim3(1), dim3(1), 0, s, record, peak, target, ceiling, gain);
  MG_CHECK_LAUNCH("mg_loudness_normalize(gain)");
  if (n == 0) return MG_OK;
  i64 blocks = (n + 1023) / 1024;  // four elements per thread
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(loud_scale_k, dim3((unsigned)blocks), dim3(256), 0, s, x, out, (i64)n, gain);
  MG_CHECK_LAUNCH("mg_loudness_normalize(scale)");
  return MG_OK;
}
