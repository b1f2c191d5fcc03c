// Polyphase resampling of PCM frames: torchaudio.functional.resample(x, orig, new) with its defaults (sinc_interp_hann,
// lowpass_filter_width 6, rolloff 0.99), what a user of the reference calls in front of wav_to_stft for a file that is not at
// 44.1 kHz (the reference's audio/functions.py:45 accepts no other rate).
//
// torchaudio's kernel, with o / n = orig / new reduced by their gcd, base = min(o, n) * rolloff, w = ceil(lpw * o / base):
//   h_p[k] = sinc(t) * cos^2(pi t / (2 lpw)) * base / o,  t = clamp(base * (k - w) / o - base * p / n, +-lpw),  k < 2w + o,
//   y[T n + p] = sum_k xpad[T o + k] h_p[k],  xpad = x zero-padded by (w, w + o),  truncated to ceil(n L / o) outputs.
// Every tap of row p with |t| = lpw after the clamp is the same number, sinc(lpw) * cos^2(pi / 2) * base / o (~1e-49): a rounding
// of zero.  The others lie in k = c_p .. c_p + 2w with c_p = floor(o p / n) (|k - w - o p / n| < lpw * o / base <= w), so the bank
// keeps 2w + 1 taps per phase from that start: output m reads x[floor(o m / n) - w + j], j <= 2w.  orig == new: one unit tap.
//
// The kernel is bound by HBM traffic (a 10-minute 48 kHz stereo int16 file: 115 MB in, 106 MB out; 0.4 G FMAs).  A workgroup owns Q
// whole periods of n outputs, stages their input span (Q o + 2w samples) in LDS once -- converted to mono float32 on the way in
// by the loader mg_pcm_to_mono uses -- and every thread keeps ONE phase's taps in registers while it walks the periods of its
// group: 2w + 1 LDS reads and FMAs per output, lanes on consecutive phases read consecutive samples.
#include <cmath>

#include "mg_common.h"

namespace {

constexpr int BMAX = 512;          // threads per workgroup at most
constexpr int OUT_PER_THREAD = 8;  // outputs per thread and tile (the staged span is read by this many FMA chains per sample)
constexpr int SPAN_MAX = 12288;    // staged samples per workgroup at most (48 KB of LDS)
constexpr int LOADS = 8;           // staged samples per thread in flight (the span is ~8.6 samples per thread at 48 -> 44.1 kHz)

struct Plan {
  int o, n, w, taps;
};

long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

bool make_plan(int orig_freq, int new_freq, int lpw, double rolloff, Plan* pl) {
  if (orig_freq <= 0 || new_freq <= 0 || lpw <= 0 || !(rolloff > 0.0) || !std::isfinite(rolloff)) return false;
  const long long g = gcd_ll(orig_freq, new_freq);
  pl->o = (int)(orig_freq / g);
  pl->n = (int)(new_freq / g);
  if (pl->o == pl->n) {
    pl->w = 0;
    pl->taps = 1;
    return true;
  }
  const double base = (double)(pl->o < pl->n ? pl->o : pl->n) * rolloff;
  const double wd = std::ceil((double)lpw * (double)pl->o / base);
  if (!(wd < (double)(1 << 24))) return false;
  pl->w = (int)wd;
  pl->taps = 2 * pl->w + 1;
  return true;
}

// NT >= taps: the phase's taps live in NT registers (16 / 32 / 64); NT == 0: any tap count, each tap read from the bank per output.
// Same tap order either way: acc = x_0 h_0, then acc = fma(x_j, h_j, acc) for j = 1 .. taps - 1.  KIND / CH: the PCM format fixed
// at compile time (-1 / 0: read from the arguments), see mg_pcm_mono_t.
template <int NT, int KIND, int CH>
__global__ void __launch_bounds__(BMAX) resample_k(const void* __restrict__ pcm, int kind, int C, long long row_stride, int rows,
                                                   long long L, const float* __restrict__ bank, const int* __restrict__ start, int o,
                                                   int n, int w, int nt, int Q, int G, float* __restrict__ out, long long Lout) {
  extern __shared__ float xs[];  // input samples T0 o - w .. (T0 + Q) o + w - 1
  const int S = Q * o + 2 * w;
  const int tid = threadIdx.x;
  const long long T0 = (long long)blockIdx.x * Q;
  const long long s0 = T0 * o - w;
  for (int r = blockIdx.y; r < rows; r += gridDim.y) {
    const long long row0 = (long long)r * row_stride;
    // LOADS samples per thread requested before the first is stored: one HBM latency per batch instead of one per sample
    for (int k0 = tid; k0 < S; k0 += LOADS * blockDim.x) {
      float v[LOADS];
#pragma unroll
      for (int u = 0; u < LOADS; ++u) {
        const long long s = s0 + k0 + u * (int)blockDim.x;
        const long long sc = s < 0 ? 0 : (s >= L ? L - 1 : s);  // (a valid address; the value is dropped)
        const float x = mg_pcm_mono_t<KIND, CH>(pcm, row0 + sc, C, kind);
        v[u] = (s >= 0 && s < L) ? x : 0.f;  // outside [0, L): torchaudio's zero padding
      }
#pragma unroll
      for (int u = 0; u < LOADS; ++u)
        if (k0 + u * (int)blockDim.x < S) xs[k0 + u * blockDim.x] = v[u];
    }
    __syncthreads();
    float* __restrict__ y = out + (long long)r * Lout;
    // thread tid < n G: phase tid % n, group tid / n of the G that share a phase (n <= blockDim); n > blockDim: G = 1, the phases
    // tid, tid + blockDim, ...
    if (tid < n * G) {
      for (int p = tid % n; p < n; p += blockDim.x) {
        const float* __restrict__ hp = bank + (size_t)p * nt;
        const int st = start[p];
        float h[NT > 0 ? NT : 1];
        if constexpr (NT > 0) {
#pragma unroll
          for (int j = 0; j < NT; ++j) h[j] = j < nt ? hp[j] : 0.f;
        }
        for (int q = tid / n; q < Q; q += G) {
          const long long m = (T0 + q) * n + p;
          if (m >= Lout) break;
          const float* x = xs + q * o + st;
          float acc;
          if constexpr (NT > 0) {
            acc = x[0] * h[0];
#pragma unroll
            for (int j = 1; j < NT; ++j)
              if (j < nt) acc = fmaf(x[j], h[j], acc);
          } else {
            acc = x[0] * hp[0];
            for (int j = 1; j < nt; ++j) acc = fmaf(x[j], hp[j], acc);
          }
          y[m] = acc;
        }
      }
    }
    __syncthreads();
  }
}

template <int NT, int KIND, int CH>
void launch_k(dim3 grid, int block, size_t lds, hipStream_t s, const void* pcm, int kind, int C, long long row_stride, int rows,
              long long L, const float* taps, const int* start, const Plan& pl, int Q, int G, float* out, long long Lout) {
  hipLaunchKernelGGL((resample_k<NT, KIND, CH>), grid, dim3(block), lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl.o,
                     pl.n, pl.w, pl.taps, Q, G, out, Lout);
}

// the formats of real files get their loads specialised: float32 / int16 with one or two channels; the rest reads kind and channels
template <int NT>
void launch(dim3 grid, int block, size_t lds, hipStream_t s, const void* pcm, int kind, int C, long long row_stride, int rows,
            long long L, const float* taps, const int* start, const Plan& pl, int Q, int G, float* out, long long Lout) {
  if (kind == MG_PCM_F32 && C == 1)
    launch_k<NT, MG_PCM_F32, 1>(grid, block, lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else if (kind == MG_PCM_F32 && C == 2)
    launch_k<NT, MG_PCM_F32, 2>(grid, block, lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else if (kind == MG_PCM_I16 && C == 1)
    launch_k<NT, MG_PCM_I16, 1>(grid, block, lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else if (kind == MG_PCM_I16 && C == 2)
    launch_k<NT, MG_PCM_I16, 2>(grid, block, lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else
    launch_k<NT, -1, 0>(grid, block, lds, s, pcm, kind, C, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
}

}  // namespace

extern "C" int64_t mg_resample_len(int64_t L, int orig_freq, int new_freq) {
  if (L < 0 || orig_freq <= 0 || new_freq <= 0) return -1;
  const long long g = gcd_ll(orig_freq, new_freq);
  const unsigned __int128 o = (unsigned)(orig_freq / g), n = (unsigned)(new_freq / g);
  const unsigned __int128 len = (n * (unsigned __int128)L + o - 1) / o;  // ceil(n L / o)
  return len > (unsigned __int128)INT64_MAX ? -1 : (int64_t)len;
}

extern "C" size_t mg_resample_bank_size(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, int* phases,
                                        int* taps) {
  Plan pl;
  if (!make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &pl)) return 0;
  if (phases) *phases = pl.n;
  if (taps) *taps = pl.taps;
  return (size_t)pl.n * (size_t)(pl.taps + 1) * 4;
}

extern "C" int mg_resample_bank(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, void* bank, size_t bank_bytes) {
  Plan pl;
  MG_CHECK_ARG(make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &pl),
               "mg_resample_bank: bad arguments (rates %d -> %d, lowpass_filter_width %d, rolloff %g)", orig_freq, new_freq,
               lowpass_filter_width, rolloff);
  const size_t need = (size_t)pl.n * (size_t)(pl.taps + 1) * 4;
  MG_CHECK_ARG(bank && bank_bytes >= need, "mg_resample_bank: %zu bytes needed", need);
  float* h = reinterpret_cast<float*>(bank);
  int32_t* start = reinterpret_cast<int32_t*>(h + (size_t)pl.n * pl.taps);
  if (pl.o == pl.n) {
    h[0] = 1.0f;
    start[0] = 0;
    return MG_OK;
  }
  // torchaudio's _get_sinc_resample_kernel, its order of operations, in float64; rounded once to float32
  const double lpw = (double)lowpass_filter_width;
  const double base = (double)(pl.o < pl.n ? pl.o : pl.n) * rolloff;
  const double scale = base / (double)pl.o;
  const double pi = 3.14159265358979323846;
  for (int p = 0; p < pl.n; ++p) {
    const int c = (int)((long long)pl.o * p / pl.n);  // floor(o p / n)
    start[p] = c;
    for (int j = 0; j < pl.taps; ++j) {
      const int k = c + j;
      double t = ((double)(-p) / (double)pl.n + (double)(k - pl.w) / (double)pl.o) * base;
      t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
      const double cw = std::cos(t * pi / lpw / 2.0);
      const double win = cw * cw;
      t *= pi;
      const double s = t == 0.0 ? 1.0 : std::sin(t) / t;
      h[(size_t)p * pl.taps + j] = (float)(s * (win * scale));
    }
  }
  return MG_OK;
}

extern "C" int mg_resample_pcm(const void* pcm, int kind, int channels, int rows, int64_t row_stride, int64_t L, int orig_freq,
                               int new_freq, int lowpass_filter_width, double rolloff, const void* bank, size_t bank_bytes, float* out,
                               mg_stream_t stream) {
  Plan pl;
  MG_CHECK_ARG(make_plan(orig_freq, new_freq, lowpass_filter_width, rolloff, &pl),
               "mg_resample_pcm: bad arguments (rates %d -> %d, lowpass_filter_width %d, rolloff %g)", orig_freq, new_freq,
               lowpass_filter_width, rolloff);
  MG_CHECK_ARG(pcm && out && bank && L > 0 && rows >= 1 && row_stride >= 0 && channels >= 1 && channels <= 64 &&
                   kind >= MG_PCM_F32 && kind <= MG_PCM_U8,
               "mg_resample_pcm: bad arguments");
  const size_t need = (size_t)pl.n * (size_t)(pl.taps + 1) * 4;
  MG_CHECK_ARG(bank_bytes >= need, "mg_resample_pcm: the bank of these rates has %zu bytes (mg_resample_bank_size), got %zu", need,
               bank_bytes);
  MG_CHECK_ARG((long long)pl.o + 2ll * pl.w <= SPAN_MAX,
               "mg_resample_pcm: %d -> %d Hz needs %lld staged samples per period (at most %d): ratio too extreme", orig_freq,
               new_freq, (long long)pl.o + 2ll * pl.w, SPAN_MAX);
  const long long Lout = mg_resample_len(L, orig_freq, new_freq);
  MG_CHECK_ARG(Lout > 0, "mg_resample_pcm: output length overflows");
  const int G = pl.n <= BMAX ? BMAX / pl.n : 1;  // threads per phase
  const int block = pl.n <= BMAX ? (pl.n * G + 63) / 64 * 64 : BMAX;
  int Q = G * OUT_PER_THREAD;  // periods per workgroup
  const int qmax = (SPAN_MAX - 2 * pl.w) / pl.o;
  if (Q > qmax) Q = qmax;
  const long long periods = (Lout + pl.n - 1) / pl.n;
  const long long tiles = (periods + Q - 1) / Q;
  MG_CHECK_ARG(tiles < (1ll << 31), "mg_resample_pcm: too many outputs");
  const dim3 grid((unsigned)tiles, (unsigned)(rows < 65535 ? rows : 65535));
  const size_t lds = (size_t)(Q * pl.o + 2 * pl.w) * sizeof(float);
  const float* taps = reinterpret_cast<const float*>(bank);
  const int* start = reinterpret_cast<const int*>(taps + (size_t)pl.n * pl.taps);
  hipStream_t s = (hipStream_t)stream;
  if (pl.taps <= 16) launch<16>(grid, block, lds, s, pcm, kind, channels, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else if (pl.taps <= 32) launch<32>(grid, block, lds, s, pcm, kind, channels, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else if (pl.taps <= 64) launch<64>(grid, block, lds, s, pcm, kind, channels, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  else launch<0>(grid, block, lds, s, pcm, kind, channels, row_stride, rows, L, taps, start, pl, Q, G, out, Lout);
  MG_CHECK_LAUNCH("mg_resample_pcm");
  return MG_OK;
}
