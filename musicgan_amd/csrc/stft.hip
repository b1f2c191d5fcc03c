// Framed, Hann-windowed 1024-point real FFT (the STFT of /root/reference/music_gan/audio/functions.py:38-62):
//   X[k,t] = 1/sqrt(sum w^2) * sum_{n<1024} w[n] xpad[256 t + n] e^{-2 pi i k n / 1024},  k = 0..511 (Nyquist dropped),
//   xpad = reflect-pad(x, 512), w = periodic Hann, T = 1 + L/256.
//
// One wave transforms one frame: the 1024 real samples are packed as 512 complex points (8 per lane), three radix-8
// Stockham passes (two exchanges through a per-wave 4 KiB LDS buffer) leave Z[j + 64 r] in lane j / register r; the
// real-FFT untangling needs Z[512-k], which lives in lane (64-j)&63 -> one wavefront shuffle per value, no LDS.
// A workgroup (8 waves, persistent: one per CU) covers 16 consecutive frames per tile and transposes its 512x16 output tile
// through LDS so that global stores are 128-byte runs along t (the output is frequency-major).  Twiddles and the window are
// built once per workgroup into LDS with sincospi (no global tables, no hidden state).
#include <cmath>

#include "fft512.h"
#include "fft_radix2.h"
#include "mg_common.h"
#include "stft_frame.h"

namespace {

constexpr int FPB = NWAVE * FPW;  // frames per tile: 8 x 8 bytes = one 64-byte run per bin row
constexpr size_t STFT_LDS = (size_t)(TW_FLOATS + NFFT + FPB * XSTR * 2) * sizeof(float);

// Persistent workgroups of 8 waves (two per CU: one's write-out runs under the other's FFTs; <= 128 registers): twiddles and window are built once
// per workgroup, then each tile of 16 consecutive frames is transformed -- one wave = 2 frames, each in its own 4 KiB LDS column
// that serves the two Stockham exchanges and finally holds the frame's 512 output bins, so there is no workgroup barrier inside
// a frame -- and the 16 columns are read out transposed so that every global store instruction writes four 128-byte runs along t.
// PcmSrc<PCM, CH> (stft_frame.h): the file's bytes go to the GPU as they are, int16 or float32, mono or interleaved stereo.
template <int PCM, int CH>
__global__ void __launch_bounds__(64 * NWAVE, 2) stft1024_kernel(const void* __restrict__ wav, float* __restrict__ out_re,
                                                              float* __restrict__ out_im, long long L, int T, int ntiles) {
  using Src = PcmSrc<PCM, CH>;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  c2* tw = reinterpret_cast<c2*>(smem);                       // tw[k], k < 512
  c2* tw1 = tw + NB;                                           // tw1[r * 8 + k]
  c2* tw2 = tw1 + 64;                                          // tw2[r * 64 + j]
  float* win = smem + TW_FLOATS;                               // Hann / sqrt(sum w^2)
  c2* xbuf = reinterpret_cast<c2*>(win + NFFT);                // [FPB][XSTR] one column per frame of the tile

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int m = tid; m < NFFT; m += 64 * NWAVE) {
    const float c = fft512_fill_tables(tw, tw1, tw2, m);
    win[m] = stft_window_entry(c);
  }
  __syncthreads();

  // Samples of a frame, 8 complex pairs per lane: requested one frame ahead (the next frame of the tile, or the first frame
  // of the workgroup's next tile before the write-out of this one), so the HBM latency runs under a whole frame of FFT work
  // instead of in front of it (a wave has nothing else to do: 4 waves per SIMD do not hide ~2500 cycles).
  auto load_frame = [&](int t, c2 (&x)[8]) { stft_load_frame<Src>(wav, L, T, t, lane, true, x); };

  c2 xn[8];  // the frame in flight
  if ((int)blockIdx.x < ntiles) load_frame(blockIdx.x * FPB + wave * FPW, xn);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int t0 = tile * FPB;
#pragma unroll 1
    for (int f = 0; f < FPW; ++f) {
      const int fl = wave * FPW + f;  // frame slot in the tile
      c2* xb = xbuf + fl * XSTR;
      c2 v[8];
      stft_apply_window(xn, win, lane, v);
      {  // one call site: next frame of this tile, first frame of the next tile, or nothing (t = T reads as zeros)
        const int tnext = tile + (int)gridDim.x < ntiles ? (tile + (int)gridDim.x) * FPB + wave * FPW : T;
        load_frame(f + 1 < FPW ? t0 + fl + 1 : tnext, xn);
      }
      fft512_wave(v, xb, tw1, tw2, lane);
      stft_untangle(v, xb, tw, lane);  // the frame's 512 bins, left in its column
    }
    __syncthreads();
    // transposed write-out: the 16 frames of one bin row per 8 lanes, two frames (16 bytes) per lane -- stores are issue-bound per
    // instruction, so half as many twice as wide; a store instruction writes eight 128-byte runs along t.  Non-temporal stores:
    // the bins are written once and not read back by this kernel, and keeping them out of the L2's way is worth 6-8 %
    // (0.146-0.166 -> 0.136-0.152 ms per 10-minute file, same box, alternating libraries)
    {
      const int fp = tid & (FPB / 2 - 1);  // frame pair
      const int t = t0 + 2 * fp;
      if (out_im == nullptr && (T & 1) == 0) {  // interleaved complex output, rows 16-byte aligned
        if (t < T) {  // T even: t + 1 < T too
#pragma unroll 8
          for (int k = tid / (FPB / 2); k < NB; k += 64 * NWAVE / (FPB / 2)) {
            const c2 o0 = lds_c2(xbuf + (2 * fp) * XSTR + k), o1 = lds_c2(xbuf + (2 * fp + 1) * XSTR + k);
            __builtin_nontemporal_store(f32x4{o0.x, o0.y, o1.x, o1.y}, reinterpret_cast<f32x4*>(out_re + 2 * ((size_t)k * T + t)));
          }
        }
      } else {
        const int f = tid & (FPB - 1);
        const int tt = t0 + f;
        if (tt < T) {
#pragma unroll 4
          for (int k = tid / FPB; k < NB; k += 64 * NWAVE / FPB) {
            const c2 o = xbuf[f * XSTR + k];
            const size_t idx = (size_t)k * T + tt;
            if (out_im != nullptr) {
              __builtin_nontemporal_store(o.x, out_re + idx);
              __builtin_nontemporal_store(o.y, out_im + idx);
            } else {
              __builtin_nontemporal_store(o, reinterpret_cast<c2*>(out_re + 2 * idx));
            }
          }
        }
      }
    }
    __syncthreads();
  }
}

// Other sample formats / channel counts: one pass to mono float32 first (rare: 8-bit, 32-bit integer, more than two channels).
__global__ void __launch_bounds__(256) pcm_to_mono_k(const void* __restrict__ pcm, float* __restrict__ mono, long long L, int C, int kind) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < L; i += (long long)gridDim.x * 256) mono[i] = mg_pcm_mono(pcm, i, C, kind);
}

template <int PCM, int CH>
static int launch_stft(const void* wav, float* out_re, float* out_im, long long L, hipStream_t stream) {
  const int T = (int)(L / HOP) + 1;
  const int ntiles = (T + FPB - 1) / FPB;
  const int n_cu = mg_cu_count();
  static MgPerDevice once;
  if (mg_first_use_on_device(once))
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&stft1024_kernel<PCM, CH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
  const int blocks = ntiles < 2 * n_cu ? ntiles : 2 * n_cu;  // two 78 KB workgroups per CU, persistent over the tiles
  hipLaunchKernelGGL((stft1024_kernel<PCM, CH>), dim3(blocks), dim3(64 * NWAVE), STFT_LDS, stream, wav, out_re, out_im, L, T, ntiles);
  MG_CHECK_LAUNCH("mg_stft_1024");
  return MG_OK;
}

// Any other (n_fft, hop) the reference's signature admits (functions.py:38-41: wav_to_stft(wav_p, nperseg, stride)): a plain
// radix-2 transform in LDS, one frame per workgroup -- not a tuned path (the drivers only ever use 1024 / 256), same definition:
// periodic Hann, centre reflect padding of n_fft / 2, division by sqrt(sum w^2), bins 0 .. n_fft/2 - 1.
__global__ void __launch_bounds__(256) stft_generic_k(const float* __restrict__ wav, float* __restrict__ out, long long L, int T, int N,
                                                      int lgN, int hop, float inv_norm) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float2* buf = reinterpret_cast<float2*>(smem);
  const int t = blockIdx.x;
  const long long base = (long long)t * hop - N / 2;
  for (int n = threadIdx.x; n < N; n += 256) {
    long long s = base + n;
    if (s < 0) s = -s;
    if (s >= L) s = 2 * (L - 1) - s;
    float sn, cs;
    sincospif(2.0f * (float)n / (float)N, &sn, &cs);
    const float w = (0.5f - 0.5f * cs) * inv_norm;
    // bit-reversed placement: the stages below are decimation in time
    buf[__brev((unsigned)n) >> (32 - lgN)] = make_float2(wav[s] * w, 0.f);
  }
  __syncthreads();
  fft_radix2_lds(buf, lgN, threadIdx.x, 256, TwForward{});
  for (int k = threadIdx.x; k < N / 2; k += 256) *reinterpret_cast<float2*>(out + 2 * ((size_t)k * T + t)) = buf[k];
}

}  // namespace

extern "C" int mg_pcm_to_mono(const void* pcm, int kind, int channels, float* mono, int64_t L, mg_stream_t stream) {
  MG_CHECK_ARG(pcm && mono && L > 0 && channels >= 1 && channels <= 64 && kind >= MG_PCM_F32 && kind <= MG_PCM_U8,
               "mg_pcm_to_mono: bad arguments");
  const long long nb = (L + 255) / 256;
  hipLaunchKernelGGL(pcm_to_mono_k, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, (hipStream_t)stream, pcm, mono,
                     (long long)L, channels, kind);
  MG_CHECK_LAUNCH("mg_pcm_to_mono");
  return MG_OK;
}

extern "C" int mg_stft_generic(const float* wav, float* out_c64, int64_t L, int n_fft, int hop, mg_stream_t stream) {
  MG_CHECK_ARG(wav && out_c64 && hop >= 1, "mg_stft_generic: bad arguments");
  MG_CHECK_ARG(n_fft >= 64 && n_fft <= 8192 && (n_fft & (n_fft - 1)) == 0, "mg_stft_generic: n_fft=%d is not a power of two in [64, 8192]",
               n_fft);
  MG_CHECK_ARG(L > n_fft / 2, "mg_stft_generic: reflect padding needs L > n_fft / 2 (got %lld)", (long long)L);
  MG_CHECK_ARG(L / hop + 1 < (1ll << 30), "mg_stft_generic: too many frames");
  const int T = (int)(L / hop) + 1;
  // periodic Hann: sum w^2 = 3 N / 8
  const float inv_norm = (float)(1.0 / sqrt(0.375 * (double)n_fft));
  hipLaunchKernelGGL(stft_generic_k, dim3((unsigned)T), dim3(256), (size_t)n_fft * sizeof(c2), (hipStream_t)stream, wav, out_c64,
                     (long long)L, T, n_fft, mg_ilog2(n_fft), hop, inv_norm);
  MG_CHECK_LAUNCH("mg_stft_generic");
  return MG_OK;
}

extern "C" int mg_stft_1024(const float* wav, float* out_re, float* out_im, int64_t L, mg_stream_t stream) {
  MG_CHECK_ARG(wav && out_re, "mg_stft_1024: bad arguments");
  MG_CHECK_ARG(L > NFFT / 2, "mg_stft_1024: reflect padding needs L > 512 (got %lld)", (long long)L);
  MG_CHECK_ARG(L / HOP + 1 < (1ll << 30), "mg_stft_1024: too many frames");
  return launch_stft<0, 1>(wav, out_re, out_im, (long long)L, (hipStream_t)stream);
}

extern "C" size_t mg_stft_1024_pcm_ws_bytes(int64_t L, int channels, int kind) {
  const bool direct = (kind == MG_PCM_F32 || kind == MG_PCM_I16) && (channels == 1 || channels == 2);
  return direct ? 0 : (size_t)L * sizeof(float);
}

extern "C" int mg_stft_1024_pcm(const void* pcm, int kind, int channels, float* out_re, float* out_im, void* ws, size_t ws_bytes,
                                int64_t L, mg_stream_t stream) {
  MG_CHECK_ARG(pcm && out_re && channels >= 1 && channels <= 64 && kind >= MG_PCM_F32 && kind <= MG_PCM_U8,
               "mg_stft_1024_pcm: bad arguments");
  MG_CHECK_ARG(L > NFFT / 2, "mg_stft_1024_pcm: reflect padding needs L > 512 (got %lld)", (long long)L);
  MG_CHECK_ARG(L / HOP + 1 < (1ll << 30), "mg_stft_1024_pcm: too many frames");
  hipStream_t s = (hipStream_t)stream;
  if (kind == MG_PCM_F32 && channels == 1) return launch_stft<0, 1>(pcm, out_re, out_im, (long long)L, s);
  if (kind == MG_PCM_F32 && channels == 2) return launch_stft<0, 2>(pcm, out_re, out_im, (long long)L, s);
  if (kind == MG_PCM_I16 && channels == 1) return launch_stft<1, 1>(pcm, out_re, out_im, (long long)L, s);
  if (kind == MG_PCM_I16 && channels == 2) return launch_stft<1, 2>(pcm, out_re, out_im, (long long)L, s);
  if (ws == nullptr || ws_bytes < (size_t)L * sizeof(float)) {
    mg_set_error("mg_stft_1024_pcm: workspace of %zu bytes needed", (size_t)L * sizeof(float));
    return MG_EWORKSPACE;
  }
  const long long nb = (L + 255) / 256;
  hipLaunchKernelGGL(pcm_to_mono_k, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, pcm, reinterpret_cast<float*>(ws),
                     (long long)L, channels, kind);
  MG_CHECK_LAUNCH("mg_stft_1024_pcm(mono)");
  return launch_stft<0, 1>(ws, out_re, out_im, (long long)L, s);
}
