// One frame of the 1024 / 256 STFT, shared by the kernels that transform one frame per wave (stft.hip writes the bins out,
// melspec.hip sums their power over mel bands): where a frame's samples come from (PcmSrc), the reflect-padded load of 8 complex
// pairs per lane, the window table, and the real-FFT untangling that leaves the frame's 512 bins in the wave's own LDS column.
// Both kernels run this one copy, so their bins hold the same bits.
#pragma once
#include "fft512.h"

namespace {

// PCM: what `wav` holds -- 0: float32 samples, 1: int16 (scaled by 1/32768 as torchaudio.load(normalize=True) does);  CH: 1 = mono,
// 2 = interleaved stereo frames as a WAV file stores them, averaged on the way in (functions.py:49: raw_audio.mean(0)) -- a
// file's bytes go to the GPU as they are and the de-interleave / scale / mono mean cost no pass of their own.
template <int PCM, int CH>
struct PcmSrc {
  // two consecutive mono samples s, s + 1 (s even: aligned loads of 4 .. 16 bytes)
  static __device__ __forceinline__ c2 pair(const void* __restrict__ w, long long s) {
    if constexpr (PCM == 0 && CH == 1) {
      return *reinterpret_cast<const c2*>(reinterpret_cast<const float*>(w) + s);
    } else if constexpr (PCM == 0) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(w) + 2 * s);
      return c2{(v[0] + v[1]) / 2.0f, (v[2] + v[3]) / 2.0f};
    } else if constexpr (CH == 1) {
      const short2 v = *reinterpret_cast<const short2*>(reinterpret_cast<const short*>(w) + s);
      return c2{(float)v.x / 32768.0f, (float)v.y / 32768.0f};
    } else {
      const short4 v = *reinterpret_cast<const short4*>(reinterpret_cast<const short*>(w) + 2 * s);
      return c2{((float)v.x / 32768.0f + (float)v.y / 32768.0f) / 2.0f, ((float)v.z / 32768.0f + (float)v.w / 32768.0f) / 2.0f};
    }
  }
  static __device__ __forceinline__ float one(const void* __restrict__ w, long long s) {
    if constexpr (PCM == 0 && CH == 1) {
      return reinterpret_cast<const float*>(w)[s];
    } else if constexpr (PCM == 0) {
      const float2 v = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(w) + 2 * s);
      return (v.x + v.y) / 2.0f;
    } else if constexpr (CH == 1) {
      return (float)reinterpret_cast<const short*>(w)[s] / 32768.0f;
    } else {
      const short2 v = *reinterpret_cast<const short2*>(reinterpret_cast<const short*>(w) + 2 * s);
      return ((float)v.x / 32768.0f + (float)v.y / 32768.0f) / 2.0f;
    }
  }
};

// Entry m of the window table from cos(2 pi m / 1024) (what fft512_fill_tables returns): Hann / sqrt(384) (sum of hann^2 over 1024
// = 384), times the 1/2 of the real-FFT untangling: a power-of-two scale commutes exactly with every rounding of the (linear)
// transform, so it costs nothing here instead of 16 multiplies there
__device__ __forceinline__ float stft_window_entry(float c) { return (0.5f - 0.5f * c) * (0.5f * 0.05103103630798288f); }

// Samples of frame t of a signal of L samples, 8 complex pairs per lane: x[r] = (xpad[256 t + n], xpad[256 t + n + 1]) with
// n = 2 (lane + 64 r) and xpad = reflect-pad(x, 512).  t >= T reads as zeros.  `paired`: the samples start at an 8-byte boundary
// (interior frames then take one aligned load per pair); every index stays inside [0, L) either way.
template <class Src>
__device__ __forceinline__ void stft_load_frame(const void* __restrict__ wav, long long L, int T, int t, int lane, bool paired,
                                                c2 (&x)[8]) {
  if (t < T) {
    const long long base = (long long)t * HOP - NFFT / 2;  // sample index of padded position 0 of this frame
    const bool interior = paired && (base >= 0) && (base + NFFT <= L);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int n = 2 * (lane + 64 * r);
      if (interior) {
        x[r] = Src::pair(wav, base + n);
      } else {
        long long s0 = base + n, s1 = base + n + 1;
        if (s0 < 0) s0 = -s0;
        if (s1 < 0) s1 = -s1;
        if (s0 >= L) s0 = 2 * (L - 1) - s0;
        if (s1 >= L) s1 = 2 * (L - 1) - s1;
        x[r] = c2{Src::one(wav, s0), Src::one(wav, s1)};
      }
    }
  } else {
#pragma unroll
    for (int r = 0; r < 8; ++r) x[r] = c2{0.f, 0.f};
  }
}

// v = x * window, pair by pair
__device__ __forceinline__ void stft_apply_window(const c2 (&x)[8], const float* win, int lane, c2 (&v)[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = x[r] * lds_c2(reinterpret_cast<const c2*>(win + 2 * (lane + 64 * r)));
}

// From Z = fft512_wave(v) to the frame's bins, left in the wave's column: xb[k] = X[k], k = lane + 64 r.
//   X[k] = (Z[k] + conj Z[512-k])/2 - i/2 * e^{-2 pi i k/1024} * (Z[k] - conj Z[512-k]).
// Z[512-k] sits in lane (64-lane)&63, register 7-r (lane != 0) or 8-r (lane == 0; r == 0 -> Z[0] itself).
__device__ __forceinline__ void stft_untangle(const c2 (&v)[8], c2* xb, const c2* tw, int lane) {
  const int src = (64 - lane) & 63;
  c2 zc[8];  // Z[512-k]
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    // value this lane must SEND for the receiver's register r: receiver lane l' = (64-lane)&63 wants register
    // (l' == 0 ? 8-r : 7-r) of its source lane; every lane != 0 is read by a lane != 0 (7-r); lane 0 reads itself.
    const c2 send_n0 = v[7 - r];
    const c2 send_0 = v[(8 - r) & 7];
    const c2 send = (lane == 0) ? send_0 : send_n0;
    zc[r] = c2{__shfl(send.x, src), __shfl(send.y, src)};  // Z[512-k] (conjugated by the consumers; the 1/2 is in the window)
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int k = lane + 64 * r;
    const c2 wd = cmul(lds_c2(tw + k), sub_conj(v[r], zc[r]));
    xb[k] = add_mi(add_conj(v[r], zc[r]), wd);  // e - i * wd  (pass 2 has read the column: the exchanges are done with it)
  }
}

}  // namespace
