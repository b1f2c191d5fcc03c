// The in-LDS radix-2 FFT of the untuned paths (mg_stft_generic, mg_codec_inv's frames, the Vorbis transforms) and the DCT-IV
// that the Vorbis decoder and encoder build on it.  One workgroup per transform; every routine ends on a workgroup barrier.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace {

// twiddle of butterfly k (< half = 2^st) of stage st: w = e^{sign * i pi k / half}
struct TwTable {  // forward, from a table w[j] = e^{-2 pi i j / N}, j < N / 2
  const float2* w;
  int lgN;
  __device__ __forceinline__ float2 operator()(int k, int st) const { return w[k << (lgN - 1 - st)]; }
};
struct TwForward {  // e^{-i pi k / half}
  __device__ __forceinline__ float2 operator()(int k, int st) const {
    float sn, cs;
    sincospif((float)k / (float)(1 << st), &sn, &cs);
    return make_float2(cs, -sn);
  }
};
struct TwInverse {  // e^{+2 pi i k / len}, len = 2 half
  __device__ __forceinline__ float2 operator()(int k, int st) const {
    float s, c;
    sincospif(2.0f * (float)k / (float)(2 << st), &s, &c);
    return make_float2(c, s);
  }
};

// The lgN decimation-in-time stages over buf[0, 2^lgN), whose input stands in bit-reversed order, by `nthreads` threads.
template <class Tw>
__device__ __forceinline__ void fft_radix2_lds(float2* buf, int lgN, int tid, int nthreads, Tw tw) {
  const int pairs = 1 << (lgN - 1);
  for (int st = 0; st < lgN; ++st) {
    const int half = 1 << st;
    for (int i = tid; i < pairs; i += nthreads) {
      const int k = i & (half - 1), j = ((i >> st) << (st + 1)) + k;
      const float2 w = tw(k, st);
      const float2 a = buf[j], b = buf[j + half];
      const float2 t = make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x);
      buf[j] = make_float2(a.x + t.x, a.y + t.y);
      buf[j + half] = make_float2(a.x - t.x, a.y - t.y);
    }
    __syncthreads();
  }
}

// DCT-IV of in[0, M) into out[0, M) (which may be `in`), times `scale`, through the M / 2 complex points of `buf`: pre-twiddle
// into bit-reversed order, FFT, post-twiddle.  pre[t] = e^{-i pi (t + 1/4) / M}, post[t] = e^{-i pi t / M}, t < M / 2, and
// w[j] = e^{-2 pi i j / (M / 2)}, j < M / 4: audio.vorbis.dct4_tables(M).  The caller's barrier stands before the call; none
// follows the last store to `out`.
__device__ __forceinline__ void dct4_lds(const float* in, float* out, float2* buf, int M, const float2* pre, const float2* post,
                                         const float2* w, float scale, int tid, int nthreads) {
  const int H = M / 2, lg = 31 - __clz(H);
  for (int t = tid; t < H; t += nthreads) {
    const float re = in[2 * t], im = in[M - 1 - 2 * t];
    const float2 q = pre[t];
    const int r = (int)(__brev((uint32_t)t) >> (32 - lg));
    buf[r] = make_float2(re * q.x - im * q.y, re * q.y + im * q.x);
  }
  __syncthreads();
  fft_radix2_lds(buf, lg, tid, nthreads, TwTable{w, lg});
  for (int s = tid; s < H; s += nthreads) {
    const float2 v = buf[s], q = post[s];
    out[2 * s] = (v.x * q.x - v.y * q.y) * scale;
    out[M - 1 - 2 * s] = -(v.x * q.y + v.y * q.x) * scale;
  }
}

}  // namespace
