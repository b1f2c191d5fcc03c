// Griffin-Lim phase refinement for the 1024 / 256 STFT (definition: DESIGN.md, "Griffin-Lim"): hold the magnitude M, alternate
//   wav = ISTFT(Z);  R = STFT(wav);  c = R - mu * R_prev;  Z = M * c / (|c| + 1e-16)
// and finish with one more ISTFT.  Per iteration: istft1024_kernel, stft1024_kernel (mg_stft_1024 as it is), gl_project.
//
// istft1024_kernel is the inverse of stft1024_kernel and built like it.  A workgroup (8 waves, persistent, two per CU) takes a tile
// of FPT = 16 consecutive frames: the 512 x 16 tile of Z is loaded with the lanes along t (128-byte runs of the frequency-major
// spectrum) and transposed through LDS into one 4 KiB column per frame; one wave inverts one frame in its column -- Hermitian
// shortcut: the 1024 real samples are the 512-point complex inverse transform of Z'[k] = (X[k] + conj X[512-k]) + i e^{+2 pi i k/1024}
// (X[k] - conj X[512-k]), evaluated as conj(FFT(conj Z')) with the forward passes and tables of fft512.h -- and leaves the windowed
// frame there; then every output sample of the tile's HPT = 13 hops gathers its <= 4 frames from LDS, newest frame first (the order
// of mg_codec_inv's inv_overlap_add), divides by the window envelope of the frames that exist and is stored once, 16 bytes per lane.
// No frame buffer in HBM: the three frames in front of a tile are recomputed (3 / 13 more FFT work; their reads of Z hit the L2).
#include "fft512.h"
#include "mg_common.h"

#include <cstdint>

namespace {

constexpr int FPT = NWAVE * FPW;         // frames per tile
constexpr int HPT = FPT - 3;             // hops of 256 output samples per tile: hop h sums frames h-3 .. h
constexpr size_t ISTFT_LDS = (size_t)(TW_FLOATS + NFFT + FPT * XSTR * 2) * sizeof(float);
constexpr int ZPT = NB * FPT / (64 * NWAVE);  // spectrum values per thread and tile

__global__ void __launch_bounds__(64 * NWAVE, 2) istft1024_kernel(const float2* __restrict__ Z, float* __restrict__ wav, int TT,
                                                                  int ntiles) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  c2* tw = reinterpret_cast<c2*>(smem);          // e^{-2 pi i k / 1024}, k < 512
  c2* tw1 = tw + NB;                              // the pass tables of fft512.h
  c2* tw2 = tw1 + 64;
  float* win = smem + TW_FLOATS;                  // periodic Hann(1024)
  c2* xbuf = reinterpret_cast<c2*>(win + NFFT);   // [FPT][XSTR]: a frame's spectrum, then its exchanges, then its 1024 samples

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int m = tid; m < NFFT; m += 64 * NWAVE) win[m] = 0.5f - 0.5f * fft512_fill_tables(tw, tw1, tw2, m);

  // tile i writes hops h0 = 2 + HPT i .. h0 + HPT - 1 of the un-trimmed signal (the centre trim drops hops 0 and 1) from the
  // frames tA = h0 - 3 .. tA + FPT - 1; frames before 0 or past TT - 1 do not exist and are left out of sum and envelope.
  const int lf = tid & (FPT - 1), lk = tid / FPT;  // this thread's frame slot and first bin of the tile load
  c2 zn[ZPT];                                      // the tile in flight: requested under the overlap-add of the tile before
  auto load_tile = [&](int tile) {
    const int t = 2 + tile * HPT - 3 + lf;
    const bool ok = tile < ntiles && t >= 0 && t < TT;
#pragma unroll
    for (int i = 0; i < ZPT; ++i) {
      const int k = lk + (64 * NWAVE / FPT) * i;
      zn[i] = c2{0.f, 0.f};
      if (ok) {
        const float2 z = Z[(size_t)k * TT + t];
        zn[i] = c2{z.x, z.y};
      }
    }
  };
  load_tile(blockIdx.x);
  __syncthreads();
  const float norm = 19.595917942265423f / (float)NFFT;  // sqrt(sum w^2) / N
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int h0 = 2 + tile * HPT, tA = h0 - 3;
#pragma unroll
    for (int i = 0; i < ZPT; ++i) xbuf[lf * XSTR + lk + (64 * NWAVE / FPT) * i] = zn[i];
    __syncthreads();
#pragma unroll 1
    for (int f = 0; f < FPW; ++f) {
      const int fl = wave * FPW + f, t = tA + fl;
      if (t < 0 || t >= TT) continue;  // wave-uniform
      c2* xb = xbuf + fl * XSTR;
      c2 v[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = lane + 64 * r;
        c2 b = lds_c2(xb + k), a = lds_c2(xb + ((NB - k) & (NB - 1)));  // X[k], X[512 - k]
        if (k == 0) {
          b.y = 0.f;          // the imaginary part of DC is ignored
          a = c2{0.f, 0.f};   // the Nyquist row is zero
        }
        const c2 wd = cmul(lds_c2(tw + k), sub_conj(a, b));
        v[r] = sub_mi(add_conj(a, b), wd);  // conj Z'[k] = (X[512-k] + conj X[k]) + i e^{-2 pi i k/1024} (X[512-k] - conj X[k])
      }
      __builtin_amdgcn_wave_barrier();
      fft512_wave(v, xb, tw1, tw2, lane);
      // y[n] = conj v, n = lane + 64 r: samples 2 n and 2 n + 1 are its real and imaginary part
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int n = lane + 64 * r;
        const c2 w = lds_c2(reinterpret_cast<const c2*>(win + 2 * n));
        xb[n] = c2{v[r].x * norm * w.x, -v[r].y * norm * w.y};
      }
    }
    __syncthreads();
    load_tile(tile + (int)gridDim.x);  // in flight under the overlap-add (under the FFTs it would cost the second workgroup per CU its registers)
    for (int hh = wave; hh < HPT; hh += NWAVE) {
      const int h = h0 + hh;
      if (h > TT) break;  // the last hop is TT: 256 (TT - 1) samples in all
      const int i0 = 4 * lane;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f}, env = {0.f, 0.f, 0.f, 0.f};
      const int t_hi = h < TT - 1 ? h : TT - 1, t_lo = h - 3 > 0 ? h - 3 : 0;
      for (int t = t_hi; t >= t_lo; --t) {
        const int off = HOP * (h - t) + i0;
        const f32x4 fr = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(xbuf + (t - tA) * XSTR) + off);
        const f32x4 w = *reinterpret_cast<const f32x4*>(win + off);
        acc += fr;
        env += w * w;
      }
      *reinterpret_cast<f32x4*>(wav + (size_t)HOP * (h - 2) + i0) = acc / env;
    }
    __syncthreads();
  }
}

// The magnitude projection, two bins per thread: c = R - mu * R_prev (FIRST: R_prev = 0 and is not read), Z = M * (c / (|c| + 1e-16)),
// and this workgroup's float64 sums of (|R| - M)^2 and M^2 for the convergence figure.  R_prev is not copied: the loop hands
// the forward STFT two buffers in turn.  Fixed grid, fixed order of every sum, no atomics.
template <bool FIRST>
__global__ void __launch_bounds__(256) gl_project(const f32x4* __restrict__ R, const f32x4* __restrict__ Rp, const float2* __restrict__ M,
                                                  f32x4* __restrict__ Z, double* __restrict__ part, float mu, size_t pairs) {
  __shared__ double red[8];
  double num = 0.0, den = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (size_t)gridDim.x * 256) {
    const f32x4 r = R[i];
    const float2 m = M[i];
    f32x4 c = r;
    if (!FIRST) {
      const f32x4 p = Rp[i];
      c = r - mu * p;
    }
    // |c| correctly rounded (through float64): with the division and the product that leaves |Z| within 3 ulp of M
    const float a0 = (float)sqrt((double)c[0] * c[0] + (double)c[1] * c[1]) + 1e-16f;
    const float a1 = (float)sqrt((double)c[2] * c[2] + (double)c[3] * c[3]) + 1e-16f;
    Z[i] = f32x4{m.x * (c[0] / a0), m.x * (c[1] / a0), m.y * (c[2] / a1), m.y * (c[3] / a1)};
    const double d0 = sqrt((double)r[0] * r[0] + (double)r[1] * r[1]) - (double)m.x;
    const double d1 = sqrt((double)r[2] * r[2] + (double)r[3] * r[3]) - (double)m.y;
    num += d0 * d0;
    num += d1 * d1;
    den += (double)m.x * m.x;
    den += (double)m.y * m.y;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    num += __shfl_xor(num, d);
    den += __shfl_xor(den, d);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * wave] = num;
    red[2 * wave + 1] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = ((red[0] + red[2]) + red[4]) + red[6];
    part[2 * blockIdx.x + 1] = ((red[1] + red[3]) + red[5]) + red[7];
  }
}

// tiny: block k adds the nb partial pairs of iteration k in a fixed order; conv[k] = sqrt(sum (|R_k| - M)^2 / sum M^2)
__global__ void __launch_bounds__(256) gl_convergence(const double* __restrict__ part, int nb, double* __restrict__ conv) {
  __shared__ double red[8];
  const double* p = part + (size_t)blockIdx.x * nb * 2;
  double num = 0.0, den = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    num += p[2 * i];
    den += p[2 * i + 1];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    num += __shfl_xor(num, d);
    den += __shfl_xor(den, d);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[2 * wave] = num;
    red[2 * wave + 1] = den;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    conv[blockIdx.x] = sqrt((((red[0] + red[2]) + red[4]) + red[6]) / (((red[1] + red[3]) + red[5]) + red[7]));
}

int project_blocks(int TT) {
  const size_t pairs = (size_t)NB * TT / 2;
  const size_t nb = (pairs + 255) / 256;
  return (int)(nb < 2048 ? nb : 2048);
}

int launch_istft(const float* Z, float* wav, int TT, hipStream_t s) {
  static MgPerDevice once;  // the LDS limit is a per-device function attribute
  if (mg_first_use_on_device(once)) {
    const hipError_t ea = hipFuncSetAttribute(reinterpret_cast<const void*>(&istft1024_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (ea != hipSuccess) {
      mg_set_error("mg_istft_1024: hipFuncSetAttribute: %s", hipGetErrorString(ea));
      return MG_ELAUNCH;
    }
  }
  const int ntiles = (TT - 1 + HPT - 1) / HPT;
  const int n_cu = mg_cu_count();
  const int blocks = ntiles < 2 * n_cu ? ntiles : 2 * n_cu;
  hipLaunchKernelGGL(istft1024_kernel, dim3(blocks), dim3(64 * NWAVE), ISTFT_LDS, s, reinterpret_cast<const float2*>(Z), wav, TT,
                     ntiles);
  MG_CHECK_LAUNCH("mg_istft_1024");
  return MG_OK;
}

}  // namespace

extern "C" int mg_istft_1024(const float* z_c64, float* wav_out, int TT, mg_stream_t stream) {
  MG_CHECK_ARG(z_c64 && wav_out, "mg_istft_1024: bad arguments");
  MG_CHECK_ARG(TT >= 4 && TT < (1 << 30), "mg_istft_1024: needs 4 <= TT < 2^30 frames (got %d)", TT);
  MG_CHECK_ARG(reinterpret_cast<uintptr_t>(z_c64) % 8 == 0 && reinterpret_cast<uintptr_t>(wav_out) % 16 == 0,
               "mg_istft_1024: the spectrum must be 8-byte aligned, the waveform 16-byte aligned");
  return launch_istft(z_c64, wav_out, TT, (hipStream_t)stream);
}

extern "C" size_t mg_griffin_lim_ws_bytes(int TT, int n_iter) {
  if (TT < 1 || n_iter < 0) return 0;
  return (size_t)2 * NB * TT * sizeof(float2) + ((size_t)n_iter * project_blocks(TT) * 2 + 2) * sizeof(double);
}

extern "C" int mg_griffin_lim(const float* magn, float* z_c64, float* wav_out, double* convergence, void* ws, size_t ws_bytes, int TT,
                              int n_iter, float momentum, mg_stream_t stream) {
  MG_CHECK_ARG(magn && z_c64 && wav_out && (ws || n_iter == 0), "mg_griffin_lim: bad arguments");
  MG_CHECK_ARG(TT >= 4 && TT < (1 << 30), "mg_griffin_lim: needs 4 <= TT < 2^30 frames (got %d)", TT);
  MG_CHECK_ARG(n_iter >= 0, "mg_griffin_lim: n_iter must not be negative (got %d)", n_iter);
  MG_CHECK_ARG(momentum >= 0.f && momentum < 1.f, "mg_griffin_lim: momentum must lie in [0, 1) (got %g)", (double)momentum);
  MG_CHECK_ARG((reinterpret_cast<uintptr_t>(magn) | reinterpret_cast<uintptr_t>(z_c64) | reinterpret_cast<uintptr_t>(wav_out) |
                reinterpret_cast<uintptr_t>(ws)) % 16 == 0 && reinterpret_cast<uintptr_t>(convergence) % 8 == 0,
               "mg_griffin_lim: magnitude, spectrum, waveform and workspace must be 16-byte aligned");
  if (ws_bytes < mg_griffin_lim_ws_bytes(TT, n_iter)) {
    mg_set_error("mg_griffin_lim: workspace too small");
    return MG_EWORKSPACE;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t bins = (size_t)NB * TT;
  float* buf[2] = {reinterpret_cast<float*>(ws), reinterpret_cast<float*>(ws) + 2 * bins};  // R of even / odd iterations
  double* part = reinterpret_cast<double*>(reinterpret_cast<float*>(ws) + 4 * bins);
  const int nb = project_blocks(TT);
  const float mu = (float)((double)momentum / (1.0 + (double)momentum));
  for (int k = 0; k < n_iter; ++k) {
    int rc = launch_istft(z_c64, wav_out, TT, s);
    if (rc != MG_OK) return rc;
    float* R = buf[k & 1];
    rc = mg_stft_1024(wav_out, R, nullptr, (int64_t)HOP * (TT - 1), stream);
    if (rc != MG_OK) return rc;
    const f32x4* Rv = reinterpret_cast<const f32x4*>(R);
    const f32x4* Pv = reinterpret_cast<const f32x4*>(buf[(k & 1) ^ 1]);
    const float2* Mv = reinterpret_cast<const float2*>(magn);
    f32x4* Zv = reinterpret_cast<f32x4*>(z_c64);
    double* pk = part + (size_t)k * nb * 2;
    if (k == 0)
      hipLaunchKernelGGL(gl_project<true>, dim3(nb), dim3(256), 0, s, Rv, Pv, Mv, Zv, pk, mu, bins / 2);
    else
      hipLaunchKernelGGL(gl_project<false>, dim3(nb), dim3(256), 0, s, Rv, Pv, Mv, Zv, pk, mu, bins / 2);
    MG_CHECK_LAUNCH("mg_griffin_lim(project)");
  }
  const int rc = launch_istft(z_c64, wav_out, TT, s);
  if (rc != MG_OK) return rc;
  if (convergence && n_iter > 0) {
    hipLaunchKernelGGL(gl_convergence, dim3(n_iter), dim3(256), 0, s, part, nb, convergence);
    MG_CHECK_LAUNCH("mg_griffin_lim(convergence)");
  }
  return MG_OK;
}
