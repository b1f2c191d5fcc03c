// Perceptual path length in the log-mel rows (Karras, Laine, Aila, "A Style-Based Generator Architecture for GANs", CVPR 2019, with
// the squared distance of log-mel rows in the place of LPIPS): the kernels behind musicgan_amd/ppl_ops.py and metrics.PPL.
// Definitions and the error bounds: DESIGN.md 4.22.
//
//   slerp    one wave (a workgroup of 64 threads) per pair of latents, any d >= 1.  Lane l owns the components 4 l .. 4 l + 3,
//            4 l + 256 .. and adds x x, y y and x y to three float64 sums in ascending order from +0.0 (every product rounded, then
//            the sum: no fma); the 64 sums of a kind are added by the butterfly 32, 16, 8, 4, 2, 1, in which both partners add the
//            same two numbers, so every lane holds the same bits.  The order depends on d alone; components past d count as zeros,
//            which change no bit, so aligned rows (16-byte loads) and unaligned ones (4-byte loads) add the same numbers in the same
//            order.  The angle, the linear fallback below 1e-6 and the weights sin((1 - t) w) / sin w, sin(t w) / sin w at t and at
//            t + eps are float64; lanes 0 .. 4 take one sine each.  At t = 0 the arguments are w and 0, so the weights are w / w = 1
//            and 0 / sin w = 0 exactly; a term whose weight is exactly 0 is left out, so that the other end comes out bit for bit.
//            An angle within 1e-6 of pi: flag 1, both outputs +0.0.  Every element of za, zb and flag is written.
//   sqdist   one wave per pair of rows, four waves per workgroup: the same lane ownership, (double)a - (double)b, its square added in
//            ascending order, the same butterfly, times `scale`.  out[i] is a function of its two rows, D and scale alone.
//   No atomics, no workspace, no LDS.
#include <cmath>

#include "nn_common.h"

namespace {

constexpr double PPL_MIN_ANGLE = 1e-6;               // project.slerp's _SLERP_MIN_ANGLE
constexpr double PPL_PI = 3.141592653589793;         // math.pi
constexpr int PPL_STEP = 4 * 64;                     // components a wave takes per step

__device__ __forceinline__ double ppl_wave_sum(double v) {
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) v += __shfl_xor(v, x);
  return v;
}

__device__ __forceinline__ float ppl_mix(double w0, float x, double w1, float y) {
  const double p = w0 * (double)x, q = w1 * (double)y;
  return (float)(w1 == 0.0 ? p : (w0 == 0.0 ? q : p + q));
}

template <bool VEC>
__global__ void __launch_bounds__(64) ppl_slerp_k(const float* __restrict__ z0, const float* __restrict__ z1,
                                                  const double* __restrict__ t, double eps, float* __restrict__ za,
                                                  float* __restrict__ zb, int* __restrict__ flag, long long d) {
  const long long pair = blockIdx.x;
  const int lane = threadIdx.x;
  const float* a = z0 + (size_t)pair * d;
  const float* b = z1 + (size_t)pair * d;
  double saa = 0.0, sbb = 0.0, sab = 0.0;
  for (long long k = 4ll * lane; k < d; k += PPL_STEP) {
    const f32x4 av = nn_load4<VEC>(a, k, d), bv = nn_load4<VEC>(b, k, d);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double x = av[u], y = bv[u];
      saa += x * x;
      sbb += y * y;
      sab += x * y;
    }
  }
  saa = ppl_wave_sum(saa);
  sbb = ppl_wave_sum(sbb);
  sab = ppl_wave_sum(sab);
  const double na = sqrt(saa), nb = sqrt(sbb);
  double omega = 0.0;
  if (na > 0.0 && nb > 0.0) omega = acos(fmax(-1.0, fmin(1.0, sab / (na * nb))));
  const bool antipodal = PPL_PI - omega < PPL_MIN_ANGLE;
  const double ta = t[pair], tb = ta + eps;
  double wa0 = 1.0 - ta, wa1 = ta, wb0 = 1.0 - tb, wb1 = tb;   // the straight line
  if (!antipodal && !(omega < PPL_MIN_ANGLE)) {                // the same branch in every lane: omega is the same bits
    const double arg = lane == 0 ? omega : lane == 1 ? wa0 * omega : lane == 2 ? wa1 * omega : lane == 3 ? wb0 * omega : wb1 * omega;
    const double s = sin(arg);
    const double s0 = __shfl(s, 0);
    wa0 = __shfl(s, 1) / s0;
    wa1 = __shfl(s, 2) / s0;
    wb0 = __shfl(s, 3) / s0;
    wb1 = __shfl(s, 4) / s0;
  }
  if (lane == 0) flag[pair] = antipodal ? 1 : 0;
  float* oa = za + (size_t)pair * d;
  float* ob = zb + (size_t)pair * d;
  for (long long k = 4ll * lane; k < d; k += PPL_STEP) {
    const f32x4 av = nn_load4<VEC>(a, k, d), bv = nn_load4<VEC>(b, k, d);
    f32x4 ra, rb;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ra[u] = antipodal ? 0.f : ppl_mix(wa0, av[u], wa1, bv[u]);
      rb[u] = antipodal ? 0.f : ppl_mix(wb0, av[u], wb1, bv[u]);
    }
    if constexpr (VEC) {   // d % 4 == 0: k < d covers all four
      *reinterpret_cast<f32x4*>(oa + k) = ra;
      *reinterpret_cast<f32x4*>(ob + k) = rb;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (k + u < d) {
          oa[k + u] = ra[u];
          ob[k + u] = rb[u];
        }
      }
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) ppl_sqdist_k(const float* __restrict__ a, const float* __restrict__ b, double scale,
                                                    double* __restrict__ out, long long n, long long D) {
  const long long pair = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (pair >= n) return;   // the whole wave
  const int lane = threadIdx.x & 63;
  const float* ra = a + (size_t)pair * D;
  const float* rb = b + (size_t)pair * D;
  double s = 0.0;
  for (long long k = 4ll * lane; k < D; k += PPL_STEP) {
    const f32x4 av = nn_load4<VEC>(ra, k, D), bv = nn_load4<VEC>(rb, k, D);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double df = (double)av[u] - (double)bv[u];
      s += df * df;
    }
  }
  s = ppl_wave_sum(s);
  if (lane == 0) out[pair] = scale * s;
}

inline bool ppl_aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mg_slerp_pairs(const float* z0, const float* z1, const double* t, int64_t n, int64_t d, double eps, float* za,
                              float* zb, int32_t* flag, mg_stream_t stream) {
  MG_CHECK_ARG(z0 && z1 && t && za && zb && flag && n > 0 && d > 0, "mg_slerp_pairs: bad arguments");
  MG_CHECK_ARG(n < (1ll << 31) && d < (1ll << 31) && n * d < (1ll << 38), "mg_slerp_pairs: %lld x %lld is more than one launch takes",
               (long long)n, (long long)d);
  MG_CHECK_ARG(eps == eps, "mg_slerp_pairs: eps is not a number");
  const bool vec = d % 4 == 0 && ppl_aligned16(z0) && ppl_aligned16(z1) && ppl_aligned16(za) && ppl_aligned16(zb);
  if (vec)
    hipLaunchKernelGGL(ppl_slerp_k<true>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, z0, z1, t, eps, za, zb, flag,
                       (long long)d);
  else
    hipLaunchKernelGGL(ppl_slerp_k<false>, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, z0, z1, t, eps, za, zb, flag,
                       (long long)d);
  MG_CHECK_LAUNCH("mg_slerp_pairs");
  return MG_OK;
}

extern "C" int mg_rows_sqdist(const float* a, const float* b, int64_t n, int64_t d, double scale, double* out, mg_stream_t stream) {
  MG_CHECK_ARG(a && b && out && n > 0 && d > 0, "mg_rows_sqdist: bad arguments");
  MG_CHECK_ARG(n < (1ll << 31) && d < (1ll << 31) && n * d < (1ll << 38), "mg_rows_sqdist: %lld x %lld is more than one launch takes",
               (long long)n, (long long)d);
  const bool vec = d % 4 == 0 && ppl_aligned16(a) && ppl_aligned16(b);
  const dim3 grid((unsigned)((n + 3) / 4));
  if (vec)
    hipLaunchKernelGGL(ppl_sqdist_k<true>, grid, dim3(256), 0, (hipStream_t)stream, a, b, scale, out, (long long)n, (long long)d);
  else
    hipLaunchKernelGGL(ppl_sqdist_k<false>, grid, dim3(256), 0, (hipStream_t)stream, a, b, scale, out, (long long)n, (long long)d);
  MG_CHECK_LAUNCH("mg_rows_sqdist");
  return MG_OK;
}
