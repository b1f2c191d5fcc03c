// DiffAugment: per-sample random translation with zero fill and cutout, and the adjoint, on (N, C, H, W) float32.
//   forward:  y[i, j]  = (i, j) in the box ? +0 : x[i - dy, j - dx] (inside the image, else +0)
//   backward: gx[i, j] = (i + dy, j + dx) inside the image and outside the box ? gy[i + dy, j + dx] : +0
// Both are "copy one source element or write +0", chosen by a select: the same kernel with the shift negated and the box tested at the
// destination (forward) or at the source (backward).  The parameters are decoded in the kernel from the sample's row of u
// (diffaug_plan.h), so a captured launch follows whatever u holds at replay time.
//
// One thread writes four consecutive columns of one row; a block works inside one (sample, channel) plane, so the parameters are
// wave-uniform.  Vector form (W % 4 == 0, both base pointers 16-byte aligned): one 16-byte store; the shifted source quad straddles at
// most two aligned quads of its row, which are loaded whole and picked from by the wave-uniform misalignment sx & 3.  Scalar form
// (everything else): the same selects on dword loads and stores.
#include "diffaug_plan.h"
#include "mg_common.h"

namespace {

constexpr int DA_THREADS = 256;

template <bool BWD, bool VEC>
__global__ __launch_bounds__(DA_THREADS) void diffaug_k(const float* __restrict__ src, const float* __restrict__ u,
                                                        float* __restrict__ dst, int C, int H, int W, int ops, float p, int slices) {
  const int plane = blockIdx.x / slices, slice = blockIdx.x - plane * slices;
  const int Wq = (W + 3) >> 2;
  const int q = slice * DA_THREADS + threadIdx.x;
  if (q >= H * Wq) return;
  const DaParams P = da_decode(u + (size_t)(plane / C) * DA_U, H, W, ops, p);
  // destination (i, j) reads source (i + sy, j + sx); the box lives in the augmented image's coordinates
  const int sy = BWD ? P.dy : -P.dy, sx = BWD ? P.dx : -P.dx;
  const int i = q / Wq, j0 = (q - i * Wq) << 2;
  const int si = i + sy, sj0 = j0 + sx;
  const int bi = BWD ? si : i, bj0 = BWD ? sj0 : j0;  // where the box is tested
  const bool row_in_box = bi >= P.y0 && bi < P.y1;
  const size_t base = (size_t)plane * H * W;
  float* __restrict__ d = dst + base + (size_t)i * W + j0;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int sj = sj0 + k, bj = bj0 + k;
    ok[k] = si >= 0 && si < H && sj >= 0 && sj < W && !(row_in_box && bj >= P.x0 && bj < P.x1);
  }
  if (si >= 0 && si < H) {
    const float* __restrict__ s = src + base + (size_t)si * W;
    if constexpr (VEC) {
      // aligned quads [c0, c0 + 4) and [c0 + 4, c0 + 8) of the source row hold columns sj0 .. sj0 + 3; W % 4 == 0, so an aligned quad
      // lies wholly inside the row or wholly outside it
      const int r = sj0 & 3, c0 = sj0 - r;
      f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
      if (c0 >= 0 && c0 < W) a = *reinterpret_cast<const f32x4*>(s + c0);
      if (r != 0 && c0 + 4 >= 0 && c0 + 4 < W) b = *reinterpret_cast<const f32x4*>(s + c0 + 4);
      switch (r) {  // wave-uniform
        case 0: v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; break;
        case 1: v[0] = a.y; v[1] = a.z; v[2] = a.w; v[3] = b.x; break;
        case 2: v[0] = a.z; v[1] = a.w; v[2] = b.x; v[3] = b.y; break;
        default: v[0] = a.w; v[1] = b.x; v[2] = b.y; v[3] = b.z; break;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (ok[k]) v[k] = s[sj0 + k];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = ok[k] ? v[k] : 0.f;  // a select, never a product: NaN / inf under the mask do not pass
  if constexpr (VEC) {
    const f32x4 o = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(d) = o;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (j0 + k < W) d[k] = v[k];
  }
}

template <bool BWD>
int diffaug_launch(const char* name, const float* src, const float* u, int n, int c, int h, int w, int ops, float p, float* dst,
                   mg_stream_t stream) {
  MG_CHECK_ARG(src && u && dst && n > 0 && c > 0 && h > 0 && w > 0, "%s: bad arguments", name);
  MG_CHECK_ARG((ops & ~(DA_TRANSLATION | DA_CUTOUT)) == 0, "%s: unknown ops 0x%x", name, ops);
  MG_CHECK_ARG(p >= 0.f && p <= 1.f, "%s: p = %g outside [0, 1]", name, (double)p);
  const long long planes = (long long)n * c, quads = (long long)h * ((w + 3) / 4);
  MG_CHECK_ARG(quads < (1ll << 31) && (long long)h * w < (1ll << 31), "%s: a %d x %d plane is more than one launch takes", name, h, w);
  const long long slices = (quads + DA_THREADS - 1) / DA_THREADS;
  MG_CHECK_ARG(planes * slices < (1ll << 31), "%s: %lld planes of %d x %d are more than one launch takes", name, planes, h, w);
  const size_t bytes = (size_t)planes * h * w * sizeof(float);
  const char *s0 = reinterpret_cast<const char*>(src), *d0 = reinterpret_cast<const char*>(dst);
  MG_CHECK_ARG(s0 + bytes <= d0 || d0 + bytes <= s0, "%s: source and destination overlap", name);
  const char* u0 = reinterpret_cast<const char*>(u);
  MG_CHECK_ARG(u0 + (size_t)n * DA_U * sizeof(float) <= d0 || d0 + bytes <= u0, "%s: u and the destination overlap", name);
  const bool vec = w % 4 == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  const dim3 grid((unsigned)(planes * slices)), block(DA_THREADS);
  if (vec)
    hipLaunchKernelGGL((diffaug_k<BWD, true>), grid, block, 0, (hipStream_t)stream, src, u, dst, c, h, w, ops, p, (int)slices);
  else
    hipLaunchKernelGGL((diffaug_k<BWD, false>), grid, block, 0, (hipStream_t)stream, src, u, dst, c, h, w, ops, p, (int)slices);
  MG_CHECK_LAUNCH(name);
  return MG_OK;
}

}  // namespace

extern "C" int mg_diffaug_fwd(const float* x, const float* u, int n, int c, int h, int w, int ops, float p, float* y,
                              mg_stream_t stream) {
  return diffaug_launch<false>("mg_diffaug_fwd", x, u, n, c, h, w, ops, p, y, stream);
}

extern "C" int mg_diffaug_bwd(const float* gy, const float* u, int n, int c, int h, int w, int ops, float p, float* gx,
                              mg_stream_t stream) {
  return diffaug_launch<true>("mg_diffaug_bwd", gy, u, n, c, h, w, ops, p, gx, stream);
}

extern "C" int mg_diffaug_decode(const float* u_host, int n, int h, int w, int ops, float p, int32_t* out) {
  MG_CHECK_ARG(u_host && out && n > 0 && h > 0 && w > 0, "mg_diffaug_decode: bad arguments");
  MG_CHECK_ARG((ops & ~(DA_TRANSLATION | DA_CUTOUT)) == 0, "mg_diffaug_decode: unknown ops 0x%x", ops);
  MG_CHECK_ARG(p >= 0.f && p <= 1.f, "mg_diffaug_decode: p = %g outside [0, 1]", (double)p);
  for (int i = 0; i < n; ++i) {
    const DaParams q = da_decode(u_host + (size_t)i * DA_U, h, w, ops, p);
    int32_t* o = out + (size_t)i * 6;
    o[0] = q.dy, o[1] = q.dx, o[2] = q.y0, o[3] = q.y1, o[4] = q.x0, o[5] = q.x1;
  }
  return MG_OK;
}
