// Kernel Inception Distance (Binkowski, Sutherland, Arbel, Gretton, "Demystifying MMD GANs", ICLR 2018): the kernels behind
// musicgan_amd/kid_ops.py and metrics.KID / metrics.poly_mmd2.  Definitions and the error bound: DESIGN.md 4.20.
//
//   standardise  one element per thread: out = (float)(((double)x - mean[j]) / sd[j]), 0 where sd[j] is 0 or not finite.
//   rowsums      out[s][i] = the sum over j of k(a[ia[s][i]], b[ib[s][j]]),  k(x, y) = (x.y / d + 1)^3, without ever storing a
//                kernel value.  The tile structure is prdc_dot_k's (csrc/prdc.hip): a workgroup of 2 x 2 waves owns 128 x 128
//                pairs of ONE subset (grid z), stages both operands through LDS in double-buffered sub-chunks of 32 components and
//                accumulates 4 x 4 tiles of 16 x 16 per wave on v_mfma_f32_16x16x4_f32 from zero over a chunk of NN_CHUNK
//                components; a finished chunk is added to the wave's float64 sums in ascending order.  d <= 4096 is at most 16
//                chunks, which the workgroup walks itself: no slices.  The rows are gathered while they are staged: a staging
//                thread's source pointer is the row its index list names (clamped to the operand, so that no list can make a read
//                leave it).  Sub-chunks past d are not walked: they would add products of zeros, which change no bit.
//                Epilogue, all in float64: u = dot / d + 1, u u u, +0.0 for a column >= mb and for the skipped diagonal; then the
//                sum of a row over its columns in an order that the column positions alone decide --
//                    the lane's 4 column tiles in ascending order, the 16 lanes of a tile row in the butterfly 1, 2, 4, 8 (both
//                    partners add the same two numbers, so all 16 hold the same bits), the workgroup's column wave 0 + column
//                    wave 1 through LDS, and the column workgroups through ws[s][column block][i],
//                which the finish kernel (one thread per row) adds from +0.0 in ascending block order.  No atomics.
#include <cmath>

#include "nn_common.h"

namespace {

constexpr int KD_T = 4;                          // 16-row tiles per wave and operand: a wave owns 64 x 64 pairs
constexpr int KD_ROWS = 2 * 16 * KD_T;           // rows per operand of a workgroup of 2 x 2 waves
constexpr int KD_KS = 32;                        // components per sub-chunk
constexpr int KD_SUBS = NN_CHUNK / KD_KS;
constexpr int KD_STRIDE = KD_KS + 8;             // floats per LDS row: prdc_dot_k's padding (8 banks mod 64 from row to row)
constexpr int KD_BUF = 2 * KD_ROWS * KD_STRIDE;  // floats per buffer: the rows of a, then those of b
constexpr int KD_LOADS = 2 * KD_ROWS * (KD_KS / 4) / 256;   // 16-byte pieces a thread stages per sub-chunk
constexpr size_t KD_LDS_BYTES = 2 * KD_BUF * sizeof(float);
constexpr int KD_MAX_D = 4096;
static_assert(KD_LOADS * 256 == 2 * KD_ROWS * (KD_KS / 4) && KD_KS % 16 == 0 && NN_CHUNK % KD_KS == 0, "staging does not tile");
static_assert(2 * KD_ROWS * sizeof(double) <= KD_LDS_BYTES, "the row sums of the two column waves go through the staging buffers");

__global__ void __launch_bounds__(256) kid_standardise_k(const float* __restrict__ x, const double* __restrict__ mean,
                                                         const double* __restrict__ sd, float* __restrict__ out, long long total,
                                                         long long d) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const long long j = p % d;
  const double s = sd[j];
  const bool usable = s != 0.0 && s - s == 0.0;   // not 0, not infinite, not NaN
  out[p] = usable ? (float)(((double)x[p] - mean[j]) / s) : 0.f;
}

template <bool VEC>
__global__ void __launch_bounds__(256) kid_rowsums_k(const float* __restrict__ a, const float* __restrict__ b,
                                                     const int* __restrict__ ia, const int* __restrict__ ib,
                                                     double* __restrict__ ws, long long na, long long nb, long long ma,
                                                     long long mb, long long D, int skip_diag) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ml = lane & 15, kq = lane >> 4;
  const int wa = w >> 1, wb = w & 1;
  const long long a0 = (long long)blockIdx.y * KD_ROWS, b0 = (long long)blockIdx.x * KD_ROWS, subset = blockIdx.z;
  // staging: piece i of this thread is 4 components of row (tid >> 3) + 32 i of the workgroup's 2 x 128 rows
  const int srow = tid >> 3, scol = (tid & 7) * 4;
  const float* src[KD_LOADS];
#pragma unroll
  for (int i = 0; i < KD_LOADS; ++i) {
    const int row = srow + 32 * i;
    const bool first = row < KD_ROWS;
    const long long pos = first ? min(a0 + row, ma - 1) : min(b0 + row - KD_ROWS, mb - 1);   // the position in the subset's list
    const int* list = first ? ia : ib;
    long long at = list ? (long long)list[subset * (first ? ma : mb) + pos] : pos;
    at = max(0ll, min(at, (first ? na : nb) - 1));
    src[i] = (first ? a : b) + (size_t)at * D;
  }
  const bool active = a0 + wa * (16 * KD_T) < ma && b0 + wb * (16 * KD_T) < mb;   // the whole wave; it still stages and meets barriers
  const float* arow = smem + (wa * (16 * KD_T) + ml) * KD_STRIDE + kq * 4;
  const float* brow = smem + (KD_ROWS + wb * (16 * KD_T) + ml) * KD_STRIDE + kq * 4;

  f32x4 acc[KD_T][KD_T];
  double sum[KD_T][KD_T][4];
#pragma unroll
  for (int ta = 0; ta < KD_T; ++ta) {
#pragma unroll
    for (int tb = 0; tb < KD_T; ++tb) {
      acc[ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) sum[ta][tb][rr] = 0.0;
    }
  }
  const int steps = (int)((D + KD_KS - 1) / KD_KS);   // <= 128; sub-chunk `it` holds the components 32 it ..
  f32x4 pre[KD_LOADS];
#pragma unroll
  for (int i = 0; i < KD_LOADS; ++i) pre[i] = nn_load4<VEC>(src[i], scol, D);
#pragma unroll
  for (int i = 0; i < KD_LOADS; ++i) *reinterpret_cast<f32x4*>(smem + (srow + 32 * i) * KD_STRIDE + scol) = pre[i];
  __syncthreads();
  for (int it = 0; it < steps; ++it) {
    const int buf = it & 1, sub = it % KD_SUBS;
    const bool more = it + 1 < steps;
    if (more) {
      const long long k = (long long)(it + 1) * KD_KS + scol;
#pragma unroll
      for (int i = 0; i < KD_LOADS; ++i) pre[i] = nn_load4<VEC>(src[i], k, D);
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < KD_KS / 16; ++s) {
        f32x4 av[KD_T], bv[KD_T];
#pragma unroll
        for (int t = 0; t < KD_T; ++t) {
          av[t] = *reinterpret_cast<const f32x4*>(arow + buf * KD_BUF + t * 16 * KD_STRIDE + s * 16);
          bv[t] = *reinterpret_cast<const f32x4*>(brow + buf * KD_BUF + t * 16 * KD_STRIDE + s * 16);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int ta = 0; ta < KD_T; ++ta) {
#pragma unroll
            for (int tb = 0; tb < KD_T; ++tb)
              acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ta][u], bv[tb][u], acc[ta][tb], 0, 0, 0);
          }
        }
      }
      if (sub == KD_SUBS - 1 || !more) {   // the chunk is complete (or d ends inside it): into the float64 sum, and from zero again
#pragma unroll
        for (int ta = 0; ta < KD_T; ++ta) {
#pragma unroll
          for (int tb = 0; tb < KD_T; ++tb) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) sum[ta][tb][rr] += (double)acc[ta][tb][rr];
            acc[ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < KD_LOADS; ++i)
        *reinterpret_cast<f32x4*>(smem + (buf ^ 1) * KD_BUF + (srow + 32 * i) * KD_STRIDE + scol) = pre[i];
    }
    __syncthreads();   // the other buffer is complete, and this one is free for the step after next
  }
  // every wave past this point, the inactive ones with sums of +0.0 that the masks below turn into +0.0 again or that belong to
  // rows nobody stores: the staging buffers are free (the loop ended on a barrier) and carry the two column waves' row sums
  double* red = reinterpret_cast<double*>(smem);
  const double dd = (double)D;
#pragma unroll
  for (int ta = 0; ta < KD_T; ++ta) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = wa * (16 * KD_T) + ta * 16 + kq * 4 + rr;   // of the workgroup's 128
      const long long i = a0 + row;
      double part = 0.0;
#pragma unroll
      for (int tb = 0; tb < KD_T; ++tb) {
        const long long j = b0 + wb * (16 * KD_T) + tb * 16 + ml;
        const double u = sum[ta][tb][rr] / dd + 1.0;
        const double v = u * u * u;
        part += (j < mb && !(skip_diag && i == j)) ? v : 0.0;
      }
#pragma unroll
      for (int x = 1; x <= 8; x <<= 1) part += __shfl_xor(part, x);
      if (ml == 0) red[wb * KD_ROWS + row] = part;
    }
  }
  __syncthreads();
  if (tid < KD_ROWS && a0 + tid < ma)
    ws[((size_t)subset * gridDim.x + blockIdx.x) * ma + a0 + tid] = red[tid] + red[KD_ROWS + tid];
}

__global__ void __launch_bounds__(256) kid_finish_k(const double* __restrict__ ws, double* __restrict__ out, long long ma,
                                                    long long cblocks, long long total) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;   // subset * ma + i
  if (p >= total) return;
  const long long subset = p / ma, i = p % ma;
  const double* part = ws + (size_t)subset * cblocks * ma + i;
  double v = 0.0;
  for (long long c = 0; c < cblocks; ++c) v += part[(size_t)c * ma];
  out[p] = v;
}

inline long long kid_blocks(long long m) { return (m + KD_ROWS - 1) / KD_ROWS; }

}  // namespace

extern "C" int mg_standardise_rows(const float* x, int64_t n, int64_t d, const double* mean, const double* sd, float* out,
                                   mg_stream_t stream) {
  MG_CHECK_ARG(x && mean && sd && out && n > 0 && d > 0, "mg_standardise_rows: bad arguments");
  MG_CHECK_ARG(n < (1ll << 31) && d < (1ll << 31) && n * d < (1ll << 38), "mg_standardise_rows: %lld x %lld is more than one launch takes",
               (long long)n, (long long)d);
  const long long total = n * d;
  hipLaunchKernelGGL(kid_standardise_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, mean, sd, out,
                     total, (long long)d);
  MG_CHECK_LAUNCH("mg_standardise_rows");
  return MG_OK;
}

extern "C" size_t mg_polyk_ws_bytes(int64_t subsets, int64_t ma, int64_t mb) {
  if (subsets < 1 || ma < 1 || mb < 1 || subsets > 65535 || kid_blocks(ma) > 65535 || kid_blocks(mb) >= (1ll << 31)) return 0;
  return (size_t)subsets * (size_t)kid_blocks(mb) * (size_t)ma * sizeof(double);
}

extern "C" int mg_polyk_rowsums(const float* a, int64_t na, const float* b, int64_t nb, const int32_t* ia, const int32_t* ib,
                                int64_t subsets, int64_t ma, int64_t mb, int64_t d, int skip_diag, double* out, void* ws,
                                size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(a && b && out && ws && na > 0 && nb > 0 && subsets > 0 && ma > 0 && mb > 0 && d > 0, "mg_polyk_rowsums: bad arguments");
  MG_CHECK_ARG(d <= KD_MAX_D, "mg_polyk_rowsums: at most %d numbers per row, got %lld", KD_MAX_D, (long long)d);
  MG_CHECK_ARG(na < (1ll << 31) && nb < (1ll << 31), "mg_polyk_rowsums: row numbers are int32");
  MG_CHECK_ARG(ia || ma <= na, "mg_polyk_rowsums: without a list the rows 0 .. ma - 1 of a are taken: ma = %lld > na = %lld",
               (long long)ma, (long long)na);
  MG_CHECK_ARG(ib || mb <= nb, "mg_polyk_rowsums: without a list the rows 0 .. mb - 1 of b are taken: mb = %lld > nb = %lld",
               (long long)mb, (long long)nb);
  MG_CHECK_ARG(!skip_diag || ma == mb, "mg_polyk_rowsums: skip_diag needs ma = mb, got %lld and %lld", (long long)ma, (long long)mb);
  const size_t need = mg_polyk_ws_bytes(subsets, ma, mb);
  MG_CHECK_ARG(need > 0 && subsets * ma < (1ll << 38), "mg_polyk_rowsums: %lld subsets of %lld x %lld rows are more than one launch takes",
               (long long)subsets, (long long)ma, (long long)mb);
  MG_CHECK_ARG((reinterpret_cast<size_t>(ws) & 7) == 0, "mg_polyk_rowsums: the workspace must be 8-byte aligned");
  if (ws_bytes < need) {
    mg_set_error("mg_polyk_rowsums: workspace too small");
    return MG_EWORKSPACE;
  }
  static MgPerDevice once;
  if (mg_first_use_on_device(once)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kid_rowsums_k<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)KD_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&kid_rowsums_k<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)KD_LDS_BYTES);
  }
  double* part = reinterpret_cast<double*>(ws);
  const long long cblocks = kid_blocks(mb), total = subsets * ma;
  const dim3 grid((unsigned)cblocks, (unsigned)kid_blocks(ma), (unsigned)subsets);
  const bool vec = d % 4 == 0 && ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(kid_rowsums_k<true>, grid, dim3(256), KD_LDS_BYTES, (hipStream_t)stream, a, b, ia, ib, part, (long long)na,
                       (long long)nb, (long long)ma, (long long)mb, (long long)d, skip_diag);
  else
    hipLaunchKernelGGL(kid_rowsums_k<false>, grid, dim3(256), KD_LDS_BYTES, (hipStream_t)stream, a, b, ia, ib, part, (long long)na,
                       (long long)nb, (long long)ma, (long long)mb, (long long)d, skip_diag);
  hipLaunchKernelGGL(kid_finish_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part, out,
                     (long long)ma, cblocks, total);
  MG_CHECK_LAUNCH("mg_polyk_rowsums");
  return MG_OK;
}
