// Precision / recall / density / coverage (Kynkaanniemi et al., NeurIPS 2019; Naeem et al., ICML 2020): the kernels behind
// nn_ops.nn_sqdist_tiled / prdc_scan and metrics.PRDC.  Definitions and the bit-identity argument: DESIGN.md 4.14.
//
//   tiled    the distance matrix of csrc/nn.hip, bit for bit, for operands of thousands of rows each.  A workgroup of 4 waves owns
//            128 queries x 128 references of ONE float64 slice (grid z = NN_SLICES) and walks that slice's chunks c = z, z + 16, ...
//            A chunk goes through LDS in sub-chunks of 32 components, double-buffered: every operand element is loaded from
//            global memory once per workgroup and chunk (by the thread whose 16 bytes it is part of) and read from LDS by the two
//            waves that need its row.  A wave accumulates 4 x 4 tiles of 16 x 16 on v_mfma_f32_16x16x4_f32 from zero over the chunk,
//            with lane group kq = lane >> 4 supplying component 16 s + 4 kq + u at MFMA (s, u) exactly as nn_dot_k does, so the
//            float32 sum of a pair and chunk is the same fmaf chain; at the chunk's end it is added to the wave's float64
//            accumulators (from +0.0, chunks in ascending order: nn_dist_k's slice sum) and the float32 ones restart from zero.
//            The slice sums go to ws[slice][query][reference]; rows past nq / nr are clamped when read and not stored.
//            LDS rows are padded to 40 floats.  A 16-byte LDS read is served in groups of 16 lanes that mix two neighbouring k-quarters
//            (lanes 0-3, 12-15 of one with 4-11 of the next): a stride of 8 banks (mod 64) puts one quarter's 8 rows on the even
//            4-bank groups and the next quarter's on the odd ones, so a group touches all 64 banks once.  A 16-byte write is served
//            8 consecutive lanes at a time, which here are the 32 consecutive floats of one row.
//   finish   one thread per pair: the tree h = 8, 4, 2, 1 over the 16 slice sums in nn_dist_k's order, the norms, the clamp.
//   scan     one wave per row of a float64 distance block, lanes striding the columns: how many columns j hold
//            dist <= radius[j], and the row's minimum; a butterfly over the wave, then lane 0 adds / takes the minimum in place.
#include <cmath>

#include "nn_common.h"

namespace {

constexpr int PT_T = 4;                          // 16-row tiles per wave and operand: a wave owns 64 x 64 pairs
constexpr int PT_ROWS = 2 * 16 * PT_T;           // rows per operand of a workgroup of 2 x 2 waves
constexpr int PT_KS = 32;                        // components per sub-chunk
constexpr int PT_SUBS = NN_CHUNK / PT_KS;
constexpr int PT_STRIDE = PT_KS + 8;             // floats per LDS row: 8 (mod 64) banks from row to row, see above
constexpr int PT_BUF = 2 * PT_ROWS * PT_STRIDE;  // floats per buffer: the queries' rows, then the references'
constexpr int PT_LOADS = 2 * PT_ROWS * (PT_KS / 4) / 256;   // 16-byte pieces a thread stages per sub-chunk
constexpr size_t PT_LDS_BYTES = 2 * PT_BUF * sizeof(float);
static_assert(PT_LOADS * 256 == 2 * PT_ROWS * (PT_KS / 4) && PT_KS % 16 == 0 && NN_CHUNK % PT_KS == 0, "staging does not tile");

template <bool VEC>
__global__ void __launch_bounds__(256) prdc_dot_k(const float* __restrict__ q, const float* __restrict__ r, double* __restrict__ ws,
                                                  long long nq, long long nr, long long D, long long nchunks) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ml = lane & 15, kq = lane >> 4;
  const int wq = w >> 1, wr = w & 1;
  const long long q0 = (long long)blockIdx.y * PT_ROWS, r0 = (long long)blockIdx.x * PT_ROWS, slice = blockIdx.z;
  // staging: piece i of this thread is 4 components of row (tid >> 3) + 32 i of the workgroup's 2 x 128 rows
  const int srow = tid >> 3, scol = (tid & 7) * 4;
  const float* src[PT_LOADS];
#pragma unroll
  for (int i = 0; i < PT_LOADS; ++i) {
    const int row = srow + 32 * i;
    src[i] = row < PT_ROWS ? q + (size_t)min(q0 + row, nq - 1) * D : r + (size_t)min(r0 + row - PT_ROWS, nr - 1) * D;
  }
  const bool active = q0 + wq * (16 * PT_T) < nq && r0 + wr * (16 * PT_T) < nr;   // the whole wave; it still stages and meets barriers
  const float* arow = smem + (wq * (16 * PT_T) + ml) * PT_STRIDE + kq * 4;
  const float* brow = smem + (PT_ROWS + wr * (16 * PT_T) + ml) * PT_STRIDE + kq * 4;

  f32x4 acc[PT_T][PT_T];
  double sum[PT_T][PT_T][4];
#pragma unroll
  for (int a = 0; a < PT_T; ++a) {
#pragma unroll
    for (int b = 0; b < PT_T; ++b) {
      acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) sum[a][b][rr] = 0.0;
    }
  }
  const long long mine = slice < nchunks ? (nchunks - slice + NN_SLICES - 1) / NN_SLICES : 0;   // chunks of this slice
  const long long steps = mine * PT_SUBS;
  f32x4 pre[PT_LOADS];
  if (steps > 0) {
    const long long k = slice * NN_CHUNK + scol;
#pragma unroll
    for (int i = 0; i < PT_LOADS; ++i) pre[i] = nn_load4<VEC>(src[i], k, D);
#pragma unroll
    for (int i = 0; i < PT_LOADS; ++i) *reinterpret_cast<f32x4*>(smem + (srow + 32 * i) * PT_STRIDE + scol) = pre[i];
  }
  __syncthreads();
  for (long long it = 0; it < steps; ++it) {
    const int buf = (int)(it & 1), sub = (int)(it % PT_SUBS);
    const bool more = it + 1 < steps;
    if (more) {
      const long long nx = it + 1, k = (slice + nx / PT_SUBS * NN_SLICES) * NN_CHUNK + nx % PT_SUBS * PT_KS + scol;
#pragma unroll
      for (int i = 0; i < PT_LOADS; ++i) pre[i] = nn_load4<VEC>(src[i], k, D);
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < PT_KS / 16; ++s) {
        f32x4 a[PT_T], b[PT_T];
#pragma unroll
        for (int t = 0; t < PT_T; ++t) {
          a[t] = *reinterpret_cast<const f32x4*>(arow + buf * PT_BUF + t * 16 * PT_STRIDE + s * 16);
          b[t] = *reinterpret_cast<const f32x4*>(brow + buf * PT_BUF + t * 16 * PT_STRIDE + s * 16);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int ta = 0; ta < PT_T; ++ta) {
#pragma unroll
            for (int tb = 0; tb < PT_T; ++tb)
              acc[ta][tb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ta][u], b[tb][u], acc[ta][tb], 0, 0, 0);
          }
        }
      }
      if (sub == PT_SUBS - 1) {   // the chunk is complete: into the float64 slice sum, and from zero again
#pragma unroll
        for (int ta = 0; ta < PT_T; ++ta) {
#pragma unroll
          for (int tb = 0; tb < PT_T; ++tb) {
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) sum[ta][tb][rr] += (double)acc[ta][tb][rr];
            acc[ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < PT_LOADS; ++i)
        *reinterpret_cast<f32x4*>(smem + (buf ^ 1) * PT_BUF + (srow + 32 * i) * PT_STRIDE + scol) = pre[i];
    }
    __syncthreads();   // the other buffer is complete, and this one is free for the step after next
  }
  if (!active) return;
  double* out = ws + (size_t)slice * nq * nr;
#pragma unroll
  for (int ta = 0; ta < PT_T; ++ta) {
#pragma unroll
    for (int tb = 0; tb < PT_T; ++tb) {
      const long long j = r0 + wr * (16 * PT_T) + tb * 16 + ml;
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const long long i = q0 + wq * (16 * PT_T) + ta * 16 + kq * 4 + rr;
        if (i < nq && j < nr) out[(size_t)i * nr + j] = sum[ta][tb][rr];
      }
    }
  }
}

__global__ void __launch_bounds__(256) prdc_finish_k(const double* __restrict__ ws, const double* __restrict__ qn,
                                                     const double* __restrict__ rn, double* __restrict__ dist, long long nq,
                                                     long long nr) {
  const long long pairs = nq * nr, p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= pairs) return;
  double red[NN_SLICES];
#pragma unroll
  for (int s = 0; s < NN_SLICES; ++s) red[s] = ws[(size_t)s * pairs + p];
#pragma unroll
  for (int h = NN_SLICES / 2; h >= 1; h >>= 1) {
#pragma unroll
    for (int s = 0; s < h; ++s) red[s] += red[s + h];
  }
  const double d = qn[p / nr] + rn[p % nr] - 2.0 * red[0];
  dist[p] = d > 0.0 ? d : 0.0;
}

__global__ void __launch_bounds__(256) prdc_scan_k(const double* __restrict__ dist, const double* __restrict__ radius,
                                                   long long* __restrict__ count, double* __restrict__ rowmin, long long nq,
                                                   long long nr) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nq) return;   // the whole wave; no barrier below
  const double* d = dist + (size_t)row * nr;
  int c = 0;
  double m = INFINITY;
#pragma unroll 4
  for (long long j = lane; j < nr; j += 64) {
    const double v = d[j];
    c += v <= radius[j] ? 1 : 0;
    m = v < m ? v : m;
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) {
    c += __shfl_xor(c, x);
    const double o = __shfl_xor(m, x);
    m = o < m ? o : m;
  }
  if (lane == 0) {
    count[row] += c;
    const double old = rowmin[row];
    rowmin[row] = m < old ? m : old;
  }
}

}  // namespace

extern "C" size_t mg_nn_tiled_ws_bytes(int64_t nq, int64_t nr, int64_t D) {
  if (nq < 1 || nr < 1 || D < 1) return 0;
  return (size_t)NN_SLICES * (size_t)nq * (size_t)nr * sizeof(double);
}

extern "C" int mg_nn_sqdist_tiled(const float* q, const float* r, const double* qn, const double* rn, int64_t nq, int64_t nr,
                                  int64_t D, double* dist, void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(q && r && qn && rn && dist && ws && nq > 0 && nr > 0 && D > 0, "mg_nn_sqdist_tiled: bad arguments");
  const long long chunks = nn_chunks(D), qblocks = (nq + PT_ROWS - 1) / PT_ROWS, rblocks = (nr + PT_ROWS - 1) / PT_ROWS;
  MG_CHECK_ARG(chunks < (1ll << 31) && qblocks <= 65535 && rblocks < (1ll << 31) && nq * nr < (1ll << 34),
               "mg_nn_sqdist_tiled: %lld x %lld rows of %lld numbers are more than one launch takes", (long long)nq, (long long)nr,
               (long long)D);
  MG_CHECK_ARG((reinterpret_cast<size_t>(ws) & 7) == 0, "mg_nn_sqdist_tiled: the workspace must be 8-byte aligned");
  if (ws_bytes < mg_nn_tiled_ws_bytes(nq, nr, D)) {
    mg_set_error("mg_nn_sqdist_tiled: workspace too small");
    return MG_EWORKSPACE;
  }
  static MgPerDevice once;
  if (mg_first_use_on_device(once)) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&prdc_dot_k<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)PT_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&prdc_dot_k<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)PT_LDS_BYTES);
  }
  double* sums = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)rblocks, (unsigned)qblocks, NN_SLICES);
  const bool vec = D % 4 == 0 && ((reinterpret_cast<size_t>(q) | reinterpret_cast<size_t>(r)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(prdc_dot_k<true>, grid, dim3(256), PT_LDS_BYTES, (hipStream_t)stream, q, r, sums, (long long)nq,
                       (long long)nr, (long long)D, chunks);
  else
    hipLaunchKernelGGL(prdc_dot_k<false>, grid, dim3(256), PT_LDS_BYTES, (hipStream_t)stream, q, r, sums, (long long)nq,
                       (long long)nr, (long long)D, chunks);
  hipLaunchKernelGGL(prdc_finish_k, dim3((unsigned)((nq * nr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sums, qn, rn, dist,
                     (long long)nq, (long long)nr);
  MG_CHECK_LAUNCH("mg_nn_sqdist_tiled");
  return MG_OK;
}

extern "C" int mg_prdc_scan(const double* dist, const double* radius, int64_t* count, double* rowmin, int64_t nq, int64_t nr,
                            mg_stream_t stream) {
  MG_CHECK_ARG(dist && radius && count && rowmin && nq > 0 && nr > 0, "mg_prdc_scan: bad arguments");
  MG_CHECK_ARG(nq < (1ll << 32) && nr < (1ll << 31), "mg_prdc_scan: %lld x %lld is more than one launch takes", (long long)nq,
               (long long)nr);
  hipLaunchKernelGGL(prdc_scan_k, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, dist, radius,
                     reinterpret_cast<long long*>(count), rowmin, (long long)nq, (long long)nr);
  MG_CHECK_LAUNCH("mg_prdc_scan");
  return MG_OK;
}
