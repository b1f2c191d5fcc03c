// Nearest neighbours in pixel space (Karras et al., "Progressive Growing of GANs", ICLR 2018, section 6.3: did the generator copy the
// training set?): the kernels behind musicgan_amd/nn_ops.py and metrics.NearestNeighbours.  The reference project has no such metric;
// the definition implemented here is the one DESIGN.md states ("Evaluation: nearest training neighbours").
//
//   d(q, r) = max(0, |q|^2 + |r|^2 - 2 q.r), rows of D float32 numbers, everything outside the dot product in float64.
//
//   sqnorm   one workgroup per row: float64 sums of the exact squares (a float32 squared has 48 significant bits), thread t takes
//            the elements t, t + 256, ..., then a fixed tree over the 256 threads.  The order depends on D alone.
//   dot      a GEMM with a tiny output (nq x nr) and an enormous reduction dimension, so D is what is split across the chip: ONE
//            WAVE accumulates 2 x (16 queries x 16 references) over ONE CHUNK of NN_CHUNK = 256 consecutive components on
//            v_mfma_f32_16x16x4_f32 and leaves its float32 sums in the workspace part[chunk][query][reference].  Both operands have
//            the reduction dimension contiguous, so a lane reads 4 consecutive floats of its row (16 bytes; the four k-quarters of
//            a row's 16 components are one 64-byte run) straight from global memory, no LDS: nothing is reused inside a wave beyond
//            the registers.  MFMA u of a step takes element u of every lane's four, so inside a chunk the components are
//            added in the fixed order  16 s + 4 (lane >> 4) + u  ->  (s, u, lane >> 4): a permutation of the chunk that depends on
//            nothing.  The MFMA is a chain of fmaf (one rounding per multiply-add), so a partial sum is a function of the two
//            rows' chunk alone: not of the tile the pair sits in, nor of nq, nr or the grid.  Rows past nq / nr are clamped to the
//            last row when read (never past a row) and not stored; components past D read as zero, which leaves a chain as it is.
//   dist     S = sum over chunks of the float32 partial sums in float64: slice s of 16 adds the chunks s, s + 16, ... in order,
//            then a fixed tree over the slices: the order depends on the number of chunks, that is on D, alone.  Then the clamp.
//   merge    one thread per query keeps its k best (distance, id) pairs, ascending, in LDS while the candidates of the batch go
//            by: a candidate whose id is the query's own (>= 0) is skipped, ties in the distance go to the smaller id, so the list
//            is the k smallest of everything fed under the total order (distance, id), however it was fed.  An empty slot holds
//            (DBL_MAX, -1), which every candidate beats.
#include <cfloat>

#include "nn_common.h"

namespace {

constexpr int NN_TQ = 2;                       // 16-query tiles per wave
constexpr int NN_QB = 16 * NN_TQ * 4;          // queries per workgroup of 4 waves
constexpr int NN_MAXK = 16;

__global__ void __launch_bounds__(256) nn_sqnorm_k(const float* __restrict__ x, double* __restrict__ out, long long D) {
  __shared__ double red[256];
  const float* row = x + (size_t)blockIdx.x * D;
  double s = 0.0;
  for (long long i = threadIdx.x; i < D; i += 256) {
    const double v = (double)row[i];
    s += v * v;
  }
  s = mg_block_sum_f64(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

template <bool VEC>
__global__ void __launch_bounds__(256) nn_dot_k(const float* __restrict__ q, const float* __restrict__ r, float* __restrict__ part,
                                                long long nq, long long nr, long long D) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, ml = lane & 15, kq = lane >> 4;
  const long long chunk = blockIdx.x;
  const long long q0 = (long long)blockIdx.y * NN_QB + w * (16 * NN_TQ), r0 = (long long)blockIdx.z * 16;
  if (q0 >= nq) return;  // the whole wave; no barrier below
  const float* rrow = r + (size_t)min(r0 + ml, nr - 1) * D;
  const float* qrow[NN_TQ];
#pragma unroll
  for (int t = 0; t < NN_TQ; ++t) qrow[t] = q + (size_t)min(q0 + t * 16 + ml, nq - 1) * D;
  f32x4 acc[NN_TQ];
#pragma unroll
  for (int t = 0; t < NN_TQ; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long long kbase = chunk * NN_CHUNK + kq * 4;
#pragma unroll 4
  for (int s = 0; s < NN_CHUNK / 16; ++s) {
    const long long k = kbase + s * 16;
    const f32x4 b = nn_load4<VEC>(rrow, k, D);
    f32x4 a[NN_TQ];
#pragma unroll
    for (int t = 0; t < NN_TQ; ++t) a[t] = nn_load4<VEC>(qrow[t], k, D);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int t = 0; t < NN_TQ; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][u], b[u], acc[t], 0, 0, 0);
    }
  }
  const long long j = r0 + ml;
#pragma unroll
  for (int t = 0; t < NN_TQ; ++t) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const long long i = q0 + t * 16 + kq * 4 + rr;
      if (i < nq && j < nr) part[((size_t)chunk * nq + i) * nr + j] = acc[t][rr];
    }
  }
}

// 16 pairs x 16 slices per workgroup: thread (pair = tid & 15, slice = tid >> 4)
__global__ void __launch_bounds__(256) nn_dist_k(const float* __restrict__ part, const double* __restrict__ qn,
                                                 const double* __restrict__ rn, double* __restrict__ dist, long long nq, long long nr,
                                                 long long nchunks) {
  __shared__ double red[256];
  const int tid = threadIdx.x, pl = tid & 15, sl = tid >> 4;
  const long long pairs = nq * nr, p = (long long)blockIdx.x * 16 + pl;
  double s = 0.0;
  if (p < pairs)
    for (long long c = sl; c < nchunks; c += NN_SLICES) s += (double)part[(size_t)c * pairs + p];
  red[tid] = s;
  __syncthreads();
  for (int h = NN_SLICES / 2; h >= 1; h >>= 1) {
    if (sl < h) red[tid] += red[tid + h * 16];
    __syncthreads();
  }
  if (sl == 0 && p < pairs) {
    const double d = qn[p / nr] + rn[p % nr] - 2.0 * red[pl];
    dist[p] = d > 0.0 ? d : 0.0;
  }
}

__device__ __forceinline__ bool nn_before(double d, long long id, double d2, long long id2) {
  return d < d2 || (d == d2 && id < id2);
}

__global__ void __launch_bounds__(64) nn_merge_k(const double* __restrict__ dist, const long long* __restrict__ qid,
                                                 const long long* __restrict__ rid, double* __restrict__ best_d,
                                                 long long* __restrict__ best_i, long long nq, long long nr, int k) {
  __shared__ double sd[NN_MAXK][64];
  __shared__ long long si[NN_MAXK][64];
  const int t = threadIdx.x;
  const long long qi = (long long)blockIdx.x * 64 + t;
  if (qi >= nq) return;  // no barrier below: a thread works on its own column of the lists
  for (int s = 0; s < k; ++s) {
    sd[s][t] = best_d[qi * k + s];
    si[s][t] = best_i[qi * k + s];
  }
  const long long own = qid ? qid[qi] : -1;
  for (long long j = 0; j < nr; ++j) {
    const double d = dist[qi * nr + j];
    const long long id = rid[j];
    if (own >= 0 && id == own) continue;
    if (!nn_before(d, id, sd[k - 1][t], si[k - 1][t])) continue;
    int s = k - 1;
    while (s > 0 && nn_before(d, id, sd[s - 1][t], si[s - 1][t])) {
      sd[s][t] = sd[s - 1][t];
      si[s][t] = si[s - 1][t];
      --s;
    }
    sd[s][t] = d;
    si[s][t] = id;
  }
  for (int s = 0; s < k; ++s) {
    best_d[qi * k + s] = sd[s][t];
    best_i[qi * k + s] = si[s][t];
  }
}

}  // namespace

extern "C" int mg_nn_chunk(void) { return NN_CHUNK; }

extern "C" size_t mg_nn_ws_bytes(int64_t nq, int64_t nr, int64_t D) {
  if (nq < 1 || nr < 1 || D < 1) return 0;
  return (size_t)nn_chunks(D) * (size_t)nq * (size_t)nr * sizeof(float);
}

extern "C" int mg_nn_sqnorm(const float* x, int64_t n, int64_t D, double* out, mg_stream_t stream) {
  MG_CHECK_ARG(x && out && n > 0 && D > 0, "mg_nn_sqnorm: bad arguments");
  MG_CHECK_ARG(n < (1ll << 31), "mg_nn_sqnorm: too many rows");
  hipLaunchKernelGGL(nn_sqnorm_k, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, x, out, (long long)D);
  MG_CHECK_LAUNCH("mg_nn_sqnorm");
  return MG_OK;
}

extern "C" int mg_nn_sqdist(const float* q, const float* r, const double* qn, const double* rn, int64_t nq, int64_t nr, int64_t D,
                            double* dist, void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(q && r && qn && rn && dist && ws && nq > 0 && nr > 0 && D > 0, "mg_nn_sqdist: bad arguments");
  const long long chunks = nn_chunks(D), qblocks = (nq + NN_QB - 1) / NN_QB, rtiles = (nr + 15) / 16;
  MG_CHECK_ARG(chunks < (1ll << 31) && qblocks <= 65535 && rtiles <= 65535 && nq * nr < (1ll << 34),
               "mg_nn_sqdist: %lld x %lld rows of %lld numbers are more than one launch takes", (long long)nq, (long long)nr,
               (long long)D);
  if (ws_bytes < mg_nn_ws_bytes(nq, nr, D)) {
    mg_set_error("mg_nn_sqdist: workspace too small");
    return MG_EWORKSPACE;
  }
  float* part = reinterpret_cast<float*>(ws);
  const dim3 grid((unsigned)chunks, (unsigned)qblocks, (unsigned)rtiles);
  const bool vec = D % 4 == 0 && ((reinterpret_cast<size_t>(q) | reinterpret_cast<size_t>(r)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(nn_dot_k<true>, grid, dim3(256), 0, (hipStream_t)stream, q, r, part, (long long)nq, (long long)nr, (long long)D);
  else
    hipLaunchKernelGGL(nn_dot_k<false>, grid, dim3(256), 0, (hipStream_t)stream, q, r, part, (long long)nq, (long long)nr,
                       (long long)D);
  hipLaunchKernelGGL(nn_dist_k, dim3((unsigned)((nq * nr + 15) / 16)), dim3(256), 0, (hipStream_t)stream, part, qn, rn, dist,
                     (long long)nq, (long long)nr, chunks);
  MG_CHECK_LAUNCH("mg_nn_sqdist");
  return MG_OK;
}

extern "C" int mg_nn_merge(const double* dist, const int64_t* qid, const int64_t* rid, double* best_d, int64_t* best_i, int64_t nq,
                           int64_t nr, int k, mg_stream_t stream) {
  MG_CHECK_ARG(dist && rid && best_d && best_i && nq > 0 && nr > 0, "mg_nn_merge: bad arguments");
  MG_CHECK_ARG(k >= 1 && k <= NN_MAXK, "mg_nn_merge: k in 1 .. %d expected, got %d", NN_MAXK, k);
  MG_CHECK_ARG(nq < (1ll << 36), "mg_nn_merge: too many queries");
  hipLaunchKernelGGL(nn_merge_k, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, (hipStream_t)stream, dist,
                     reinterpret_cast<const long long*>(qid), reinterpret_cast<const long long*>(rid), best_d,
                     reinterpret_cast<long long*>(best_i), (long long)nq, (long long)nr, k);
  MG_CHECK_LAUNCH("mg_nn_merge");
  return MG_OK;
}
