// Float64 mean and covariance of float32 rows: the kernels behind mel_ops.moments and metrics.Frechet.
//
//   mean_j = (sum_i x_ij) / n;   cov_jk = sum_i (x_ij - mean_j)(x_ik - mean_k) / (n - 1)      two passes, all float64
//
// The rows are cut into chunks of MO_CHUNK; a chunk's sums start from +0.0 and take its rows in ascending order, and a second launch
// adds the chunk sums in chunk order: every sum is a function of (n, d) and the rows alone, bit for bit from run to run.
//   mean     a thread per column walks its chunk; then a thread per column adds the chunks and divides by n.
//   cov      a workgroup per (pair of 32-column tiles bj <= bk, chunk): slabs of 32 rows, centred in float64, go through LDS and
//            every thread keeps 2 x 2 sums.  Tiles below the diagonal are not computed: the finishing launch, a thread per element of
//            the full matrix, reads the partial of (min(j, k), max(j, k)), so cov[j,k] and cov[k,j] hold the same bits.
// Not a hot path (2 G multiply-adds at 8192 x 512): no matrix cores, no atomics.
#include "mg_common.h"

namespace {

constexpr int MO_CHUNK = 1024;   // rows per partial sum: a compile-time constant, part of the definition of the bits
constexpr int MO_TILE = 32;      // columns of a covariance tile, and rows of a slab
constexpr int MO_MAX_D = 4096;
constexpr long long MO_MAX_N = 1ll << 24;

__global__ void __launch_bounds__(256) mo_mean_partial_k(const float* __restrict__ x, double* __restrict__ part, long long n, int d) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  const long long r0 = (long long)blockIdx.y * MO_CHUNK, r1 = r0 + MO_CHUNK < n ? r0 + MO_CHUNK : n;
  double s = 0.0;
  for (long long r = r0; r < r1; ++r) s += (double)x[(size_t)r * d + col];
  part[(size_t)blockIdx.y * d + col] = s;
}

__global__ void __launch_bounds__(256) mo_mean_finish_k(const double* __restrict__ part, double* __restrict__ mean, long long n, int d,
                                                        int chunks) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  if (col >= d) return;
  double s = part[col];
  for (int c = 1; c < chunks; ++c) s += part[(size_t)c * d + col];
  mean[col] = s / (double)n;
}

__global__ void __launch_bounds__(256) mo_cov_partial_k(const float* __restrict__ x, const double* __restrict__ mean,
                                                        double* __restrict__ part, long long n, int d, int tiles) {
  __shared__ double a[MO_TILE][MO_TILE], b[MO_TILE][MO_TILE];
  // blockIdx.x numbers the pairs bj <= bk row by row: row bj holds tiles - bj of them
  int bj = 0, rest = blockIdx.x;
  while (rest >= tiles - bj) {
    rest -= tiles - bj;
    ++bj;
  }
  const int bk = bj + rest, j0 = bj * MO_TILE, k0 = bk * MO_TILE;
  const int tid = threadIdx.x, ty = (tid >> 4) * 2, tx = (tid & 15) * 2;
  const long long r0 = (long long)blockIdx.y * MO_CHUNK, r1 = r0 + MO_CHUNK < n ? r0 + MO_CHUNK : n;
  double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0;
  for (long long base = r0; base < r1; base += MO_TILE) {
    const int rows = (int)(r1 - base < MO_TILE ? r1 - base : MO_TILE);
#pragma unroll
    for (int q = 0; q < MO_TILE * MO_TILE / 256; ++q) {
      const int e = tid + 256 * q, r = e / MO_TILE, cc = e % MO_TILE;
      const bool in = r < rows;
      const size_t row = (size_t)(base + (in ? r : 0)) * d;
      a[r][cc] = in && j0 + cc < d ? (double)x[row + j0 + cc] - mean[j0 + cc] : 0.0;
      b[r][cc] = in && k0 + cc < d ? (double)x[row + k0 + cc] - mean[k0 + cc] : 0.0;
    }
    __syncthreads();
    for (int r = 0; r < rows; ++r) {   // ascending rows
      const double a0 = a[r][ty], a1 = a[r][ty + 1], b0 = b[r][tx], b1 = b[r][tx + 1];
      s00 += a0 * b0;
      s01 += a0 * b1;
      s10 += a1 * b0;
      s11 += a1 * b1;
    }
    __syncthreads();
  }
  double* out = part + (size_t)blockIdx.y * d * d;
  const int j = j0 + ty, k = k0 + tx;
  if (j < d && k < d) out[(size_t)j * d + k] = s00;
  if (j < d && k + 1 < d) out[(size_t)j * d + k + 1] = s01;
  if (j + 1 < d && k < d) out[(size_t)(j + 1) * d + k] = s10;
  if (j + 1 < d && k + 1 < d) out[(size_t)(j + 1) * d + k + 1] = s11;
}

__global__ void __launch_bounds__(256) mo_cov_finish_k(const double* __restrict__ part, double* __restrict__ cov, long long n, int d,
                                                       int chunks) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, dd = (size_t)d * d;
  if (e >= dd) return;
  const int j = (int)(e / d), k = (int)(e % d);
  const double* p = part + (size_t)(j < k ? j : k) * d + (j < k ? k : j);   // the element on or above the diagonal
  double s = p[0];
  for (int c = 1; c < chunks; ++c) s += p[(size_t)c * dd];
  cov[e] = s / (double)(n - 1);
}

long long mo_chunks(long long n) { return (n + MO_CHUNK - 1) / MO_CHUNK; }

}  // namespace

extern "C" size_t mg_moments_ws_bytes(int64_t n, int64_t d) {
  if (n < 2 || n > MO_MAX_N || d < 1 || d > MO_MAX_D) return 0;
  return (size_t)mo_chunks(n) * (size_t)(d + d * d) * sizeof(double);
}

extern "C" int mg_moments(const float* rows, int64_t n, int64_t d, double* mean, double* cov, void* ws, size_t ws_bytes,
                          mg_stream_t stream) {
  MG_CHECK_ARG(rows && mean && cov && ws, "mg_moments: bad arguments");
  MG_CHECK_ARG(n >= 2 && n <= MO_MAX_N, "mg_moments: 2 .. %lld rows expected, got %lld", MO_MAX_N, (long long)n);
  MG_CHECK_ARG(d >= 1 && d <= MO_MAX_D, "mg_moments: 1 .. %d numbers per row expected, got %lld", MO_MAX_D, (long long)d);
  MG_CHECK_ARG((reinterpret_cast<size_t>(ws) & 7) == 0, "mg_moments: the workspace must be 8-byte aligned");
  if (ws_bytes < mg_moments_ws_bytes(n, d)) {
    mg_set_error("mg_moments: workspace too small");
    return MG_EWORKSPACE;
  }
  const int chunks = (int)mo_chunks(n), di = (int)d, tiles = (di + MO_TILE - 1) / MO_TILE;
  double* mean_part = reinterpret_cast<double*>(ws);
  double* cov_part = mean_part + (size_t)chunks * di;
  const unsigned cols = (unsigned)((di + 255) / 256);
  hipLaunchKernelGGL(mo_mean_partial_k, dim3(cols, (unsigned)chunks), dim3(256), 0, (hipStream_t)stream, rows, mean_part, (long long)n,
                     di);
  hipLaunchKernelGGL(mo_mean_finish_k, dim3(cols), dim3(256), 0, (hipStream_t)stream, mean_part, mean, (long long)n, di, chunks);
  hipLaunchKernelGGL(mo_cov_partial_k, dim3((unsigned)(tiles * (tiles + 1) / 2), (unsigned)chunks), dim3(256), 0, (hipStream_t)stream,
                     rows, mean, cov_part, (long long)n, di, tiles);
  hipLaunchKernelGGL(mo_cov_finish_k, dim3((unsigned)(((size_t)di * di + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cov_part, cov,
                     (long long)n, di, chunks);
  MG_CHECK_LAUNCH("mg_moments");
  return MG_OK;
}
