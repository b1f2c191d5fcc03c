// Deterministic k-means for NDB / JSD (Richardson & Weiss, NeurIPS 2018): the kernels behind musicgan_amd/km_ops.py and
// metrics.KMeans / metrics.NDB.  Definitions and the determinism argument: DESIGN.md 4.15.  The distances of a Lloyd iteration come
// from csrc/prdc.hip (mg_nn_sqdist_tiled); this file is the other half.
//
//   assign   one wave per row of a float64 distance block, lanes striding the columns: the smallest entry and its column, ties to
//            the smaller column, through a butterfly on (value, column).  A wave walks rows w, w + waves, ... and counts the labels
//            it rewrites with another value; one integer atomic per wave adds that to `changed`, which a one-thread launch zeroed.
//   order    a stable counting sort of the positions by label without a workspace.  hist: ONE workgroup counts the labels in LDS
//            (integer atomics) and scans the k counts into start[0 .. k].  place: one wave per bin walks all n labels in ascending
//            position, 64 at a time (KM_PLACE such groups loaded ahead); a ballot gives every matching lane its rank, so a bin's
//            positions come out ascending whatever the other bins hold.  Wave k gathers the positions whose label is outside 0 .. k-1 behind start[k], so that every
//            element of `order` is written whatever `label` holds.
//   update   partial: bin j's ordered member list is cut into chunks of KM_CHUNK members; chunk c of bin j owns slot
//            start[j] / KM_CHUNK + j + c of the workspace (slots of different bins never overlap: floor((s + m) / C) + 1 >=
//            floor(s / C) + ceil(m / C); a workgroup finds its bin by bisection on that increasing sequence, an unused slot exits).
//            A thread owns 4 consecutive components and adds the chunk's members to 4 float64 sums from +0.0 in list order.
//            finish: one thread per (bin, component) adds the bin's chunk sums in chunk order, divides by the member count in
//            float64 and rounds once to float32.  An empty bin is not touched.  The sum of a component is therefore a function of
//            the bin's ordered member list and of KM_CHUNK alone: not of k, of the grid, or of what the other bins hold.
//   count    bin sizes of a label vector added to int64 counters: a histogram per workgroup in LDS, then one integer atomic per
//            non-empty bin and workgroup.
#include <cmath>

#include "nn_common.h"

namespace {

constexpr int KM_MAX_K = 1024;
constexpr long long KM_MAX_N = 1ll << 20;
constexpr int KM_CHUNK = 32;   // members per partial sum: a compile-time constant, part of the definition of the update's bits
constexpr int KM_LOADS = 8;    // rows a thread of the update has in flight (no part of the result)
constexpr int KM_PLACE = 4;    // groups of 64 labels a wave of the ordering has in flight

__global__ void km_zero_k(unsigned long long* __restrict__ v) { *v = 0ull; }

__global__ void __launch_bounds__(256) km_assign_k(const double* __restrict__ dist, int* __restrict__ label, double* __restrict__ mind,
                                                   unsigned long long* __restrict__ changed, long long n, int k) {
  const int lane = threadIdx.x & 63;
  const long long waves = (long long)gridDim.x * 4;
  int diff = 0;   // lane 0's count
  for (long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += waves) {   // the whole wave; no barrier below
    const double* d = dist + (size_t)row * k;
    double m = INFINITY;
    int c = 0x7fffffff;
    for (int j = lane; j < k; j += 64) {
      const double v = d[j];
      if (v < m || (v == m && j < c)) {
        m = v;
        c = j;
      }
    }
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
      const double om = __shfl_xor(m, x);
      const int oc = __shfl_xor(c, x);
      if (om < m || (om == m && oc < c)) {
        m = om;
        c = oc;
      }
    }
    if (lane == 0) {
      if (c >= k) {   // a row of NaN: no entry compares; column 0, as an index that is always inside
        c = 0;
        m = d[0];
      }
      diff += label[row] != c ? 1 : 0;
      label[row] = c;
      mind[row] = m;
    }
  }
  if (lane == 0 && diff) atomicAdd(changed, (unsigned long long)diff);
}

__global__ void __launch_bounds__(1024) km_hist_k(const int* __restrict__ label, int* __restrict__ start, int n, int k) {
  __shared__ int h[KM_MAX_K + 1];   // h[k]: labels outside 0 .. k-1
  __shared__ int s[KM_MAX_K];
  const int tid = threadIdx.x;
  h[tid] = 0;
  if (tid == 0) h[KM_MAX_K] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += 1024) {
    const int l = label[i];
    atomicAdd(&h[l >= 0 && l < k ? l : k], 1);
  }
  __syncthreads();
  s[tid] = tid < k ? h[tid] : 0;
  __syncthreads();
  for (int off = 1; off < KM_MAX_K; off <<= 1) {   // inclusive scan
    const int v = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += v;
    __syncthreads();
  }
  if (tid < k) start[tid + 1] = s[tid];
  if (tid == 0) start[0] = 0;
}

__global__ void __launch_bounds__(256) km_place_k(const int* __restrict__ label, const int* __restrict__ start,
                                                  int* __restrict__ order, int n, int k) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j > k) return;   // the whole wave
  int base = start[j < k ? j : k];
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int i0 = 0; i0 < n; i0 += 64 * KM_PLACE) {   // KM_PLACE loads in flight, consumed in ascending position
    int l[KM_PLACE];
#pragma unroll
    for (int u = 0; u < KM_PLACE; ++u) {
      const int i = i0 + 64 * u + lane;
      l[u] = i < n ? label[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < KM_PLACE; ++u) {
      const int i = i0 + 64 * u + lane;
      const bool match = i < n && (j < k ? l[u] == j : (l[u] < 0 || l[u] >= k));
      const unsigned long long b = __ballot(match);
      const int pos = base + __popcll(b & below);
      if (match && pos < n) order[pos] = i;
      base += __popcll(b);
    }
  }
}

__device__ __forceinline__ int km_slot(int s, int j) { return s / KM_CHUNK + j; }

template <bool VEC>
__global__ void __launch_bounds__(256) km_partial_k(const float* __restrict__ x, const int* __restrict__ order,
                                                    const int* __restrict__ start, double* __restrict__ ws, int n, long long D, int k) {
  const int slot = blockIdx.y;
  int lo = 0, hi = k - 1;   // the last bin whose first slot is <= slot
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (km_slot(start[mid], mid) <= slot) lo = mid;
    else hi = mid - 1;
  }
  const int s0 = start[lo], m = start[lo + 1] - s0, c = slot - km_slot(s0, lo);
  if (c < 0 || (long long)c * KM_CHUNK >= m) return;   // a slot no chunk owns
  const int first = s0 + c * KM_CHUNK, cnt = min(KM_CHUNK, m - c * KM_CHUNK);
  const long long col = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (s0 < 0 || first + cnt > n || col >= D) return;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  for (int t0 = 0; t0 < cnt; t0 += KM_LOADS) {   // KM_LOADS rows in flight per thread, added in list order
    f32x4 v[KM_LOADS];
#pragma unroll
    for (int u = 0; u < KM_LOADS; ++u) {
      const int row = order[first + min(t0 + u, cnt - 1)];   // past the chunk's end: its last row again, loaded and not added
      v[u] = nn_load4<VEC>(x + (size_t)((unsigned)row < (unsigned)n ? row : 0) * D, col, D);   // (a row outside x: never with km_place_k's order)
    }
#pragma unroll
    for (int u = 0; u < KM_LOADS; ++u) {
      if (t0 + u < cnt) {
        a0 += (double)v[u][0];
        a1 += (double)v[u][1];
        a2 += (double)v[u][2];
        a3 += (double)v[u][3];
      }
    }
  }
  double* out = ws + (size_t)slot * D + col;
  out[0] = a0;
  if (col + 1 < D) out[1] = a1;
  if (col + 2 < D) out[2] = a2;
  if (col + 3 < D) out[3] = a3;
}

__global__ void __launch_bounds__(256) km_finish_k(const double* __restrict__ ws, const int* __restrict__ start,
                                                   float* __restrict__ centroid, long long D) {
  const int j = blockIdx.y;
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  const int s0 = start[j], m = start[j + 1] - s0;
  if (m <= 0 || col >= D) return;   // an empty bin keeps its centroid
  const int chunks = (m + KM_CHUNK - 1) / KM_CHUNK;
  const double* p = ws + (size_t)km_slot(s0, j) * D + col;
  double s = p[0];
  for (int c = 1; c < chunks; ++c) s += p[(size_t)c * D];
  centroid[(size_t)j * D + col] = (float)(s / (double)m);
}

__global__ void __launch_bounds__(256) km_count_k(const int* __restrict__ label, unsigned long long* __restrict__ count, long long n,
                                                  int k) {
  __shared__ int h[KM_MAX_K];
  for (int j = threadIdx.x; j < k; j += 256) h[j] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int l = label[i];
    if (l >= 0 && l < k) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  for (int j = threadIdx.x; j < k; j += 256) {
    if (h[j]) atomicAdd(&count[j], (unsigned long long)h[j]);
  }
}

long long km_slots(long long n, long long k) { return n / KM_CHUNK + k; }

}  // namespace

extern "C" int mg_km_assign(const double* dist, int64_t n, int k, int32_t* label, double* mind, int64_t* changed, mg_stream_t stream) {
  MG_CHECK_ARG(dist && label && mind && changed && n > 0, "mg_km_assign: bad arguments");
  MG_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "mg_km_assign: k in 1 .. %d expected, got %d", KM_MAX_K, k);
  MG_CHECK_ARG(n < (1ll << 40), "mg_km_assign: %lld rows are more than one launch takes", (long long)n);
  unsigned long long* ch = reinterpret_cast<unsigned long long*>(changed);
  hipLaunchKernelGGL(km_zero_k, dim3(1), dim3(1), 0, (hipStream_t)stream, ch);
  const long long blocks = (n + 3) / 4;
  hipLaunchKernelGGL(km_assign_k, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, dist, label,
                     mind, ch, (long long)n, k);
  MG_CHECK_LAUNCH("mg_km_assign");
  return MG_OK;
}

extern "C" int mg_km_order(const int32_t* label, int64_t n, int k, int32_t* start, int32_t* order, mg_stream_t stream) {
  MG_CHECK_ARG(label && start && order && n > 0, "mg_km_order: bad arguments");
  MG_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "mg_km_order: k in 1 .. %d expected, got %d", KM_MAX_K, k);
  MG_CHECK_ARG(n <= KM_MAX_N, "mg_km_order: at most %lld points expected, got %lld", KM_MAX_N, (long long)n);
  hipLaunchKernelGGL(km_hist_k, dim3(1), dim3(1024), 0, (hipStream_t)stream, label, start, (int)n, k);
  hipLaunchKernelGGL(km_place_k, dim3((unsigned)((k + 1 + 3) / 4)), dim3(256), 0, (hipStream_t)stream, label, start, order, (int)n, k);
  MG_CHECK_LAUNCH("mg_km_order");
  return MG_OK;
}

extern "C" size_t mg_km_update_ws_bytes(int64_t n, int64_t d, int k) {
  if (n < 1 || d < 1 || k < 1) return 0;
  return (size_t)km_slots(n, k) * (size_t)d * sizeof(double);
}

extern "C" int mg_km_update(const float* x, int64_t n, int64_t d, const int32_t* order, const int32_t* start, int k, float* centroid,
                            void* ws, size_t ws_bytes, mg_stream_t stream) {
  MG_CHECK_ARG(x && order && start && centroid && ws && n > 0 && d > 0, "mg_km_update: bad arguments");
  MG_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "mg_km_update: k in 1 .. %d expected, got %d", KM_MAX_K, k);
  MG_CHECK_ARG(n <= KM_MAX_N && d < (1ll << 40), "mg_km_update: %lld rows of %lld numbers are more than one launch takes",
               (long long)n, (long long)d);
  MG_CHECK_ARG((reinterpret_cast<size_t>(ws) & 7) == 0, "mg_km_update: the workspace must be 8-byte aligned");
  if (ws_bytes < mg_km_update_ws_bytes(n, d, k)) {
    mg_set_error("mg_km_update: workspace too small");
    return MG_EWORKSPACE;
  }
  double* sums = reinterpret_cast<double*>(ws);
  const dim3 grid((unsigned)((d + 1023) / 1024), (unsigned)km_slots(n, k));   // at most 2^20 / 32 + 1024 slots
  const bool vec = d % 4 == 0 && (reinterpret_cast<size_t>(x) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(km_partial_k<true>, grid, dim3(256), 0, (hipStream_t)stream, x, order, start, sums, (int)n, (long long)d, k);
  else
    hipLaunchKernelGGL(km_partial_k<false>, grid, dim3(256), 0, (hipStream_t)stream, x, order, start, sums, (int)n, (long long)d, k);
  hipLaunchKernelGGL(km_finish_k, dim3((unsigned)((d + 255) / 256), (unsigned)k), dim3(256), 0, (hipStream_t)stream, sums, start,
                     centroid, (long long)d);
  MG_CHECK_LAUNCH("mg_km_update");
  return MG_OK;
}

extern "C" int mg_km_count(const int32_t* label, int64_t n, int k, int64_t* count, mg_stream_t stream) {
  MG_CHECK_ARG(label && count && n > 0, "mg_km_count: bad arguments");
  MG_CHECK_ARG(k >= 1 && k <= KM_MAX_K, "mg_km_count: k in 1 .. %d expected, got %d", KM_MAX_K, k);
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(km_count_k, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, (hipStream_t)stream, label,
                     reinterpret_cast<unsigned long long*>(count), (long long)n, k);
  MG_CHECK_LAUNCH("mg_km_count");
  return MG_OK;
}
