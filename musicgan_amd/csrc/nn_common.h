// What the two evaluations of the squared-distance matrix (csrc/nn.hip: one wave per chunk, csrc/prdc.hip: LDS-staged tiles) share:
// the chunk of components a float32 chain covers, the number of float64 slices the chunks are dealt into, and the operand load.
// Both files give the same bits only as long as they agree on all three.
#pragma once
#include "mg_common.h"

constexpr int NN_CHUNK = 256;                  // components one wave accumulates in float32
constexpr int NN_SLICES = 16;                  // slice s adds the chunks s, s + 16, ... in float64

// 4 consecutive components of a row from k on; zero from D on.  VEC: D % 4 == 0 and 16-byte aligned rows, so k < D covers all four.
template <bool VEC>
__device__ __forceinline__ f32x4 nn_load4(const float* __restrict__ row, long long k, long long D) {
  if constexpr (VEC) {
    return k < D ? *reinterpret_cast<const f32x4*>(row + k) : f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    f32x4 v;
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = k + u < D ? row[k + u] : 0.f;
    return v;
  }
}

static inline long long nn_chunks(long long D) { return (D + NN_CHUNK - 1) / NN_CHUNK; }
