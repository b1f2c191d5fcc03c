// Median selection for csrc/hpss.hip, on the bit patterns of non-negative float32 values taken as unsigned integers (the order of
// the values; a NaN is just a large key, so every input is a permutation problem and nothing can fault or be lost).
//
//   median<N>   the middle one of N - 1 keys held in registers (N = 32 or 64): Batcher's odd-even merge sort for N inputs (191 / 543
//               comparators), the N-th input being the largest key.  The comparator list is a constant expression and is applied
//               through a fold over an index sequence, so every array index is a literal: the array lives in registers, nothing goes
//               to scratch memory, and the comparators that the wanted output does not depend on are dropped by the compiler.
//               A window of an odd length L < N - 1 is padded with (N - 1 - L) / 2 smallest and as many largest keys: the middle
//               key of the N - 1 is then the middle key of the L.
//   reflect     scipy.ndimage's mode='reflect' (d c b a | a b c d | d c b a): index j on an axis of n -> r = j mod 2 n, r < n ? r :
//               2 n - 1 - r; folds as often as it has to.
//
// Device code; the CPU test compiles the same text with g++ (HPSS_FN defined as `static inline`).
#pragma once
#include <cstdint>
#include <utility>

#ifndef HPSS_FN
#define HPSS_FN __device__ __forceinline__
#endif

namespace hpss {

constexpr uint32_t KEY_MIN = 0u, KEY_MAX = 0xFFFFFFFFu;

struct Network {
  int n;
  int lo[543], hi[543];
};

constexpr Network make_network(int n) {
  Network r{};
  for (int p = 1; p < n; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j <= n - 1 - k; j += 2 * k)
        for (int i = 0; i <= (k - 1 < n - j - k - 1 ? k - 1 : n - j - k - 1); ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            r.lo[r.n] = i + j;
            r.hi[r.n] = i + j + k;
            ++r.n;
          }
  return r;
}

template <int N>
struct Sorter {
  static_assert(N == 32 || N == 64, "networks for 32 and 64 inputs are built");
  static constexpr Network NET = make_network(N);
  static constexpr int COUNT = N == 32 ? 191 : 543;
  static_assert(NET.n == COUNT, "odd-even merge sort: 191 comparators for 32 inputs, 543 for 64");
};

template <int N, int C>
HPSS_FN void compare_exchange(uint32_t (&a)[N]) {
  constexpr int i = Sorter<N>::NET.lo[C], j = Sorter<N>::NET.hi[C];
  const uint32_t x = a[i], y = a[j];
  a[i] = x < y ? x : y;
  a[j] = x < y ? y : x;
}

template <int N, int... C>
HPSS_FN void run_network(uint32_t (&a)[N], std::integer_sequence<int, C...>) {
  (compare_exchange<N, C>(a), ...);
}

// a[0 .. N-2]: the keys (a[N-1] is overwritten); returns the middle one, the (N/2)-th smallest
template <int N>
HPSS_FN uint32_t median(uint32_t (&a)[N]) {
  a[N - 1] = KEY_MAX;
  run_network(a, std::make_integer_sequence<int, Sorter<N>::COUNT>{});
  return a[N / 2 - 1];
}

HPSS_FN long long reflect(long long j, long long n) {
  long long r = j % (2 * n);
  if (r < 0) r += 2 * n;
  return r < n ? r : 2 * n - 1 - r;
}

}  // namespace hpss
