// The Ogg page checksum (CRC-32, polynomial 0x04C11DB7, init 0, MSB first, no final xor) for the page kernels of vorbis.hip and
// vorbis_encode.hip.  Plain C++ over byte pointers, marked host+device, so the chunk-combining arithmetic also runs in a host
// build: a page of `len` bytes is cut into `nlanes` chunks, each lane takes the CRC of its chunk and shifts it past the bytes
// that follow with a GF(2) multiply, and the page's CRC is the xor of the lanes' parts.
#ifndef MG_OGG_CRC_H
#define MG_OGG_CRC_H

#include <stdint.h>

#ifndef OGG_HD
#define OGG_HD __host__ __device__ inline
#endif

namespace ogg {

constexpr uint32_t OGG_POLY = 0x04C11DB7u;

OGG_HD uint32_t crc_table_entry(uint32_t i) {
  uint32_t r = i << 24;
  for (int k = 0; k < 8; ++k) r = (r & 0x80000000u) ? (r << 1) ^ OGG_POLY : (r << 1);
  return r;
}

OGG_HD uint32_t gf2_mulmod(uint32_t a, uint32_t b) {  // a * b mod the Ogg polynomial (both as 32-bit remainders)
  uint32_t r = 0;
  for (int i = 31; i >= 0; --i) {
    r = (r << 1) ^ ((r >> 31) ? OGG_POLY : 0u);
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}

OGG_HD uint32_t xpow8(int64_t k) {  // x^(8k) mod P
  uint32_t r = 1u, sq = 1u << 8;    // x^0, x^8
  while (k) {
    if (k & 1) r = gf2_mulmod(r, sq);
    sq = gf2_mulmod(sq, sq);
    k >>= 1;
  }
  return r;
}

// Lane `lane`'s part of the CRC of the page p[0, len), T[i] = crc_table_entry(i).  The page's own CRC field, bytes 22 .. 25, reads
// as zero, as the format defines the checksum.  Lanes whose chunk lies past the end contribute 0.
OGG_HD uint32_t page_crc_part(const uint8_t* p, int64_t len, int lane, int nlanes, const uint32_t* T) {
  const int64_t chunk = (len + nlanes - 1) / nlanes;
  const int64_t a = (int64_t)lane * chunk, b = a + chunk < len ? a + chunk : len;
  if (a >= b) return 0;
  uint32_t c = 0;
  for (int64_t i = a; i < b; ++i) {
    const uint32_t byte = (i >= 22 && i < 26) ? 0u : p[i];
    c = (c << 8) ^ T[((c >> 24) ^ byte) & 0xFF];
  }
  return b < len ? gf2_mulmod(c, xpow8(len - b)) : c;  // shift past the bytes after this chunk
}

#ifdef __HIPCC__
// One workgroup's page CRC (thread t of NT, LDS: T[256], part[NT / 64]); the result is valid in thread 0.  The page's bytes must
// be visible to the workgroup before the call.
template <int NT>
__device__ __forceinline__ uint32_t page_crc_block(const uint8_t* p, int64_t len, int t, uint32_t* T, uint32_t* part) {
  static_assert(NT >= 256 && NT % 64 == 0, "every table entry needs a thread");
  if (t < 256) T[t] = crc_table_entry((uint32_t)t);
  __syncthreads();
  uint32_t c = page_crc_part(p, len, t, NT, T);
  for (int s = 32; s >= 1; s >>= 1) c ^= (uint32_t)__shfl_xor((int)c, s, 64);
  if ((t & 63) == 0) part[t >> 6] = c;
  __syncthreads();
  uint32_t x = 0;
  if (t == 0)
    for (int w = 0; w < NT / 64; ++w) x ^= part[w];
  return x;
}
#endif

}  // namespace ogg

#endif
