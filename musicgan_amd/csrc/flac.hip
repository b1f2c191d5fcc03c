// FLAC decoding (RFC 9639) on the device: what torchaudio.load does for a .flac input (the reference's
// audio/functions.py:43, th_audio.load).  The host parses the metadata blocks (musicgan_amd/audio/flac.py) and hands over the
// audio region -- the bytes from the first frame header to the end -- zero padded to mg_flac_padded_bytes.
//
// Pipeline, every step a launch on the caller's stream, nothing read back in between:
//   1. scan (count, offsets, write): every byte offset is tested for a frame header -- sync code, valid fields, CRC-8 -- and the
//      candidates are written compacted, in offset order.  One thread per 16 bytes; bound by reading the region.
//   2. chain (one workgroup): frame 0 starts at byte 0; frame n + 1 is the first candidate after frame n that carries the
//      expected number (n + 1, or first sample + block size for variable blocking).  Writes the frame table.
//   3. decode (one wave per frame, flac_core.h): subframes, Rice residuals, prediction, CRC-16, decorrelation, output.
//   4. finalize (one thread): the first frame with a problem, for the host's single status read.
// A sync pattern inside compressed data that passes every header check is taken by the chain as a frame; the decoded end of the
// frame in front of it then disagrees with it (F_END) and the host resumes the chain at the decoded end (mg_flac_rechain).
#include "mg_common.h"

#include "flac_core.h"

namespace {

using flac::Cand;
using flac::Frame;

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_BYTES = 16;  // bytes per thread
constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_BYTES;
constexpr int CHAIN_THREADS = 256;
constexpr int CHAIN_WIN = 2048;  // candidates staged per window (32 KiB of LDS)
constexpr int DECODE_GRID_MAX = 256 * 16;

struct Layout {
  int64_t nchunks;
  size_t counts, offs, cands, frames, total;
};

Layout layout(int64_t nbytes, int64_t cap) {
  Layout l;
  l.nchunks = (nbytes + SCAN_CHUNK - 1) / SCAN_CHUNK;
  l.counts = flac::S_COUNT * 8;
  l.offs = l.counts + ((size_t)l.nchunks * 4 + 15) / 16 * 16;
  l.cands = l.offs + ((size_t)l.nchunks * 4 + 15) / 16 * 16;
  l.frames = l.cands + (size_t)cap * sizeof(Cand);
  l.total = l.frames + (size_t)cap * sizeof(Frame);
  return l;
}

// wave-uniform block-wide exclusive prefix of one value per thread (blockDim.x == SCAN_THREADS); also returns the total
__device__ uint32_t block_exclusive(uint32_t v, uint32_t* total) {
  __shared__ uint32_t s[SCAN_THREADS];
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < SCAN_THREADS; d <<= 1) {
    const uint32_t a = t >= d ? s[t - d] : 0;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  *total = s[SCAN_THREADS - 1];
  const uint32_t r = s[t] - v;
  __syncthreads();
  return r;
}

template <bool WRITE>
__global__ void __launch_bounds__(SCAN_THREADS) flac_scan_k(const uint8_t* __restrict__ d, int64_t n, uint32_t* __restrict__ counts,
                                                          const uint32_t* __restrict__ offs, Cand* __restrict__ cands, int64_t cap) {
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_BYTES;
  uint32_t w[5];
  // 16 bytes and the first word after them: the region is padded, so these loads stay inside the buffer
  const uint4 q = *reinterpret_cast<const uint4*>(d + base);
  w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
  w[4] = *reinterpret_cast<const uint32_t*>(d + base + 16);
  uint32_t hits = 0;  // bit j: a header starts at base + j
#pragma unroll
  for (int j = 0; j < SCAN_BYTES; ++j) {
    const uint32_t b0 = (w[j >> 2] >> (8 * (j & 3))) & 0xFF, b1 = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFF;
    if (b0 == 0xFF && (b1 & 0xFE) == 0xF8 && base + j < n) hits |= 1u << j;
  }
  flac::Hdr h[1];
  uint32_t valid = 0;
  for (uint32_t m = hits; m; m &= m - 1) {
    const int j = __builtin_ctz(m);
    if (flac::parse_header(d, n, base + j, h)) valid |= 1u << j;
  }
  uint32_t total;
  uint32_t at = block_exclusive((uint32_t)__builtin_popcount(valid), &total);
  if (!WRITE) {
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
    return;
  }
  int64_t idx = (int64_t)offs[blockIdx.x] + at;
  for (uint32_t m = valid; m; m &= m - 1, ++idx) {
    const int j = __builtin_ctz(m);
    flac::parse_header(d, n, base + j, h);
    if (idx < cap) {
      Cand c;
      c.off = (uint32_t)(base + j);
      c.num_lo = (uint32_t)h->num;
      c.num_hi = (uint32_t)(h->num >> 32);
      c.bs_blk = (uint32_t)h->bs | (uint32_t)h->blocking << 16;
      cands[idx] = c;
    }
  }
}

__global__ void __launch_bounds__(1024) flac_offsets_k(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offs,
                                                     int64_t nchunks, int64_t* __restrict__ st) {
  __shared__ uint32_t s[1024];
  __shared__ uint64_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (int64_t b = 0; b < nchunks; b += 1024) {
    const uint32_t v = b + t < nchunks ? counts[b + t] : 0;
    s[t] = v;
    __syncthreads();
    for (int dd = 1; dd < 1024; dd <<= 1) {
      const uint32_t a = t >= dd ? s[t - dd] : 0;
      __syncthreads();
      s[t] += a;
      __syncthreads();
    }
    const uint64_t c0 = carry;
    if (b + t < nchunks) offs[b + t] = (uint32_t)(c0 + s[t] - v);
    __syncthreads();
    if (t == 0) carry = c0 + s[1023];
    __syncthreads();
  }
  if (t == 0) st[flac::S_NCAND] = (int64_t)carry;
}

__device__ inline uint64_t cand_num(const Cand& c) { return (uint64_t)c.num_hi << 32 | c.num_lo; }

// frame table from frame `f0` on, starting at byte `off0` (f0 == 0: byte 0); frames in front of f0 are kept
__global__ void __launch_bounds__(CHAIN_THREADS) flac_chain_k(const Cand* __restrict__ cands, Frame* __restrict__ frames,
                                                            int64_t* __restrict__ st, int64_t n, int64_t cap, int64_t f0,
                                                            int64_t off0) {
  __shared__ Cand win[CHAIN_WIN];
  __shared__ int64_t s_f, s_scan, s_done, s_first, s_blk, s_cur_off, s_cur_bs;
  const int t = threadIdx.x;
  const int64_t ncand = st[flac::S_NCAND];
  if (t == 0) {
    st[flac::S_CHAIN_ERR] = flac::CHAIN_OK;
    st[flac::S_FIRST_BAD] = INT64_MAX;
    s_done = 0;
    s_f = f0;
    s_first = 0;
    if (f0 > 0) {
      s_first = (int64_t)(frames[f0 - 1].first + frames[f0 - 1].bs);
      frames[f0 - 1].next = (uint32_t)off0;  // the frame in front ends where the chain resumes
    }
    if (ncand > cap) {
      st[flac::S_CHAIN_ERR] = flac::CHAIN_OVERFLOW;
      s_f = 0;
      s_done = 1;
    } else if (off0 >= n) {
      s_done = 1;
    } else {
      int64_t lo = 0, hi = ncand;  // first candidate with off >= off0
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)cands[mid].off < off0) lo = mid + 1;
        else hi = mid;
      }
      const int blk = lo < ncand ? (int)(cands[lo].bs_blk >> 16) : 0;
      if (f0 == 0) st[flac::S_BLOCKING] = blk;
      const uint64_t want = blk ? (uint64_t)s_first : (uint64_t)f0;
      if (lo >= ncand || (int64_t)cands[lo].off != off0 || blk != st[flac::S_BLOCKING] || cand_num(cands[lo]) != want) {
        st[flac::S_CHAIN_ERR] = flac::CHAIN_NO_HEADER;
        st[flac::S_ERR_FRAME] = f0;
        st[flac::S_ERR_OFF] = off0;
        s_done = 1;
      } else {
        s_blk = blk;
        s_cur_off = cands[lo].off;
        s_cur_bs = cands[lo].bs_blk & 0xFFFF;
        s_scan = lo + 1;
      }
    }
  }
  __syncthreads();
  while (!s_done) {
    const int64_t w0 = s_scan;
    for (int k = t; k < CHAIN_WIN; k += CHAIN_THREADS)
      if (w0 + k < ncand) win[k] = cands[w0 + k];
    __syncthreads();
    if (t == 0) {
      int64_t j = w0, f = s_f, first = s_first, cur_off = s_cur_off, cur_bs = s_cur_bs;
      const int blk = (int)s_blk;
      const int64_t wend = w0 + CHAIN_WIN < ncand ? w0 + CHAIN_WIN : ncand;
      for (; j < wend; ++j) {
        const Cand c = win[j - w0];
        const uint64_t want = blk ? (uint64_t)(first + cur_bs) : (uint64_t)(f + 1);
        if ((int)(c.bs_blk >> 16) != blk || cand_num(c) != want) continue;
        Frame fr;
        fr.first = (uint64_t)first;
        fr.start = (uint32_t)cur_off;
        fr.next = c.off;
        fr.bs = (uint32_t)cur_bs;
        fr.flags = 0;
        fr.dec_end = 0;
        fr.pad = 0;
        frames[f] = fr;
        ++f;
        first += cur_bs;
        cur_off = c.off;
        cur_bs = c.bs_blk & 0xFFFF;
      }
      s_f = f, s_first = first, s_cur_off = cur_off, s_cur_bs = cur_bs, s_scan = j;
      if (j >= ncand) {  // the current frame is the last one
        Frame fr;
        fr.first = (uint64_t)first;
        fr.start = (uint32_t)cur_off;
        fr.next = (uint32_t)n;
        fr.bs = (uint32_t)cur_bs;
        fr.flags = 0;
        fr.dec_end = 0;
        fr.pad = 0;
        frames[f] = fr;
        s_f = f + 1;
        s_first = first + cur_bs;
        s_done = 1;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    st[flac::S_NFRAMES] = s_f;
    st[flac::S_TOTAL] = s_first;
  }
}

__global__ void __launch_bounds__(64) flac_decode_k(flac::Job jb, Frame* __restrict__ frames, int64_t* __restrict__ st) {
  __shared__ flac::Shared sh;
  __shared__ uint16_t table[256];
  __shared__ uint32_t xpow[65];
  const int lane = threadIdx.x;
  flac::crc16_setup(table, xpow, lane);
  __syncthreads();
  jb.crc_table = table;
  jb.xpow = xpow;
  const int64_t nframes = st[flac::S_NFRAMES];
  for (int64_t f = blockIdx.x; f < nframes; f += gridDim.x) {
    Frame fr = frames[f];
    flac::decode_frame(jb, fr, sh, lane, 64);
    if (lane == 0) {
      frames[f].flags = fr.flags;
      frames[f].dec_end = fr.dec_end;
      if (fr.flags) atomicMin(reinterpret_cast<unsigned long long*>(st + flac::S_FIRST_BAD), (unsigned long long)f);
    }
  }
}

__global__ void flac_finalize_k(const Frame* __restrict__ frames, int64_t* __restrict__ st) {
  const int64_t f = st[flac::S_FIRST_BAD];
  if (f < st[flac::S_NFRAMES]) {
    st[flac::S_BAD_FLAGS] = frames[f].flags;
    st[flac::S_BAD_START] = frames[f].start;
    st[flac::S_BAD_END] = frames[f].dec_end;
    st[flac::S_BAD_NEXT] = frames[f].next;
  }
}

int check_region(const char* who, const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cap) {
  MG_CHECK_ARG(data && ws && nbytes > 0 && nbytes < (1ll << 32) - 64 && cap >= 1 && cap < (1ll << 31),
               "%s: bad arguments (nbytes %lld, cap %lld)", who, (long long)nbytes, (long long)cap);
  MG_CHECK_ARG(((uintptr_t)data & 15) == 0, "%s: the region must be 16-byte aligned", who);
  const Layout l = layout(nbytes, cap);
  MG_CHECK_ARG(ws_bytes >= l.total, "%s: workspace of %zu bytes, %zu needed (mg_flac_ws_bytes)", who, ws_bytes, l.total);
  return MG_OK;
}

}  // namespace

extern "C" size_t mg_flac_padded_bytes(int64_t nbytes) {
  if (nbytes < 0) return 0;
  return (size_t)((nbytes + SCAN_CHUNK - 1) / SCAN_CHUNK * SCAN_CHUNK + 16);
}

extern "C" size_t mg_flac_ws_bytes(int64_t nbytes, int64_t cand_cap) {
  if (nbytes <= 0 || cand_cap < 1) return 0;
  return layout(nbytes, cand_cap).total;
}

extern "C" int mg_flac_scan(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, mg_stream_t stream) {
  const int rc = check_region("mg_flac_scan", data, nbytes, ws, ws_bytes, cand_cap);
  if (rc) return rc;
  const Layout l = layout(nbytes, cand_cap);
  uint8_t* w = static_cast<uint8_t*>(ws);
  int64_t* st = reinterpret_cast<int64_t*>(w);
  uint32_t* counts = reinterpret_cast<uint32_t*>(w + l.counts);
  uint32_t* offs = reinterpret_cast<uint32_t*>(w + l.offs);
  Cand* cands = reinterpret_cast<Cand*>(w + l.cands);
  Frame* frames = reinterpret_cast<Frame*>(w + l.frames);
  const uint8_t* d = static_cast<const uint8_t*>(data);
  hipStream_t s = (hipStream_t)stream;
  MG_CHECK_ARG(l.nchunks < (1ll << 31), "mg_flac_scan: region too large");
  flac_scan_k<false><<<(unsigned)l.nchunks, SCAN_THREADS, 0, s>>>(d, nbytes, counts, offs, cands, cand_cap);
  flac_offsets_k<<<1, 1024, 0, s>>>(counts, offs, l.nchunks, st);
  flac_scan_k<true><<<(unsigned)l.nchunks, SCAN_THREADS, 0, s>>>(d, nbytes, counts, offs, cands, cand_cap);
  flac_chain_k<<<1, CHAIN_THREADS, 0, s>>>(cands, frames, st, nbytes, cand_cap, 0, 0);
  MG_CHECK_LAUNCH("mg_flac_scan");
  return MG_OK;
}

extern "C" int mg_flac_rechain(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, int64_t frame,
                               int64_t offset, mg_stream_t stream) {
  const int rc = check_region("mg_flac_rechain", data, nbytes, ws, ws_bytes, cand_cap);
  if (rc) return rc;
  MG_CHECK_ARG(frame >= 1 && frame < cand_cap && offset > 0, "mg_flac_rechain: bad frame %lld / offset %lld", (long long)frame,
               (long long)offset);
  const Layout l = layout(nbytes, cand_cap);
  uint8_t* w = static_cast<uint8_t*>(ws);
  flac_chain_k<<<1, CHAIN_THREADS, 0, (hipStream_t)stream>>>(reinterpret_cast<Cand*>(w + l.cands), reinterpret_cast<Frame*>(w + l.frames),
                                                            reinterpret_cast<int64_t*>(w), nbytes, cand_cap, frame, offset);
  MG_CHECK_LAUNCH("mg_flac_rechain");
  return MG_OK;
}

extern "C" int mg_flac_decode(const void* data, int64_t nbytes, void* ws, size_t ws_bytes, int64_t cand_cap, int channels, int bps,
                              int sample_rate, int32_t* planar, void* out, int64_t out_frames, mg_stream_t stream) {
  const int rc = check_region("mg_flac_decode", data, nbytes, ws, ws_bytes, cand_cap);
  if (rc) return rc;
  MG_CHECK_ARG(channels >= 1 && channels <= flac::MAX_CH && bps >= 4 && bps <= 24 && sample_rate > 0 && out_frames >= 0 &&
                   (out_frames == 0 || (planar && out)),
               "mg_flac_decode: bad arguments (channels %d, bits %d, rate %d, frames %lld)", channels, bps, sample_rate,
               (long long)out_frames);
  const Layout l = layout(nbytes, cand_cap);
  uint8_t* w = static_cast<uint8_t*>(ws);
  int64_t* st = reinterpret_cast<int64_t*>(w);
  Frame* frames = reinterpret_cast<Frame*>(w + l.frames);
  flac::Job jb;
  jb.d = static_cast<const uint8_t*>(data);
  jb.n = nbytes;
  jb.nwords = (int64_t)mg_flac_padded_bytes(nbytes) / 4;
  jb.channels = channels;
  jb.bps = bps;
  jb.rate = sample_rate;
  jb.ws = planar;
  jb.out_frames = out_frames;
  jb.out = out;
  jb.crc_table = nullptr;
  jb.xpow = nullptr;
  hipStream_t s = (hipStream_t)stream;
  const int64_t grid = cand_cap < DECODE_GRID_MAX ? cand_cap : DECODE_GRID_MAX;
  flac_decode_k<<<(unsigned)grid, 64, 0, s>>>(jb, frames, st);
  flac_finalize_k<<<1, 1, 0, s>>>(frames, st);
  MG_CHECK_LAUNCH("mg_flac_decode");
  return MG_OK;
}
