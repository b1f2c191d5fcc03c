// Ogg Vorbis decoding (Vorbis I specification) on the device: what torchaudio.load does for a .ogg input (the reference's
// audio/functions.py:43).  The host walks the Ogg pages, parses the three header packets, packs the setup into the int32 / float32
// tables read here (musicgan_amd/audio/vorbis.py, pack_setup) and builds the audio-packet table.
//
// Phases, each a launch on the caller's stream, nothing read back in between (`phases` selects them, for timing):
//   1. pages (one workgroup per page): the CRC-32 of every audio page -- lane-parallel partial CRCs shifted into place with a
//      GF(2) multiply and xor-combined -- and the page bodies gathered into one contiguous payload, so packets are contiguous.
//   2. packets (one wave per audio packet; lane 0 reads the bits): mode, window flags, floor 1 Y values per channel and the
//      curve's posts, the nonzero flags propagated over coupled pairs, residues 0 / 1 / 2 per submap.  Codewords come from a
//      2^10-entry table of the next bits; longer codewords from a binary search of the left-aligned sorted codewords.
//   3. spectrum (one thread per packet and bin): inverse coupling, floor curve (render_line in closed form) x residue.
//   4. imdct (one workgroup per packet and channel): the n/2 coefficients' DCT-IV through an n/8-point complex FFT in LDS,
//      written back in place: the IMDCT's n outputs are the DCT-IV's n/2 values with signs (y = unfold(c), see unfold()).
//   5. overlap (one thread per output frame): window slopes, overlap-add of the two blocks covering the frame, interleave, trim.
//   6. finalize (one workgroup): the first bad page and the first bad packet, for the host's single status read.
// Every sum has a fixed order: the same input gives the same bits on every run.
#include "fft_radix2.h"
#include "mg_common.h"
#include "ogg_crc.h"

namespace {

constexpr int MAX_CH = 8;
constexpr int MAX_POSTS = 65;
constexpr int POST_STRIDE = 66;
constexpr int PAGE_THREADS = 256;
constexpr int SPEC_THREADS = 256;
constexpr int SPEC_GRID_Y = 65535;  // the largest grid y extent
constexpr int IMDCT_THREADS = 256;
constexpr int MAX_FFT = 2048;  // n / 4 complex points for n = 8192
constexpr int OLA_THREADS = 256;
constexpr int FIN_THREADS = 256;

// int32 setup layout (audio/vorbis.py pack_setup)
constexpr int BOOK_INTS = 8, FLOOR_INTS = 484, RES_INTS = 520, MAP_INTS = 556;
enum { H_CH = 0, H_BS0, H_BS1, H_NMODE, H_NF, H_NR, H_NM, H_NB, H_BOOK, H_FLOOR, H_RES, H_MAP, H_MODE, H_MODEBITS,
       H_DB = 16, H_TW0, H_TW1 };
enum { F_PARTS = 0, F_MULT, F_RBITS, F_VALUES, F_PCLASS = 4, F_CDIM = 36, F_CSUB = 52, F_CMASTER = 68, F_SUBBOOK = 84, F_X = 212,
       F_ORDER = 280, F_LOW = 348, F_HIGH = 416 };
enum { M_SUBMAPS = 0, M_STEPS, M_MAG = 4, M_ANG = 260, M_MUX = 516, M_SFLOOR = 524, M_SRES = 540 };

// packet table (int64 x PK) and packet info (int32 x PI)
constexpr int PK = 5;  // payload offset, bytes, spectrum offset (floats), first returned frame, host blockflag
constexpr int PI = 4;  // flags (blockflag | prev << 1 | next << 2 | mode << 4), bits consumed, error, 0
constexpr int PG = 4;  // page: file offset, body offset, body bytes, payload offset

enum { E_NOT_AUDIO = 1, E_MODE = 2, E_BLOCK = 3 };

struct Ws {
  int64_t* status;
  int32_t* page_bad;
  int32_t* pinfo;
  int32_t* floor_n;
  int32_t* posts;
  uint8_t* cls;
  float* spec;
};

__host__ __device__ inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

struct Layout {
  size_t page_bad, pinfo, floor_n, posts, cls, spec, total;
};

Layout layout(int64_t npk, int64_t npages, int64_t spec_floats, int ch, int64_t cls_stride) {
  Layout l;
  l.page_bad = 256;
  l.pinfo = l.page_bad + al((size_t)npages * 4);
  l.floor_n = l.pinfo + al((size_t)npk * PI * 4);
  l.posts = l.floor_n + al((size_t)npk * ch * 4);
  l.cls = l.posts + al((size_t)npk * ch * POST_STRIDE * 4);
  l.spec = l.cls + al((size_t)npk * cls_stride);
  l.total = l.spec + al((size_t)spec_floats * 4);
  return l;
}

// ------------------------------------------------------------------ 1. pages
__global__ void __launch_bounds__(PAGE_THREADS) vorbis_pages_k(const uint8_t* __restrict__ file, const int64_t* __restrict__ pages,
                                                               int64_t crc_from, uint8_t* __restrict__ payload,
                                                               int32_t* __restrict__ page_bad) {
  __shared__ uint32_t T[256];
  __shared__ uint32_t part[PAGE_THREADS / 64];
  const int t = threadIdx.x;
  const int64_t pg = blockIdx.x;
  const int64_t off = pages[pg * PG], body = pages[pg * PG + 1], blen = pages[pg * PG + 2], pay = pages[pg * PG + 3];
  for (int64_t i = t; i < blen; i += PAGE_THREADS) payload[pay + i] = file[body + i];
  if (pg < crc_from) {
    if (t == 0) page_bad[pg] = 0;
    return;
  }
  const uint32_t x = ogg::page_crc_block<PAGE_THREADS>(file + off, body + blen - off, t, T, part);
  if (t == 0) {
    const uint32_t stored = (uint32_t)file[off + 22] | ((uint32_t)file[off + 23] << 8) | ((uint32_t)file[off + 24] << 16) |
                            ((uint32_t)file[off + 25] << 24);
    page_bad[pg] = x != stored;
  }
}

// ------------------------------------------------------------------ 2. packets
struct Bits {
  const uint8_t* p;  // 4-byte aligned base of the payload
  int64_t start;     // packet's first bit in the payload
  int pos, nbits;
  bool eop;

  __device__ uint32_t peek32() const {
    const int64_t b = start + pos;
    const int64_t w = b >> 5;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
    const uint64_t lo = (uint64_t)q[w] | ((uint64_t)q[w + 1] << 32);
    const int sh = (int)(b & 31);
    return (uint32_t)(lo >> sh);
  }
  __device__ uint32_t read(int k) {  // k <= 32
    if (k == 0) return 0;
    if (eop || pos + k > nbits) {
      eop = true;
      pos = nbits;
      return 0;
    }
    const uint32_t v = peek32();
    pos += k;
    return k == 32 ? v : (v & ((1u << k) - 1u));
  }
};

struct Setup {
  const int32_t* s;
  const float* f;
  __device__ const int32_t* book(int b) const { return s + s[H_BOOK] + b * BOOK_INTS; }
  __device__ const int32_t* floor1(int i) const { return s + s[H_FLOOR] + i * FLOOR_INTS; }
  __device__ const int32_t* residue(int i) const { return s + s[H_RES] + i * RES_INTS; }
  __device__ const int32_t* mapping(int i) const { return s + s[H_MAP] + i * MAP_INTS; }
  __device__ const int32_t* mode(int i) const { return s + s[H_MODE] + i * 4; }
};

__device__ int decode_entry(Bits& br, const Setup& S, int b) {
  if (br.eop || br.pos >= br.nbits) {
    br.eop = true;
    return -1;
  }
  const int32_t* bk = S.book(b);
  const uint32_t peek = br.peek32();
  const int pbits = bk[2];
  int32_t e = S.s[bk[4] + (int)(peek & ((1u << pbits) - 1u))];
  int len, entry;
  if (e >= 0) {
    len = e >> 24;
    entry = e & 0xFFFFFF;
  } else {
    const uint32_t v = __brev(peek);  // the next 32 bits, first bit read as the most significant
    const int32_t* srt = S.s + bk[5];
    int lo = 0, hi = bk[3] - 1, k = -1;
    while (lo <= hi) {  // the largest left-aligned codeword <= v
      const int mid = (lo + hi) >> 1;
      if ((uint32_t)srt[2 * mid] <= v) {
        k = mid;
        lo = mid + 1;
      } else {
        hi = mid - 1;
      }
    }
    if (k < 0) {
      br.eop = true;
      return -1;
    }
    len = srt[2 * k + 1] & 0xFF;
    entry = srt[2 * k + 1] >> 8;
    const uint32_t code = (uint32_t)srt[2 * k];
    if (len < 32 && ((code ^ v) >> (32 - len)) != 0) {  // no codeword is a prefix of these bits
      br.eop = true;
      return -1;
    }
  }
  if (br.pos + len > br.nbits) {
    br.eop = true;
    br.pos = br.nbits;
    return -1;
  }
  br.pos += len;
  return entry;
}

__device__ __forceinline__ int ilog_d(int v) { return v > 0 ? 32 - __clz(v) : 0; }

struct PacketCtx {
  Setup S;
  float* spec;  // this packet's channels, n2 floats each
  uint8_t* cls;
  int n2, ch;
};

// adds one partition's VQ vectors (kind 0: interleaved by `step`; kind 1 / 2: in order) at interleaved position `off` of the
// submap's vector; `chs` channels of the submap listed in `chan` (type 2 interleaves them: position i -> channel i % chs, bin i / chs)
__device__ bool decode_partition(Bits& br, const PacketCtx& P, int book, int kind, int64_t off, int psize, const int* chan, int chs,
                                 int j_single, int64_t size) {
  const int32_t* bk = P.S.book(book);
  const int dims = bk[0];
  const int vq = bk[6];
  if (vq < 0 || dims <= 0) return false;
  if (kind == 0) {
    const int step = psize / dims;
    float* v = P.spec + (int64_t)j_single * P.n2;
    for (int j = 0; j < step; ++j) {
      const int e = decode_entry(br, P.S, book);
      if (e < 0) return true;
      for (int d = 0; d < dims; ++d) v[off + j + d * step] += P.S.f[vq + (int64_t)e * dims + d];
    }
  } else {
    int i = 0;
    while (i < psize) {
      const int e = decode_entry(br, P.S, book);
      if (e < 0) return true;
      for (int d = 0; d < dims; ++d, ++i) {  // a vector may run past the partition, as the specification's loop does
        const int64_t pos = off + i;
        if (pos >= size) continue;
        const float val = P.S.f[vq + (int64_t)e * dims + d];
        if (kind == 2) {
          P.spec[(int64_t)chan[pos % chs] * P.n2 + pos / chs] += val;
        } else {
          P.spec[(int64_t)j_single * P.n2 + pos] += val;
        }
      }
    }
  }
  return br.eop;
}

// one residue of a submap.  type 2: one vector of n2 * chs values; types 0, 1: one per channel
__device__ void decode_residue(Bits& br, const PacketCtx& P, const int32_t* R, const int* chan, int chs, uint32_t dnd) {
  const int type = R[0];
  const int vecs = type == 2 ? 1 : chs;
  const int64_t size = type == 2 ? (int64_t)P.n2 * chs : P.n2;
  if (type == 2) {
    bool all = true;
    for (int j = 0; j < chs; ++j) all = all && ((dnd >> chan[j]) & 1u);
    if (all) return;
  }
  const int64_t begin = R[1] < size ? R[1] : size, end = R[2] < size ? R[2] : size;
  const int psize = R[3], ncls = R[4], classbook = R[5], cpc = R[6];
  const int64_t nread = end - begin;
  const int64_t parts = nread > 0 ? nread / psize : 0;
  if (parts == 0) return;
  const int64_t stride = parts + cpc;
  for (int pass = 0; pass < 8; ++pass) {
    int64_t pc = 0;
    while (pc < parts) {
      if (pass == 0) {
        for (int j = 0; j < vecs; ++j) {
          if (type != 2 && ((dnd >> chan[j]) & 1u)) continue;
          int temp = decode_entry(br, P.S, classbook);
          if (temp < 0) return;
          for (int i = cpc - 1; i >= 0; --i) {
            P.cls[j * stride + i + pc] = (uint8_t)(temp % ncls);
            temp /= ncls;
          }
        }
      }
      for (int i = 0; i < cpc && pc < parts; ++i, ++pc) {
        for (int j = 0; j < vecs; ++j) {
          if (type != 2 && ((dnd >> chan[j]) & 1u)) continue;
          const int book = R[8 + 8 * P.cls[j * stride + pc] + pass];
          if (book < 0) continue;
          if (decode_partition(br, P, book, type, begin + pc * psize, psize, chan, chs, type == 2 ? 0 : chan[j], size)) return;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(64) vorbis_packets_k(const uint8_t* __restrict__ payload, const int64_t* __restrict__ pk,
                                                        int64_t npk, const int32_t* __restrict__ setup, const float* __restrict__ fs,
                                                        Ws ws, int64_t cls_stride) {
  __shared__ int Y[MAX_POSTS];
  __shared__ int fin[MAX_POSTS];
  __shared__ int step2[MAX_POSTS];
  __shared__ int chan[MAX_CH];
  const int64_t p = blockIdx.x;
  const int lane = threadIdx.x;
  Setup S{setup, fs};
  const int ch = setup[H_CH];
  const int bf_host = (int)pk[p * PK + 4];
  const int n = bf_host ? setup[H_BS1] : setup[H_BS0];
  const int n2 = n / 2;
  float* spec = ws.spec + pk[p * PK + 2];
  for (int64_t i = lane; i < (int64_t)ch * n2; i += 64) spec[i] = 0.f;
  __syncthreads();
  if (lane != 0) return;
  int32_t* info = ws.pinfo + p * PI;
  int32_t* fn = ws.floor_n + p * ch;
  for (int c = 0; c < ch; ++c) fn[c] = 0;
  Bits br{payload, pk[p * PK] * 8, 0, (int)(pk[p * PK + 1] * 8), false};
  info[2] = 0;
  if (br.read(1) != 0) {
    info[2] = E_NOT_AUDIO;
    return;
  }
  const int mode = (int)br.read(setup[H_MODEBITS]);
  if (mode >= setup[H_NMODE]) {
    info[2] = E_MODE;
    return;
  }
  const int bf = S.mode(mode)[0];
  const int32_t* M = S.mapping(S.mode(mode)[1]);
  int prev = 0, next = 0;
  if (bf) {
    prev = (int)br.read(1);
    next = (int)br.read(1);
  }
  if (bf != bf_host) {
    info[2] = E_BLOCK;
    return;
  }
  info[0] = bf | (prev << 1) | (next << 2) | (mode << 4);
  // floors: the posts of each used channel's curve, sorted by X, written as (X << 16 | clamped Y * multiplier)
  uint32_t used = 0;  // bit c: channel c's floor is used
  for (int c = 0; c < ch; ++c) {
    if (br.eop) continue;
    const int32_t* F = S.floor1(M[M_SFLOOR + M[M_MUX + c]]);
    if (br.read(1) == 0) continue;
    const int mult = F[F_MULT];
    const int range = mult == 1 ? 256 : mult == 2 ? 128 : mult == 3 ? 86 : 64;
    const int bits = ilog_d(range - 1);
    Y[0] = (int)br.read(bits);
    Y[1] = (int)br.read(bits);
    int off = 2;
    for (int i = 0; i < F[F_PARTS]; ++i) {
      const int cl = F[F_PCLASS + i];
      const int cdim = F[F_CDIM + cl], cbits = F[F_CSUB + cl];
      const int csub = (1 << cbits) - 1;
      int cval = 0;
      if (cbits > 0) cval = decode_entry(br, S, F[F_CMASTER + cl]);
      for (int j = 0; j < cdim; ++j) {
        const int book = F[F_SUBBOOK + 8 * cl + (cval & csub)];
        cval >>= cbits;
        Y[off + j] = book >= 0 ? decode_entry(br, S, book) : 0;
      }
      off += cdim;
    }
    if (br.eop) continue;  // the packet ended inside this floor: the channel is unused
    used |= 1u << c;
    // amplitude synthesis (step 1)
    const int nx = F[F_VALUES];
    fin[0] = Y[0];
    fin[1] = Y[1];
    step2[0] = step2[1] = 1;
    for (int i = 2; i < nx; ++i) {
      const int lo = F[F_LOW + i], hi = F[F_HIGH + i];
      const int x0 = F[F_X + lo], y0 = fin[lo], x1 = F[F_X + hi], y1 = fin[hi];
      const int dy = y1 - y0, adx = x1 - x0;
      const int err = abs(dy) * (F[F_X + i] - x0);
      const int o = err / adx;
      const int predicted = dy < 0 ? y0 - o : y0 + o;
      const int val = Y[i];
      const int highroom = range - predicted, lowroom = predicted;
      const int room = 2 * (highroom < lowroom ? highroom : lowroom);
      step2[i] = 0;
      if (val) {
        step2[lo] = step2[hi] = step2[i] = 1;
        if (val >= room)
          fin[i] = highroom > lowroom ? val - lowroom + predicted : predicted - val + highroom - 1;
        else
          fin[i] = (val & 1) ? predicted - ((val + 1) >> 1) : predicted + (val >> 1);
      } else {
        fin[i] = predicted;
      }
    }
    int32_t* post = ws.posts + (p * ch + c) * POST_STRIDE;
    int np = 0;
    for (int k = 0; k < nx; ++k) {
      const int j = F[F_ORDER + k];
      if (k > 0 && !step2[j]) continue;
      int y = fin[j] * mult;
      y = y < 0 ? 0 : (y > 255 ? 255 : y);
      post[np++] = (int32_t)(((uint32_t)F[F_X + j] << 16) | (uint32_t)y);
    }
    fn[c] = np;
  }
  // nonzero flags over coupled pairs
  uint32_t nz = used;
  for (int s = 0; s < M[M_STEPS]; ++s) {
    const uint32_t pair = (1u << M[M_MAG + s]) | (1u << M[M_ANG + s]);
    if (nz & pair) nz |= pair;
  }
  const uint32_t dnd = ~nz;
  PacketCtx P{S, spec, ws.cls + p * cls_stride, n2, ch};
  for (int sm = 0; sm < M[M_SUBMAPS]; ++sm) {
    if (br.eop) break;
    int chs = 0;
    for (int c = 0; c < ch; ++c)
      if (M[M_MUX + c] == sm) chan[chs++] = c;
    decode_residue(br, P, S.residue(M[M_SRES + sm]), chan, chs, dnd);
  }
  info[1] = br.pos;
}

// ------------------------------------------------------------------ 3. spectrum: inverse coupling, floor curve x residue
__device__ int floor_at(const int32_t* __restrict__ post, int np, int x) {
  int lo = 0, hi = np - 1;
  while (lo < hi) {  // the last post with X <= x (post 0 has X = 0)
    const int mid = (lo + hi + 1) >> 1;
    if ((int)((uint32_t)post[mid] >> 16) <= x) lo = mid;
    else hi = mid - 1;
  }
  const int x0 = (int)((uint32_t)post[lo] >> 16), y0 = post[lo] & 0xFFFF;
  if (lo == np - 1) return y0;
  const int x1 = (int)((uint32_t)post[lo + 1] >> 16), y1 = post[lo + 1] & 0xFFFF;
  // render_line's integer steps in closed form: after k steps the error term has wrapped floor(k * ady / adx) times
  const int dy = y1 - y0, adx = x1 - x0;
  const int base = dy / adx;
  const int ady = abs(dy) - abs(base) * adx;
  const int k = x - x0;
  const int wraps = (k * ady) / adx;
  return y0 + base * k + (dy < 0 ? -wraps : wraps);
}

__device__ void spectrum_bin(const int64_t* __restrict__ pk, const int32_t* __restrict__ setup, const float* __restrict__ fs,
                             const Ws& ws, int64_t p, int x) {
  const int info0 = ws.pinfo[p * PI];
  if (ws.pinfo[p * PI + 2]) return;
  const int bf = info0 & 1, mode = info0 >> 4;
  const int n2 = (bf ? setup[H_BS1] : setup[H_BS0]) / 2;
  if (x >= n2) return;
  const int ch = setup[H_CH];
  Setup S{setup, fs};
  const int32_t* M = S.mapping(S.mode(mode)[1]);
  float* spec = ws.spec + pk[p * PK + 2];
  for (int s = M[M_STEPS] - 1; s >= 0; --s) {
    float* pm = spec + (int64_t)M[M_MAG + s] * n2 + x;
    float* pa = spec + (int64_t)M[M_ANG + s] * n2 + x;
    const float m = *pm, a = *pa;
    float nm, na;
    if (m > 0.f) {
      if (a > 0.f) nm = m, na = m - a;
      else na = m, nm = m + a;
    } else {
      if (a > 0.f) nm = m, na = m + a;
      else na = m, nm = m - a;
    }
    *pm = nm;
    *pa = na;
  }
  const float* db = fs + setup[H_DB];
  for (int c = 0; c < ch; ++c) {
    const int np = ws.floor_n[p * ch + c];
    float* v = spec + (int64_t)c * n2 + x;
    *v = np ? *v * db[floor_at(ws.posts + (p * ch + c) * POST_STRIDE, np, x)] : 0.f;
  }
}

// grid: (bins / SPEC_THREADS, min(packets, SPEC_GRID_Y)); packets beyond the grid's y extent are taken in strides of it
__global__ void __launch_bounds__(SPEC_THREADS) vorbis_spectrum_k(const int64_t* __restrict__ pk, int64_t npk,
                                                                  const int32_t* __restrict__ setup, const float* __restrict__ fs,
                                                                  Ws ws) {
  const int x = blockIdx.x * SPEC_THREADS + threadIdx.x;
  for (int64_t p = blockIdx.y; p < npk; p += gridDim.y) spectrum_bin(pk, setup, fs, ws, p, x);
}

// ------------------------------------------------------------------ 4. IMDCT (DCT-IV in place)
__global__ void __launch_bounds__(IMDCT_THREADS) vorbis_imdct_k(const int64_t* __restrict__ pk, const int32_t* __restrict__ setup,
                                                                const float* __restrict__ fs, Ws ws, int64_t npk) {
  __shared__ float2 buf[MAX_FFT];
  const int ch = setup[H_CH];
  const int64_t p = blockIdx.x / ch;
  const int c = blockIdx.x % ch;
  if (ws.pinfo[p * PI + 2]) return;
  const int bf = ws.pinfo[p * PI] & 1;
  const int n = bf ? setup[H_BS1] : setup[H_BS0];
  const int M = n / 2, H = n / 4;
  const float* tw = fs + (bf ? setup[H_TW1] : setup[H_TW0]);
  const float2* pre = reinterpret_cast<const float2*>(tw);
  const float2* post = pre + H;
  const float2* w = post + H;
  float* X = ws.spec + pk[p * PK + 2] + (int64_t)c * M;
  dct4_lds(X, X, buf, M, pre, post, w, 1.0f, threadIdx.x, IMDCT_THREADS);
}

// ------------------------------------------------------------------ 5. window, overlap-add, interleave, trim
// sample i of a block's IMDCT output from its DCT-IV values c (M = n / 2 of them)
__device__ __forceinline__ float unfold(const float* c, int M, int i) {
  const int m = i + M / 2;
  if (m < M) return c[m];
  if (m < 2 * M) return -c[2 * M - 1 - m];
  return -c[m - 2 * M];
}

__device__ float window_at(const int32_t* setup, const float* fs, int flags, int i) {
  const int bf = flags & 1, prev = (flags >> 1) & 1, next = (flags >> 2) & 1;
  const int n0 = setup[H_BS0], n1 = setup[H_BS1];
  const int n = bf ? n1 : n0;
  const float* slope0 = fs + setup[H_TW0] + n0 + 2 * (n0 / 8 > 1 ? n0 / 8 : 1);  // after pre, post, fft twiddles
  const float* slope1 = fs + setup[H_TW1] + n1 + 2 * (n1 / 8 > 1 ? n1 / 8 : 1);
  int ls, le;
  const float* lsl;
  if (bf && !prev) ls = n / 4 - n0 / 4, le = n / 4 + n0 / 4, lsl = slope0;
  else ls = 0, le = n / 2, lsl = bf ? slope1 : slope0;
  int rs, re;
  const float* rsl;
  if (bf && !next) rs = 3 * n / 4 - n0 / 4, re = 3 * n / 4 + n0 / 4, rsl = slope0;
  else rs = n / 2, re = n, rsl = bf ? slope1 : slope0;
  if (i < ls || i >= re) return 0.f;
  if (i < le) return lsl[i - ls];
  if (i < rs) return 1.f;
  return rsl[re - 1 - i];  // the falling slope is the rising one reversed
}

__global__ void __launch_bounds__(OLA_THREADS) vorbis_overlap_k(const int64_t* __restrict__ pk, int64_t npk,
                                                                const int32_t* __restrict__ setup, const float* __restrict__ fs, Ws ws,
                                                                float* __restrict__ out, int64_t frames, int64_t trim_start) {
  const int64_t f = (int64_t)blockIdx.x * OLA_THREADS + threadIdx.x;
  if (f >= frames) return;
  const int64_t t = f + trim_start;
  int64_t lo = 1, hi = npk - 1;
  while (lo < hi) {  // the last packet whose returned range starts at or before t
    const int64_t mid = (lo + hi + 1) >> 1;
    if (pk[mid * PK + 3] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int64_t i = lo;
  const int ch = setup[H_CH];
  const int fa = ws.pinfo[(i - 1) * PI], fb = ws.pinfo[i * PI];
  const bool oka = ws.pinfo[(i - 1) * PI + 2] == 0, okb = ws.pinfo[i * PI + 2] == 0;
  const int pn = (fa & 1) ? setup[H_BS1] : setup[H_BS0], cn = (fb & 1) ? setup[H_BS1] : setup[H_BS0];
  const int q = (int)(t - pk[i * PK + 3]);
  const int ip = pn / 2 + q, ic = q + cn / 4 - pn / 4;
  const float wa = (oka && ip < pn) ? window_at(setup, fs, fa, ip) : 0.f;
  const float wb = (okb && ic >= 0 && ic < cn) ? window_at(setup, fs, fb, ic) : 0.f;
  const float* ca = ws.spec + pk[(i - 1) * PK + 2];
  const float* cb = ws.spec + pk[i * PK + 2];
  for (int c = 0; c < ch; ++c) {
    float v = 0.f;
    if (wa != 0.f) v += wa * unfold(ca + (int64_t)c * (pn / 2), pn / 2, ip);
    if (wb != 0.f) v += wb * unfold(cb + (int64_t)c * (cn / 2), cn / 2, ic);
    out[f * ch + c] = v;
  }
}

// ------------------------------------------------------------------ 6. status
__global__ void __launch_bounds__(FIN_THREADS) vorbis_finalize_k(Ws ws, int64_t npages, int64_t npk) {
  __shared__ int64_t s0[FIN_THREADS], s1[FIN_THREADS];
  const int t = threadIdx.x;
  int64_t bp = INT64_MAX, bk = INT64_MAX;
  for (int64_t i = t; i < npages; i += FIN_THREADS)
    if (ws.page_bad[i] && i < bp) bp = i;
  for (int64_t i = t; i < npk; i += FIN_THREADS)
    if (ws.pinfo[i * PI + 2] && i < bk) bk = i;
  s0[t] = bp;
  s1[t] = bk;
  __syncthreads();
  for (int s = FIN_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      s0[t] = s0[t] < s0[t + s] ? s0[t] : s0[t + s];
      s1[t] = s1[t] < s1[t + s] ? s1[t] : s1[t + s];
    }
    __syncthreads();
  }
  if (t == 0) {
    ws.status[0] = s0[0] == INT64_MAX ? -1 : s0[0];
    ws.status[1] = s1[0] == INT64_MAX ? -1 : s1[0];
    ws.status[2] = s1[0] == INT64_MAX ? 0 : ws.pinfo[s1[0] * PI + 2];
  }
}

}  // namespace

extern "C" size_t mg_vorbis_payload_bytes(int64_t nbytes) {
  if (nbytes < 0) return 0;
  return (size_t)((nbytes + 3) / 4 * 4 + 16);
}

extern "C" size_t mg_vorbis_ws_bytes(int64_t packets, int64_t pages, int64_t spec_floats, int channels, int64_t cls_stride) {
  if (packets < 0 || pages < 0 || spec_floats < 0 || channels < 1 || channels > MAX_CH || cls_stride < 0) return 0;
  return layout(packets, pages, spec_floats, channels, cls_stride).total;
}

extern "C" int mg_vorbis_decode(const void* file, int64_t file_bytes, const int64_t* pages, int64_t npages, int64_t crc_from,
                                const int32_t* setup, const float* fsetup, int channels, int blocksize0, int blocksize1,
                                const int64_t* packets, int64_t npk, void* payload, int64_t payload_bytes, void* ws, size_t ws_bytes,
                                int64_t spec_floats, int64_t cls_stride, float* out, int64_t out_frames, int64_t trim_start,
                                int phases, mg_stream_t stream) {
  MG_CHECK_ARG(file && pages && setup && fsetup && packets && payload && ws && npages >= 1 && npk >= 0 && file_bytes > 0,
               "mg_vorbis_decode: null or empty argument");
  MG_CHECK_ARG(channels >= 1 && channels <= MAX_CH, "mg_vorbis_decode: %d channels (1-%d)", channels, MAX_CH);
  MG_CHECK_ARG(blocksize0 >= 64 && blocksize1 <= 8192 && blocksize0 <= blocksize1 && (blocksize0 & (blocksize0 - 1)) == 0 &&
                   (blocksize1 & (blocksize1 - 1)) == 0,
               "mg_vorbis_decode: blocksizes %d / %d", blocksize0, blocksize1);
  MG_CHECK_ARG(ws_bytes >= mg_vorbis_ws_bytes(npk, npages, spec_floats, channels, cls_stride),
               "mg_vorbis_decode: workspace of %zu bytes too small", ws_bytes);
  MG_CHECK_ARG(payload_bytes >= 16 && (reinterpret_cast<uintptr_t>(payload) & 3) == 0,
               "mg_vorbis_decode: the payload buffer must be 4-byte aligned (mg_vorbis_payload_bytes)");
  MG_CHECK_ARG(out_frames == 0 || (out && npk >= 2), "mg_vorbis_decode: no output buffer");
  MG_CHECK_ARG(npages < (1ll << 31) && npk * channels < (1ll << 31), "mg_vorbis_decode: stream too long");
  const Layout l = layout(npk, npages, spec_floats, channels, cls_stride);
  uint8_t* w = static_cast<uint8_t*>(ws);
  Ws W{reinterpret_cast<int64_t*>(w), reinterpret_cast<int32_t*>(w + l.page_bad), reinterpret_cast<int32_t*>(w + l.pinfo),
       reinterpret_cast<int32_t*>(w + l.floor_n), reinterpret_cast<int32_t*>(w + l.posts), w + l.cls,
       reinterpret_cast<float*>(w + l.spec)};
  hipStream_t s = (hipStream_t)stream;
  uint8_t* pay = static_cast<uint8_t*>(payload);
  if (phases & 1) vorbis_pages_k<<<(unsigned)npages, PAGE_THREADS, 0, s>>>(static_cast<const uint8_t*>(file), pages, crc_from, pay,
                                                                         W.page_bad);
  if (npk > 0) {
    if (phases & 2) vorbis_packets_k<<<(unsigned)npk, 64, 0, s>>>(pay, packets, npk, setup, fsetup, W, cls_stride);
    if (phases & 4) {
      dim3 g((unsigned)mg_cdiv(blocksize1 / 2, SPEC_THREADS), (unsigned)(npk < SPEC_GRID_Y ? npk : SPEC_GRID_Y));
      vorbis_spectrum_k<<<g, SPEC_THREADS, 0, s>>>(packets, npk, setup, fsetup, W);
    }
    if (phases & 8) vorbis_imdct_k<<<(unsigned)(npk * channels), IMDCT_THREADS, 0, s>>>(packets, setup, fsetup, W, npk);
    if ((phases & 16) && out_frames > 0)
      vorbis_overlap_k<<<(unsigned)((out_frames + OLA_THREADS - 1) / OLA_THREADS), OLA_THREADS, 0, s>>>(
          packets, npk, setup, fsetup, W, out, out_frames, trim_start);
  }
  if (phases & 32) vorbis_finalize_k<<<1, FIN_THREADS, 0, s>>>(W, npages, npk);
  MG_CHECK_LAUNCH("mg_vorbis_decode");
  return MG_OK;
}
