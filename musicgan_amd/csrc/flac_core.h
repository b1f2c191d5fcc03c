// FLAC (RFC 9639) frame parsing and decoding, written once for the GPU kernels of flac.hip.  Every function here is plain C++
// over byte pointers and is marked host+device, so the same code runs in a kernel lane and in a host build of the decoder.
//
// Work split of one frame (mg_flac_decode gives each frame one wave, `nlanes` = 64):
//   - the frame header and the subframes are parsed by every lane in lock step (wave-uniform values, the residuals written by
//     lane 0): Rice codes are a serial dependency chain, read through a 64-bit window with clz for the unary runs;
//   - FIXED and LPC prediction is restored by one lane per channel, the history in registers;
//   - the CRC-16 is computed by all lanes over interleaved 4-byte words and combined by GF(2) multiplication;
//   - wasted bits, inter-channel decorrelation, left-justification and interleaving run over all lanes, one sample each.
#ifndef MG_FLAC_CORE_H
#define MG_FLAC_CORE_H

#include <stdint.h>

#ifndef FLAC_HD
#define FLAC_HD __host__ __device__ inline
#endif
#ifndef FLAC_SYNC
#define FLAC_SYNC() __syncthreads()
#endif

namespace flac {

// per-frame status bits (mg_flac_decode)
enum : uint32_t {
  F_CRC = 1,     // CRC-16 over the frame as decoded does not check
  F_END = 2,     // the decoded end (after the CRC-16) is not the start of the next frame of the chain
  F_HDR = 4,     // header rate / depth / channels disagree with STREAMINFO, or the header does not parse
  F_SYNTAX = 8,  // a reserved or invalid subframe field, or a read past the end of the data
  F_RANGE = 16,  // the frame's samples lie beyond the output (more samples than STREAMINFO's total)
};

constexpr int MAX_CH = 8;
constexpr int MAX_ORDER = 32;

struct Cand {  // one frame-header candidate of the scan
  uint32_t off;      // byte offset in the audio region
  uint32_t num_lo;   // coded number (frame index, or first sample for variable blocking), 36 bits
  uint32_t num_hi;
  uint32_t bs_blk;   // block size | blocking strategy << 16
};

struct Frame {  // one entry of the frame table (chain), completed by the decoder
  uint64_t first;    // first sample
  uint32_t start;    // byte offset of the header
  uint32_t next;     // byte offset of the next frame of the chain (the region's length for the last one)
  uint32_t bs;
  uint32_t flags;    // F_* of the decode
  uint32_t dec_end;  // byte offset after the CRC-16 as decoded
  uint32_t pad;
};

// status block at the start of the workspace (int64 each)
enum {
  S_NCAND = 0, S_NFRAMES, S_TOTAL, S_CHAIN_ERR, S_ERR_FRAME, S_ERR_OFF, S_BLOCKING, S_FIRST_BAD,
  S_BAD_FLAGS, S_BAD_START, S_BAD_END, S_BAD_NEXT, S_COUNT = 16
};
enum { CHAIN_OK = 0, CHAIN_NO_HEADER = 1, CHAIN_OVERFLOW = 3 };

struct Hdr {
  uint64_t num;
  int blocking, bs, rate, ch_code, channels, bps, len;  // rate / bps: 0 = from STREAMINFO; len: header bytes incl. CRC-8
};

FLAC_HD uint8_t crc8(const uint8_t* p, int n) {
  uint32_t c = 0;
  for (int i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 0x80) ? ((c << 1) ^ 0x07) & 0xFF : (c << 1) & 0xFF;
  }
  return (uint8_t)c;
}

// The frame header at byte o of d[0, n): 1 and its fields when it is a valid header whose CRC-8 checks, else 0.
FLAC_HD int parse_header(const uint8_t* d, int64_t n, int64_t o, Hdr* h) {
  if (o + 6 > n) return 0;
  const uint8_t* p = d + o;
  if (p[0] != 0xFF || (p[1] & 0xFE) != 0xF8) return 0;
  const int bcode = p[2] >> 4, rcode = p[2] & 15, ccode = p[3] >> 4, scode = (p[3] >> 1) & 7;
  if (bcode == 0 || rcode == 15 || ccode > 10 || scode == 3 || (p[3] & 1)) return 0;
  h->blocking = p[1] & 1;
  int i = 4;
  const uint32_t b0 = p[i++];
  uint64_t v;
  int extra;
  if (b0 < 0x80) {
    v = b0;
    extra = 0;
  } else if (b0 >= 0xC0 && b0 < 0xFF) {
    int lead = 0;
    while ((b0 << lead) & 0x80) ++lead;  // 2..7 leading ones
    extra = lead - 1;
    v = lead == 7 ? 0 : (b0 & (0x7Fu >> lead));
  } else {
    return 0;
  }
  if (extra == 6 && !h->blocking) return 0;  // frame numbers are at most 31 bits
  if (o + i + extra + 1 > n) return 0;
  for (int k = 0; k < extra; ++k) {
    const uint32_t b = p[i++];
    if ((b & 0xC0) != 0x80) return 0;
    v = (v << 6) | (b & 0x3F);
  }
  h->num = v;
  int bs;
  if (bcode == 1) bs = 192;
  else if (bcode <= 5) bs = 576 << (bcode - 2);
  else if (bcode == 6 || bcode == 7) {
    const int nb = bcode == 6 ? 1 : 2;
    if (o + i + nb + 1 > n) return 0;
    bs = nb == 1 ? p[i] : (p[i] << 8 | p[i + 1]);
    bs += 1;
    i += nb;
    if (bs > 65535) return 0;
  } else bs = 256 << (bcode - 8);
  int rate = 0;
  const int rates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  if (rcode < 12) rate = rates[rcode];
  else {
    const int nb = rcode == 12 ? 1 : 2;
    if (o + i + nb + 1 > n) return 0;
    const int r = nb == 1 ? p[i] : (p[i] << 8 | p[i + 1]);
    rate = rcode == 12 ? r * 1000 : (rcode == 13 ? r : r * 10);
    i += nb;
  }
  if (crc8(p, i) != p[i]) return 0;
  const int sizes[8] = {0, 8, 12, 0, 16, 20, 24, 32};
  h->bs = bs;
  h->rate = rate;
  h->ch_code = ccode;
  h->channels = ccode < 8 ? ccode + 1 : 2;
  h->bps = sizes[scode];
  h->len = i + 1;
  return 1;
}

// ---------------------------------------------------------------- CRC-16 (poly 0x8005, init 0, MSB first)
FLAC_HD uint32_t crc16_byte(uint32_t c, uint32_t b, const uint16_t* T) { return ((c << 8) & 0xFFFF) ^ T[((c >> 8) ^ b) & 0xFF]; }

FLAC_HD uint32_t crc16_table_entry(uint32_t i) {
  uint32_t t = i << 8;
  for (int k = 0; k < 8; ++k) t = (t & 0x8000) ? ((t << 1) ^ 0x8005) & 0xFFFF : (t << 1) & 0xFFFF;
  return t;
}

// a(x) b(x) mod P(x) in GF(2): the CRC register a moved past as many zero bytes as b = x^(8 k) mod P stands for
FLAC_HD uint32_t crc16_mulmod(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = (r & 0x8000) ? ((r << 1) ^ 0x8005) & 0xFFFF : (r << 1) & 0xFFFF;
    if ((b >> i) & 1) r ^= a;
  }
  return r;
}

// Lane `lane` of 64 fills its share of table[256] (crc16_byte's T) and of xpow[65], xpow[t] = x^(32 t) mod P: what Job::crc_table
// and Job::xpow point at.  The caller's barrier follows.
FLAC_HD void crc16_setup(uint16_t* table, uint32_t* xpow, int lane) {
  for (int i = lane; i < 256; i += 64) table[i] = (uint16_t)crc16_table_entry((uint32_t)i);
  const uint32_t x32 = crc16_mulmod(0x8005, 0x8005);  // x^16 = 0x8005 mod P, squared
  uint32_t p = 1;
  for (int k = 0; k < lane; ++k) p = crc16_mulmod(p, x32);
  xpow[lane] = p;
  if (lane == 63) xpow[64] = crc16_mulmod(p, x32);
}

// ---------------------------------------------------------------- bit reader over the zero-padded region
// `d` is readable (zero) up to nwords 32-bit words; words at or past nwords read as 0 and set `over`.
struct Bits {
  const uint8_t* d;
  int64_t nwords;
  uint64_t cache;  // next bits, MSB first; bits past `nbits` are 0
  int nbits;
  int64_t w;       // next word to load
  int over;
};

FLAC_HD uint32_t load_be32(const Bits& b, int64_t w) {
  const uint32_t x = reinterpret_cast<const uint32_t*>(b.d)[w];
  return (x >> 24) | ((x >> 8) & 0xFF00) | ((x << 8) & 0xFF0000) | (x << 24);
}

FLAC_HD uint32_t next_word(Bits& b) {
  if (b.w >= b.nwords) {
    b.over = 1;
    return 0;
  }
  return load_be32(b, b.w++);
}

FLAC_HD void bits_init(Bits& b, const uint8_t* d, int64_t nwords, int64_t bitpos) {
  b.d = d;
  b.nwords = nwords;
  b.over = 0;
  b.w = bitpos >> 5;
  const uint32_t hi = next_word(b), lo = next_word(b);
  b.cache = ((uint64_t)hi << 32 | lo) << (bitpos & 31);
  b.nbits = 64 - (int)(bitpos & 31);
}

FLAC_HD void refill(Bits& b) {
  if (b.nbits <= 32) {
    b.cache |= (uint64_t)next_word(b) << (32 - b.nbits);
    b.nbits += 32;
  }
}

FLAC_HD int64_t bits_pos(const Bits& b) { return b.w * 32 - b.nbits; }

FLAC_HD uint32_t get_bits(Bits& b, int k) {  // k <= 32
  if (k == 0) return 0;
  if (b.nbits < k) refill(b);
  const uint32_t v = (uint32_t)(b.cache >> (64 - k));
  b.cache = k == 64 ? 0 : b.cache << k;
  b.nbits -= k;
  return v;
}

FLAC_HD int32_t get_signed(Bits& b, int k) {  // k <= 32
  if (k == 0) return 0;
  const uint32_t v = get_bits(b, k);
  return k == 32 ? (int32_t)v : (int32_t)(v << (32 - k)) >> (32 - k);
}

// number of 0 bits before the next 1 (which is consumed)
FLAC_HD uint32_t get_unary(Bits& b) {
  uint32_t q = 0;
  while (b.cache == 0) {
    q += (uint32_t)b.nbits;
    b.nbits = 0;
    refill(b);
    if (b.over) return q;
  }
  const int z = __builtin_clzll(b.cache);
  q += (uint32_t)z;
  b.cache = (b.cache << z) << 1;
  b.nbits -= z + 1;
  return q;
}

FLAC_HD int32_t get_rice(Bits& b, int k) {
  const uint32_t q = get_unary(b);
  const uint32_t u = (q << k) | get_bits(b, k);
  return (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
}

// ---------------------------------------------------------------- one frame
struct Sub {  // what the restore and finish steps need of a subframe
  int type;   // 0 CONSTANT, 1 VERBATIM, 2 FIXED, 3 LPC
  int order, shift, wasted, prec, sbps;
  int32_t cval;
  int32_t coef[MAX_ORDER];
};

struct Shared {  // per-frame state shared by the lanes (LDS in the kernel)
  Sub sub[MAX_CH];
  uint32_t part[64];
  int ok;
};

struct Job {  // everything of one decode call
  const uint8_t* d;
  int64_t n;       // bytes of the region
  int64_t nwords;  // readable 32-bit words (zero padded past n)
  int channels, bps, rate;
  int32_t* ws;     // planar samples [channel][out_frames]
  int64_t out_frames;
  void* out;       // (out_frames, channels) int16 (bps <= 16) or int32
  const uint16_t* crc_table;
  const uint32_t* xpow;  // xpow[t] = x^(32 t) mod P, t = 0 .. nlanes
};

template <int MAXO, bool WIDE>
FLAC_HD void restore_lpc(int32_t* s, int bs, const Sub& sb) {
  int32_t c[MAXO], h[MAXO];
#pragma unroll
  for (int j = 0; j < MAXO; ++j) {
    c[j] = j < sb.order ? sb.coef[j] : 0;
    h[j] = j < sb.order ? s[sb.order - 1 - j] : 0;  // h[0]: the most recent sample
  }
  const int shift = sb.shift;
  int32_t r = sb.order < bs ? s[sb.order] : 0;
  for (int i = sb.order; i < bs; ++i) {
    const int32_t rn = i + 1 < bs ? s[i + 1] : 0;  // the next residual is requested before this sample's chain
    int32_t v;
    if (WIDE) {
      int64_t acc = 0;
#pragma unroll
      for (int j = 0; j < MAXO; ++j) acc += (int64_t)c[j] * h[j];
      v = r + (int32_t)(acc >> shift);
    } else {
      int32_t acc = 0;
#pragma unroll
      for (int j = 0; j < MAXO; ++j) acc += c[j] * h[j];
      v = r + (acc >> shift);
    }
    s[i] = v;
#pragma unroll
    for (int j = MAXO - 1; j > 0; --j) h[j] = h[j - 1];
    h[0] = v;
    r = rn;
  }
}

FLAC_HD void restore(int32_t* s, int bs, const Sub& sb) {
  if (sb.type == 2) {
    restore_lpc<4, false>(s, bs, sb);  // FIXED: shift 0, so 32-bit wrap-around arithmetic gives the exact sample
    return;
  }
  if (sb.type != 3) return;
  int lg = 0;
  while ((1 << lg) < sb.order) ++lg;
  const bool wide = sb.sbps + sb.prec + lg > 32;
  if (sb.order <= 4) wide ? restore_lpc<4, true>(s, bs, sb) : restore_lpc<4, false>(s, bs, sb);
  else if (sb.order <= 8) wide ? restore_lpc<8, true>(s, bs, sb) : restore_lpc<8, false>(s, bs, sb);
  else if (sb.order <= 12) wide ? restore_lpc<12, true>(s, bs, sb) : restore_lpc<12, false>(s, bs, sb);
  else if (sb.order <= 16) wide ? restore_lpc<16, true>(s, bs, sb) : restore_lpc<16, false>(s, bs, sb);
  else wide ? restore_lpc<32, true>(s, bs, sb) : restore_lpc<32, false>(s, bs, sb);
}

// Parses channel `ch`'s subframe (every lane in lock step); lane 0 writes warm-up samples and residuals to s[0, bs).
// Returns 0 on a syntax error.
FLAC_HD int parse_subframe(Bits& br, int bs, int sbps, int lane, int32_t* s, Sub& sb) {
  if (get_bits(br, 1) != 0) return 0;
  const int t = (int)get_bits(br, 6);
  int wasted = 0;
  if (get_bits(br, 1)) {
    wasted = 1 + (int)get_unary(br);
    if (wasted >= sbps) return 0;
  }
  sbps -= wasted;
  int type, order = 0;
  if (t == 0) type = 0;
  else if (t == 1) type = 1;
  else if (t >= 8 && t <= 12) type = 2, order = t - 8;
  else if (t >= 32) type = 3, order = t - 31;
  else return 0;
  if (order > bs) return 0;
  int prec = 0, shift = 0;
  int32_t cval = 0;
  int32_t coef[MAX_ORDER];
  if (type == 0) {
    cval = get_signed(br, sbps);
  } else if (type == 1) {
    for (int i = 0; i < bs; ++i) {
      const int32_t v = get_signed(br, sbps);
      if (lane == 0) s[i] = v;
    }
  } else {
    for (int i = 0; i < order; ++i) {
      const int32_t v = get_signed(br, sbps);
      if (lane == 0) s[i] = v;
    }
    if (type == 2) {
      const int32_t fc[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
      for (int j = 0; j < MAX_ORDER; ++j) coef[j] = j < 4 ? fc[order][j] : 0;
    } else {
      prec = (int)get_bits(br, 4) + 1;
      if (prec == 16) return 0;
      shift = get_signed(br, 5);
      if (shift < 0) return 0;
      for (int j = 0; j < order; ++j) coef[j] = get_signed(br, prec);
      for (int j = order; j < MAX_ORDER; ++j) coef[j] = 0;
    }
    const int method = (int)get_bits(br, 2);
    if (method > 1) return 0;
    const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
    const int porder = (int)get_bits(br, 4);
    const int pn = bs >> porder;
    if ((pn << porder) != bs || pn < order) return 0;
    int i = order;
    for (int p = 0; p < (1 << porder); ++p) {
      const int k = (int)get_bits(br, pbits);
      const int end = (p + 1) * pn;
      if (k == esc) {
        const int wbits = (int)get_bits(br, 5);
        for (; i < end; ++i) {
          const int32_t v = get_signed(br, wbits);
          if (lane == 0) s[i] = v;
        }
      } else {
        for (; i < end; ++i) {
          const int32_t v = get_rice(br, k);
          if (lane == 0) s[i] = v;
        }
      }
      if (br.over) return 0;
    }
  }
  if (br.over) return 0;
  if (lane == 0) {
    sb.type = type;
    sb.order = order;
    sb.shift = shift;
    sb.wasted = wasted;
    sb.prec = prec;
    sb.sbps = sbps;
    sb.cval = cval;
    if (type >= 2)
      for (int j = 0; j < MAX_ORDER; ++j) sb.coef[j] = coef[j];
  }
  return 1;
}

// CRC-16 of bytes [start, end) of the region by `nlanes` lanes: the range is cut into 4-byte words aligned to its END (leading
// bytes before `start` read as 0, which a CRC with init 0 ignores); lane l takes words l, l + nlanes, ... in Horner form and the
// lanes' parts are combined by lane 0 in `sh.part`.  Returns the CRC on lane 0.
FLAC_HD uint32_t frame_crc_part(const Job& jb, int64_t start, int64_t end, int lane, int nlanes) {
  const int64_t K = (end - start + 3) / 4;
  const int64_t base = end - 4 * K;
  uint32_t acc = 0;
  int64_t last = -1;
  for (int64_t k = lane; k < K; k += nlanes) {
    uint32_t c = 0;
    for (int j = 0; j < 4; ++j) {
      const int64_t o = base + 4 * k + j;
      c = crc16_byte(c, o >= start ? jb.d[o] : 0, jb.crc_table);
    }
    acc = crc16_mulmod(acc, jb.xpow[nlanes]) ^ c;
    last = k;
  }
  // shift past the words after this lane's last one (fewer than nlanes)
  return last < 0 ? 0 : crc16_mulmod(acc, jb.xpow[K - 1 - last]);
}

// One frame by `nlanes` lanes; FLAC_SYNC() orders the steps (a workgroup barrier in the kernel).  F.flags / F.dec_end are set
// on lane 0.  Every branch around a FLAC_SYNC() depends on wave-uniform values only.
FLAC_HD void decode_frame(const Job& jb, Frame& F, Shared& sh, int lane, int nlanes) {
  Hdr h;
  uint32_t flags = 0;
  int64_t dec_end = F.start;
  const int C = jb.channels;
  const int hdr_ok = parse_header(jb.d, jb.n, F.start, &h);
  if (!hdr_ok || h.channels != C || (h.bps && h.bps != jb.bps) || (h.rate && h.rate != jb.rate) || h.bs != (int)F.bs)
    flags |= F_HDR;
  else if (F.first + F.bs > (uint64_t)jb.out_frames)
    flags |= F_RANGE;
  if (!flags) {
    Bits br;
    bits_init(br, jb.d, jb.nwords, ((int64_t)F.start + h.len) * 8);
    for (int c = 0; c < C && !flags; ++c) {
      const int side = (h.ch_code == 8 && c == 1) || (h.ch_code == 9 && c == 0) || (h.ch_code == 10 && c == 1);
      if (!parse_subframe(br, (int)F.bs, jb.bps + side, lane, jb.ws + c * jb.out_frames + F.first, sh.sub[c])) flags |= F_SYNTAX;
    }
    dec_end = (bits_pos(br) + 7) / 8 + 2;  // zero padding to a byte, then the CRC-16
    if (dec_end > jb.n) flags |= F_SYNTAX;
  }
  FLAC_SYNC();
  if (!flags) {
    sh.part[lane] = frame_crc_part(jb, F.start, dec_end, lane, nlanes);
    FLAC_SYNC();
    if (lane == 0) {
      uint32_t crc = 0;
      for (int l = 0; l < nlanes; ++l) crc ^= sh.part[l];
      sh.ok = crc == 0;
    }
    for (int c = lane; c < C; c += nlanes) restore(jb.ws + c * jb.out_frames + F.first, (int)F.bs, sh.sub[c]);
    FLAC_SYNC();
    if (!sh.ok) flags |= F_CRC;
    const int bps = jb.bps;
    for (int i = lane; i < (int)F.bs; i += nlanes) {
      const int64_t pos = (int64_t)F.first + i;
      int32_t v[MAX_CH];
#pragma unroll
      for (int c = 0; c < MAX_CH; ++c) {
        if (c < C) {
          const Sub& sb = sh.sub[c];
          const int32_t x = sb.type == 0 ? sb.cval : jb.ws[c * jb.out_frames + pos];
          v[c] = (int32_t)((uint32_t)x << sb.wasted);
        } else {
          v[c] = 0;
        }
      }
      if (h.ch_code == 8) {
        v[1] = v[0] - v[1];  // left / side: R = L - S
      } else if (h.ch_code == 9) {
        v[0] = v[0] + v[1];  // side / right: L = S + R
      } else if (h.ch_code == 10) {
        const int32_t m = (int32_t)((uint32_t)v[0] << 1) | (v[1] & 1), sd = v[1];
        v[0] = (m + sd) >> 1;
        v[1] = (m - sd) >> 1;
      }
      if (bps <= 16) {
        int16_t* o = reinterpret_cast<int16_t*>(jb.out) + pos * C;
#pragma unroll
        for (int c = 0; c < MAX_CH; ++c)
          if (c < C) o[c] = (int16_t)((uint32_t)v[c] << (16 - bps));
      } else {
        int32_t* o = reinterpret_cast<int32_t*>(jb.out) + pos * C;
#pragma unroll
        for (int c = 0; c < MAX_CH; ++c)
          if (c < C) o[c] = (int32_t)((uint32_t)v[c] << (32 - bps));
      }
    }
  }
  if (dec_end != (int64_t)F.next) flags |= F_END;
  if (lane == 0) {
    F.flags = flags;
    F.dec_end = (uint32_t)(dec_end < 0xFFFFFFFFll ? dec_end : 0xFFFFFFFFll);
  }
  FLAC_SYNC();  // sh is reused by the next frame
}

}  // namespace flac

#endif
