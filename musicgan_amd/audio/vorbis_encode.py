"""Ogg Vorbis encoding, host side: the fixed encoder setup (codebooks, floor 1, residue 2, mapping, modes), the three header
packets laid out as Ogg pages, and the int32 / float32 tables the device encoder reads (ops.vorbis_encode, csrc/vorbis_encode.hip).

The setup depends on the channel count alone (the identification header also on the sample rate), so every file of one channel
count carries the same setup packet, whatever its quality: the decoder's setup cache (audio/vorbis.py) parses it once.

- Blocksizes 256 / 2048; only long blocks are written.  Two modes (0 short, 1 long) over one mapping.
- Floor 1: multiplier 2 (Y in 0..127), rangebits 10, NPOSTS posts: X = 0 and 1024 and 39 more spaced geometrically, listed in
  bisection order so that each post is predicted from the nearest posts around it.  13 partitions of one class of 3 dimensions,
  no subclasses: every post's `val` is coded with one 128-entry book, so every val the fit can produce has a codeword.
- Residue 2 over all channels interleaved, partitions of PSIZE = 16 values, 6 classifications picked by the largest |value| in a
  partition (0: all zero; 1: <= 1; 2: <= 2; 3: <= 4; 4: <= 8; 5: <= QMAX_CODED = 263), 2 classifications per class codeword.
  Class 5 is a two-pass cascade: pass 0 codes 17 k (|k| <= 15), pass 1 the rest in -8..8.
- Stereo: one square-polar coupling step (magnitude 0, angle 1).  3-8 channels are left uncoupled.  A coupled angle can reach
  twice a channel's value, so each channel's quantised values are kept within QMAX = 131 (posts are raised until they are).
- Codeword lengths: Huffman codes of per-class Laplacian models (computed here, `_huffman`), at most MAXLEN bits, complete
  (Kraft sum exactly 1).  Codewords are assigned in entry order as the specification's section 3.2.1 defines
  (vorbis.make_codewords).

Quality q in [-1, 10] enters only through the floor offset S(q) = 15 + 2.5 q dB: each post is set S(q) dB below the largest
coefficient magnitude around it, or below the block's largest less MASK_DB = 20 dB where that is higher (content far below the
block's loudest is coded coarsely: a crude stand-in for simultaneous masking), and coefficients are quantised to rint(X / F)
against the floor curve F the decoder renders."""
from __future__ import annotations

import heapq
import math
import struct

import numpy as np

from . import vorbis as V

BLOCKSIZES = (256, 2048)
N2 = BLOCKSIZES[1] // 2          # coefficients per long block, and the hop
MULT = 2
RANGE = 128                      # floor Y range at multiplier 2
RANGEBITS = 10
PART_DIMS = 3
NPARTS = 13
NPOSTS = 2 + PART_DIMS * NPARTS  # 41
PSIZE = 16
NCLASS = 6
CPC = 2                          # classifications per class codeword
QMAX = 131                       # bound on |q| of each channel
QMAX_CODED = 263                 # the largest |value| the residue books code (coupled angles reach 2 QMAX)
CASCADE = 17
MAXLEN = 20
SERIAL = 0x4D47414E              # every stream's Ogg serial number (fixed: same input, same bytes)
VENDOR = b"musicgan_amd Vorbis encoder"
QUALITY_DEFAULT = 3.0
MASK_DB = 20.0                   # csrc/vorbis_encode.hip MASK_GAIN = 10^(-MASK_DB / 20)

# books: 0 floor val, 1 class codeword, 2-5 the VQ books of classes 1-4, 6 class 5's coarse pass, 7 its fine pass
# (dims, values per dimension, Laplacian scale of a value) for the residue books; values are -h .. h, h = (nval - 1) / 2
RES_BOOKS = ((4, 3, 0.6), (2, 5, 1.0), (2, 9, 1.8), (2, 17, 3.5))
COARSE_N, FINE_N = 2 * 15 + 1, CASCADE
CLASS_PRIOR = (0.34, 0.24, 0.16, 0.12, 0.09, 0.05)
FLOOR_SCALE = 7.0

# int32 table layout (mirrored by csrc/vorbis_encode.hip)
TI_BOOK = 0        # [8] first entry of each book in the code / length arrays
TI_NPOSTS = 8
TI_NCODES = 9
TI_X, TI_LO, TI_HI, TI_ORD = 16, 16 + 65, 16 + 2 * 65, 16 + 3 * 65
TI_BIN = 16 + 4 * 65          # [1024] the sorted interval (rank) each bin lies in
TI_CODES = TI_BIN + N2       # codes (bit-reversed: the first bit read is bit 0), then lengths
# float32 table layout
TF_SLOPE, TF_PRE, TF_POST, TF_FFT, TF_DB = 0, N2, 2 * N2, 3 * N2, 3 * N2 + N2 // 2
TF_SIZE = TF_DB + 256


def s_db(quality: float) -> float:
    """the floor offset S(q) in dB below the local spectral peak (monotone in q)"""
    return 15.0 + 2.5 * float(quality)


# ------------------------------------------------------------------ codeword lengths
def _huffman(p) -> list:
    """Huffman code lengths of probabilities p (ties broken by entry order: deterministic), flattened until no length exceeds
    MAXLEN; complete: sum 2^-len == 1"""
    p = np.asarray(p, dtype=np.float64)
    p = p / p.sum()
    while True:
        heap = [(float(v), i, (i,)) for i, v in enumerate(p)]
        heapq.heapify(heap)
        lens = [0] * len(p)
        nxt = len(p)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for e in a[2] + b[2]:
                lens[e] += 1
            heapq.heappush(heap, (a[0] + b[0], nxt, a[2] + b[2]))
            nxt += 1
        if max(lens) <= MAXLEN:
            return lens
        p = p ** 0.8
        p = p / p.sum()


def _laplace(vals, scale):
    return np.exp(-np.abs(np.asarray(vals, dtype=np.float64)) / scale)


def _vq_entries(dims, nval):
    """(entries, dims) values of a lookup-1 book whose multiplicands are 0 .. nval - 1 with minimum -(nval - 1) / 2"""
    h = (nval - 1) // 2
    e = np.arange(nval ** dims)
    return np.stack([(e // nval ** d) % nval - h for d in range(dims)], axis=1)


# ------------------------------------------------------------------ bit writer
class _Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, k):
        assert 0 <= v < (1 << k) or k == 0, (v, k)
        self.v |= int(v) << self.n
        self.n += k

    def tobytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def _f32pack(v: float) -> int:
    """the Vorbis 32-bit float of an integer value (|v| < 2^21)"""
    if v == 0:
        return 0
    m, e = abs(int(v)), 788
    assert m < (1 << 21)
    return (0x80000000 if v < 0 else 0) | (e << 21) | m


def _post_xs():
    """the interior posts, in bisection order of their sorted positions"""
    xs = np.round(np.geomspace(3, 1000, NPOSTS - 2)).astype(np.int64)
    for i in range(1, len(xs)):
        xs[i] = max(xs[i], xs[i - 1] + 1)
    out, todo = [], [(0, len(xs))]
    while todo:
        nxt = []
        for a, b in todo:
            if a >= b:
                continue
            m = (a + b) // 2
            out.append(int(xs[m]))
            nxt += [(a, m), (m + 1, b)]
        todo = nxt
    return out


class _Setup:
    """the setup's books and tables for one channel count"""

    def __init__(self, ch: int):
        self.ch = ch
        books = []  # (dims, lengths, lookup (None or (nval, minv, delta)))
        books.append((1, _huffman(_laplace(np.arange(RANGE), FLOOR_SCALE) + 1e-4), None))
        cls = np.array(CLASS_PRIOR)
        books.append((CPC, _huffman(np.outer(cls, cls).reshape(-1)), None))
        for dims, nval, scale in RES_BOOKS:
            vals = _vq_entries(dims, nval)
            books.append((dims, _huffman(_laplace(vals, scale).prod(axis=1)), (nval, -((nval - 1) // 2), 1)))
        books.append((1, _huffman(_laplace(np.arange(COARSE_N) - 15, 2.0)), (COARSE_N, -15 * CASCADE, CASCADE)))
        books.append((1, _huffman(_laplace(np.arange(FINE_N) - 8, 6.0)), (FINE_N, -8, 1)))
        self.books = books
        self.codes = [V.make_codewords(b[1]) for b in books]
        self.X = [0, 1 << RANGEBITS] + _post_xs()
        assert len(self.X) == NPOSTS and len(set(self.X)) == NPOSTS
        self.order = sorted(range(NPOSTS), key=lambda k: self.X[k])
        self.low, self.high = [0, 0], [0, 0]
        for j in range(2, NPOSTS):
            self.low.append(max((k for k in range(j) if self.X[k] < self.X[j]), key=lambda k: self.X[k]))
            self.high.append(min((k for k in range(j) if self.X[k] > self.X[j]), key=lambda k: self.X[k]))
        self.setup_packet = self._setup_packet()
        self.ints, self.floats = self._tables()
        self.max_packet_bytes = self._max_packet_bytes()

    def _setup_packet(self) -> bytes:
        w = _Bits()
        w.put(len(self.books) - 1, 8)
        for dims, lens, lookup in self.books:
            w.put(0x564342, 24)
            w.put(dims, 16)
            w.put(len(lens), 24)
            w.put(0, 1)  # not ordered
            w.put(0, 1)  # not sparse
            for ln in lens:
                w.put(ln - 1, 5)
            if lookup is None:
                w.put(0, 4)
                continue
            nval, minv, delta = lookup
            w.put(1, 4)
            w.put(_f32pack(minv), 32)
            w.put(_f32pack(delta), 32)
            vbits = max(1, (nval - 1).bit_length())
            w.put(vbits - 1, 4)
            w.put(0, 1)  # sequence_p
            for m in range(nval):
                w.put(m, vbits)
        w.put(0, 6)   # one time-domain transform, type 0
        w.put(0, 16)
        w.put(0, 6)   # one floor, type 1
        w.put(1, 16)
        w.put(NPARTS, 5)
        for _ in range(NPARTS):
            w.put(0, 4)
        w.put(PART_DIMS - 1, 3)
        w.put(0, 2)   # no subclasses: the one book codes every post
        w.put(0 + 1, 8)
        w.put(MULT - 1, 2)
        w.put(RANGEBITS, 4)
        for x in self.X[2:]:
            w.put(x, RANGEBITS)
        w.put(0, 6)   # one residue, type 2
        w.put(2, 16)
        w.put(0, 24)
        w.put(N2 * self.ch, 24)
        w.put(PSIZE - 1, 24)
        w.put(NCLASS - 1, 6)
        w.put(1, 8)
        cascades = [0, 1, 1, 1, 1, 3]
        for c in cascades:
            w.put(c & 7, 3)
            w.put(0, 1)
        for c in range(NCLASS):
            if c in (1, 2, 3, 4):
                w.put(c + 1, 8)
            elif c == 5:
                w.put(6, 8)
                w.put(7, 8)
        w.put(0, 6)   # one mapping, type 0
        w.put(0, 16)
        w.put(0, 1)   # one submap
        if self.ch == 2:
            w.put(1, 1)
            w.put(0, 8)
            w.put(0, 1)
            w.put(1, 1)
        else:
            w.put(0, 1)
        w.put(0, 2)
        w.put(0, 8)
        w.put(0, 8)
        w.put(0, 8)
        w.put(1, 6)   # two modes: 0 short, 1 long, both on mapping 0
        for bf in (0, 1):
            w.put(bf, 1)
            w.put(0, 16)
            w.put(0, 16)
            w.put(0, 8)
        w.put(1, 1)   # framing
        return b"\x05vorbis" + w.tobytes()

    def _tables(self):
        codes, lens, starts = [], [], []
        for (_, ln, _), cw in zip(self.books, self.codes):
            starts.append(len(codes))
            for L, c in zip(ln, cw):
                codes.append(int(format(c, f"0{L}b")[::-1], 2))
                lens.append(L)
        ints = np.zeros(TI_CODES + 2 * len(codes), dtype=np.int64)
        ints[TI_BOOK:TI_BOOK + 8] = starts
        ints[TI_NPOSTS] = NPOSTS
        ints[TI_NCODES] = len(codes)
        ints[TI_X:TI_X + NPOSTS] = self.X
        ints[TI_LO:TI_LO + NPOSTS] = self.low
        ints[TI_HI:TI_HI + NPOSTS] = self.high
        ints[TI_ORD:TI_ORD + NPOSTS] = self.order
        xs = np.sort(self.X)
        ints[TI_BIN:TI_BIN + N2] = np.searchsorted(xs, np.arange(N2), side="right") - 1
        ints[TI_CODES:TI_CODES + len(codes)] = codes
        ints[TI_CODES + len(codes):] = lens
        floats = np.concatenate([V.window_slope(N2), V.dct4_tables(N2), V.inverse_db_table()])
        assert len(floats) == TF_SIZE
        return ints.astype(np.int32), floats.astype(np.float32)

    def _max_packet_bytes(self) -> int:
        mx = [max(b[1]) for b in self.books]
        parts = N2 * self.ch // PSIZE
        floor = 1 + 14 + (NPOSTS - 2) * mx[0]
        per_part = max(PSIZE // RES_BOOKS[k][0] * mx[2 + k] for k in range(4))
        per_part = max(per_part, PSIZE * (mx[6] + mx[7]))
        bits = 4 + self.ch * floor + (parts // CPC) * mx[1] + parts * per_part
        return (bits + 7) // 8


_SETUPS = {}


def setup_for(ch: int) -> _Setup:
    s = _SETUPS.get(ch)
    if s is None:
        s = _SETUPS[ch] = _Setup(ch)
    return s


def ident_packet(ch: int, rate: int) -> bytes:
    b0, b1 = (int(math.log2(b)) for b in BLOCKSIZES)
    return b"\x01vorbis" + struct.pack("<IBIiii", 0, ch, rate, 0, 0, 0) + bytes([b0 | (b1 << 4), 1])


def comment_packet() -> bytes:
    return b"\x03vorbis" + struct.pack("<I", len(VENDOR)) + VENDOR + struct.pack("<I", 0) + b"\x01"


def ogg_page(body: bytes, lacing, granule: int, seq: int, flags: int) -> bytes:
    hdr = (b"OggS" + bytes([0, flags]) + struct.pack("<qII", granule, SERIAL, seq) + b"\0\0\0\0" + bytes([len(lacing)]) +
           bytes(lacing))
    crc = V.ogg_crc(hdr + body)
    return hdr[:22] + struct.pack("<I", crc) + hdr[26:] + body


_HEADERS = {}


def header_pages(ch: int, rate: int):
    """(the header pages' bytes, their count): page 0 the identification header alone (BOS), then the comment and setup headers
    on pages of at most 255 lacing values; every header page carries granule 0.  Cached per (channels, rate)."""
    key = (ch, rate)
    if key in _HEADERS:
        return _HEADERS[key]
    s = setup_for(ch)
    ident = ident_packet(ch, rate)
    pages = [ogg_page(ident, [len(ident)], 0, 0, 2)]
    segs, body = [], b""
    for p in (comment_packet(), s.setup_packet):
        segs += [255] * (len(p) // 255) + [len(p) % 255]
        body += p
    seq, pos, cont = 1, 0, False
    while segs:
        take, rest = segs[:255], segs[255:]
        n = sum(take)
        pages.append(ogg_page(body[pos:pos + n], take, 0, seq, 1 if cont else 0))
        cont = take[-1] == 255
        pos += n
        seq += 1
        segs = rest
    _HEADERS[key] = (b"".join(pages), len(pages))
    return _HEADERS[key]
