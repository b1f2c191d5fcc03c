"""Ogg Vorbis (Vorbis I specification, RFC 3533 Ogg framing), host side: the Ogg page walk, the three header packets, the
codebook decode and VQ tables, and the audio-packet table.  The packets themselves are decoded on the GPU (ops.vorbis_decode,
csrc/vorbis.hip).  Every failure raises VorbisError, a ValueError whose message names the file.

Device layout of the setup (`pack_setup`): one int32 array of fixed-size records (the struct definitions in csrc/vorbis.hip
mirror the *_INTS constants below) and one float32 array (VQ values, floor1_inverse_dB_table, IMDCT twiddles, window slopes)."""
from __future__ import annotations

import dataclasses
import math

import numpy as np


class VorbisError(ValueError):
    pass


# ------------------------------------------------------------------ Ogg
_CRC_TABLE = None


def _crc_table():
    global _CRC_TABLE
    if _CRC_TABLE is None:
        t = np.zeros(256, dtype=np.uint32)
        for i in range(256):
            r = i << 24
            for _ in range(8):
                r = ((r << 1) ^ 0x04C11DB7) if r & 0x80000000 else (r << 1)
            t[i] = r & 0xFFFFFFFF
        _CRC_TABLE = [int(v) for v in t]
    return _CRC_TABLE


def ogg_crc(data) -> int:
    """Ogg's CRC-32: polynomial 0x04C11DB7, not reflected, initial 0, no final xor (computed with the CRC field zeroed)"""
    t, c = _crc_table(), 0
    for b in bytes(data):
        c = ((c << 8) & 0xFFFFFFFF) ^ t[(c >> 24) ^ b]
    return c


@dataclasses.dataclass
class Pages:
    offset: np.ndarray     # int64 file offset of each page
    body: np.ndarray       # int64 file offset of each page's body
    body_len: np.ndarray   # int64
    granule: np.ndarray    # int64 (-1: no packet ends on the page)
    flags: np.ndarray      # header type flags (1 continued, 2 BOS, 4 EOS)
    crc: np.ndarray        # stored CRC (uint32 as int64)
    serial: np.ndarray
    nseg: np.ndarray
    lacing: np.ndarray     # uint8, every page's lacing values concatenated
    seg_page: np.ndarray   # int64 page of each lacing value


def walk_pages(data: np.ndarray, name: str) -> Pages:
    """every page header of the whole file (a Python loop over pages: a header gives the next page's offset)"""
    n = len(data)
    offs, nsegs = [], []
    pos = 0
    if n < 27 or bytes(data[:4]) != b"OggS":
        raise VorbisError(f"{name}: not an Ogg stream (no 'OggS' capture pattern)")
    while pos < n:
        if pos + 27 > n:
            raise VorbisError(f"{name}: page {len(offs)} at byte offset {pos}: truncated page header")
        if data[pos] != 0x4F or data[pos + 1] != 0x67 or data[pos + 2] != 0x67 or data[pos + 3] != 0x53:
            raise VorbisError(f"{name}: page {len(offs)} at byte offset {pos}: no 'OggS' capture pattern (corrupt stream)")
        if data[pos + 4] != 0:
            raise VorbisError(f"{name}: page {len(offs)} at byte offset {pos}: Ogg stream structure version {data[pos + 4]}")
        ns = int(data[pos + 26])
        if pos + 27 + ns > n:
            raise VorbisError(f"{name}: page {len(offs)} at byte offset {pos}: truncated page (lacing runs past the end)")
        blen = int(data[pos + 27:pos + 27 + ns].sum(dtype=np.int64))
        if pos + 27 + ns + blen > n:
            raise VorbisError(f"{name}: page {len(offs)} at byte offset {pos}: truncated page (the body runs past the end "
                              f"of the file)")
        offs.append(pos)
        nsegs.append(ns)
        pos += 27 + ns + blen
    offset = np.asarray(offs, dtype=np.int64)
    nseg = np.asarray(nsegs, dtype=np.int64)
    hdr = data[offset[:, None] + np.arange(27)[None, :]]
    le = lambda a: (a.astype(np.int64) << (8 * np.arange(a.shape[1], dtype=np.int64))).sum(axis=1)  # noqa: E731
    gran_u = hdr[:, 6:14].copy().view("<i8").reshape(-1)
    seg_page = np.repeat(np.arange(len(offset), dtype=np.int64), nseg)
    seg_idx = np.arange(int(nseg.sum()), dtype=np.int64) - np.repeat(np.cumsum(nseg) - nseg, nseg)
    lacing = data[offset[seg_page] + 27 + seg_idx] if len(seg_page) else np.zeros(0, np.uint8)
    body_len = np.bincount(seg_page, weights=lacing, minlength=len(offset)).astype(np.int64)
    return Pages(offset=offset, body=offset + 27 + nseg, body_len=body_len, granule=gran_u.astype(np.int64),
                 flags=hdr[:, 5].astype(np.int64), crc=le(hdr[:, 22:26]), serial=le(hdr[:, 14:18]), nseg=nseg,
                 lacing=lacing.astype(np.uint8), seg_page=seg_page)


def page_crc_ok(data: np.ndarray, pages: Pages, i: int) -> bool:
    o, e = int(pages.offset[i]), int(pages.body[i] + pages.body_len[i])
    b = bytearray(data[o:e].tobytes())
    b[22:26] = b"\0\0\0\0"
    return ogg_crc(b) == int(pages.crc[i])


def split_packets(pages: Pages):
    """(packet start segment, packet end segment (inclusive), byte length, page the packet ends on, payload offset) per packet,
    vectorised over the lacing values: a packet ends at every lacing value below 255"""
    lac = pages.lacing.astype(np.int64)
    ends = np.flatnonzero(lac < 255)
    starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64)
    seg_end = np.cumsum(lac)  # payload offset after each segment (the page bodies concatenated)
    pay_end = seg_end[ends] if len(ends) else np.zeros(0, np.int64)
    pay_start = seg_end[starts] - lac[starts] if len(ends) else np.zeros(0, np.int64)
    return starts, ends, pay_end - pay_start, pages.seg_page[ends] if len(ends) else np.zeros(0, np.int64), pay_start


# ------------------------------------------------------------------ bit reading (headers)
class BitReader:
    """LSB-first bit reader over a bytes object (Vorbis packing)"""

    def __init__(self, b: bytes):
        self.v = int.from_bytes(b, "little")
        self.n = 8 * len(b)
        self.pos = 0

    def read(self, bits: int) -> int:
        if self.pos + bits > self.n:
            self.pos = self.n + 1
            raise EOFError
        r = (self.v >> self.pos) & ((1 << bits) - 1)
        self.pos += bits
        return r


def ilog(x: int) -> int:
    return int(x).bit_length() if x > 0 else 0


def float32_unpack(x: int) -> float:
    mantissa = x & 0x1FFFFF
    sign = x & 0x80000000
    exponent = (x & 0x7FE00000) >> 21
    if sign:
        mantissa = -mantissa
    return math.ldexp(mantissa, exponent - 788)


def lookup1_values(entries: int, dims: int) -> int:
    """the greatest r with r ** dims <= entries"""
    r = int(round(entries ** (1.0 / dims))) + 1
    while r > 0 and r ** dims > entries:
        r -= 1
    return r


def make_codewords(lengths):
    """codewords (MSB-first integers) assigned in entry order, as the Vorbis I specification's section 3.2.1 defines;
    entries of length 0 are unused (None).  An over-specified length list raises ValueError."""
    marker = [0] * 33
    out = []
    for ln in lengths:
        if ln <= 0:
            out.append(None)
            continue
        entry = marker[ln]
        if ln < 32 and (entry >> ln):
            raise ValueError("over-specified codebook lengths")
        out.append(entry)
        for j in range(ln, 0, -1):
            if marker[j] & 1:
                if j == 1:
                    marker[1] += 1
                else:
                    marker[j] = marker[j - 1] << 1
                break
            marker[j] += 1
        for j in range(ln + 1, 33):
            if (marker[j] >> 1) == entry:
                entry = marker[j]
                marker[j] = marker[j - 1] << 1
            else:
                break
    return out


# ------------------------------------------------------------------ headers
@dataclasses.dataclass
class Codebook:
    dims: int
    entries: int
    lengths: list
    codes: list
    lookup_type: int
    values: np.ndarray     # (entries, dims) float64, None for lookup type 0


@dataclasses.dataclass
class Floor1:
    partition_class: list
    class_dims: list
    class_subclasses: list
    class_masterbook: list
    subclass_books: list   # [class][subclass] book number, -1 unused
    multiplier: int
    rangebits: int
    X: list
    order: list            # post indices sorted by X
    low: list              # low_neighbor per post (posts 0, 1: 0)
    high: list


@dataclasses.dataclass
class Residue:
    type: int
    begin: int
    end: int
    partition_size: int
    classifications: int
    classbook: int
    books: list            # [classification][pass] book number, -1 unused


@dataclasses.dataclass
class Mapping:
    magnitude: list
    angle: list
    mux: list
    submap_floor: list
    submap_residue: list


@dataclasses.dataclass
class Setup:
    channels: int
    rate: int
    bitrate_max: int
    bitrate_nominal: int
    bitrate_min: int
    blocksize: tuple
    vendor: str
    comments: list
    books: list
    floor_types: list
    floors: list
    residues: list
    mappings: list
    modes: list            # (blockflag, mapping)
    setup_bits: int        # bit position of the setup header's framing bit
    key: bytes = b""       # identification fields the tables depend on + the setup packet (pack_setup's cache key)


MAX_CHANNELS = 8
MAX_POSTS = 65

_OTHER_CODECS = ((b"OpusHead", "Opus"), (b"\x7fFLAC", "FLAC"), (b"Speex   ", "Speex"), (b"\x80theora", "Theora"),
                 (b"fishead\0", "Skeleton"), (b"\x80kate", "Kate"))


def _ident(pkt: bytes, name: str):
    if len(pkt) < 30 or pkt[:7] != b"\x01vorbis":
        for magic, codec in _OTHER_CODECS:
            if pkt.startswith(magic):
                raise VorbisError(f"{name}: the Ogg stream holds {codec}, not Vorbis (Ogg Vorbis only)")
        raise VorbisError(f"{name}: bad Vorbis identification header")
    version = int.from_bytes(pkt[7:11], "little")
    ch = pkt[11]
    rate = int.from_bytes(pkt[12:16], "little")
    bmax, bnom, bmin = (int.from_bytes(pkt[16 + 4 * i:20 + 4 * i], "little", signed=True) for i in range(3))
    b0, b1 = 1 << (pkt[28] & 15), 1 << (pkt[28] >> 4)
    if version != 0:
        raise VorbisError(f"{name}: Vorbis version {version} (0 expected)")
    if ch == 0 or rate == 0:
        raise VorbisError(f"{name}: bad Vorbis identification header ({ch} channels, {rate} Hz)")
    if ch > MAX_CHANNELS:
        raise VorbisError(f"{name}: {ch} channels (at most {MAX_CHANNELS} are supported)")
    if not (64 <= b0 <= b1 <= 8192) or not (pkt[29] & 1):
        raise VorbisError(f"{name}: bad Vorbis identification header (blocksizes {b0}/{b1} or framing bit)")
    return ch, rate, bmax, bnom, bmin, (b0, b1)


def _comment(pkt: bytes, name: str):
    try:
        if pkt[:7] != b"\x03vorbis":
            raise IndexError
        p = 7
        n = int.from_bytes(pkt[p:p + 4], "little")
        vendor = pkt[p + 4:p + 4 + n].decode("utf-8", "replace")
        p += 4 + n
        cnt = int.from_bytes(pkt[p:p + 4], "little")
        p += 4
        out = []
        for _ in range(cnt):
            n = int.from_bytes(pkt[p:p + 4], "little")
            if p + 4 + n > len(pkt):
                raise IndexError
            out.append(pkt[p + 4:p + 4 + n].decode("utf-8", "replace"))
            p += 4 + n
        if p >= len(pkt) or not (pkt[p] & 1):
            raise IndexError
        return vendor, out
    except IndexError:
        raise VorbisError(f"{name}: bad Vorbis comment header") from None


def _codebook(r: BitReader, name: str, i: int) -> Codebook:
    if r.read(24) != 0x564342:
        raise VorbisError(f"{name}: bad Vorbis setup header (codebook {i} sync pattern)")
    dims, entries = r.read(16), r.read(24)
    ordered = r.read(1)
    lengths = []
    if not ordered:
        sparse = r.read(1)
        for _ in range(entries):
            if sparse and not r.read(1):
                lengths.append(0)
            else:
                lengths.append(r.read(5) + 1)
    else:
        cur = r.read(5) + 1
        while len(lengths) < entries:
            num = r.read(ilog(entries - len(lengths)))
            if len(lengths) + num > entries or cur > 32:
                raise VorbisError(f"{name}: bad Vorbis setup header (codebook {i} ordered lengths)")
            lengths += [cur] * num
            cur += 1
    lookup = r.read(4)
    values = None
    if lookup in (1, 2):
        mn, delta = float32_unpack(r.read(32)), float32_unpack(r.read(32))
        vbits, seq = r.read(4) + 1, r.read(1)
        nval = lookup1_values(entries, dims) if lookup == 1 else entries * dims
        mult = np.array([r.read(vbits) for _ in range(nval)], dtype=np.float64)
        values = np.zeros((entries, dims), dtype=np.float64)
        e = np.arange(entries)
        last = np.zeros(entries)
        div = np.ones(entries, dtype=np.int64)
        for d in range(dims):
            off = (e // div) % nval if lookup == 1 else e * dims + d
            values[:, d] = mult[off] * delta + mn + last
            if seq:
                last = values[:, d].copy()
            if lookup == 1:
                div = div * nval
    elif lookup != 0:
        raise VorbisError(f"{name}: bad Vorbis setup header (codebook {i} lookup type {lookup})")
    if dims == 0 and lookup:
        raise VorbisError(f"{name}: bad Vorbis setup header (codebook {i} has 0 dimensions)")
    try:
        codes = make_codewords(lengths)
    except ValueError:
        raise VorbisError(f"{name}: bad Vorbis setup header (codebook {i} lengths over-specify the tree)") from None
    return Codebook(dims=dims, entries=entries, lengths=lengths, codes=codes, lookup_type=lookup, values=values)


def _floor1(r: BitReader, nbooks: int, name: str) -> Floor1:
    parts = r.read(5)
    pclass = [r.read(4) for _ in range(parts)]
    nclass = max(pclass) + 1 if pclass else 0
    cdim, csub, cmaster, sbooks = [], [], [], []
    for _ in range(nclass):
        cdim.append(r.read(3) + 1)
        csub.append(r.read(2))
        cmaster.append(r.read(8) if csub[-1] else -1)
        sbooks.append([r.read(8) - 1 for _ in range(1 << csub[-1])])
    mult = r.read(2) + 1
    rangebits = r.read(4)
    X = [0, 1 << rangebits]
    for c in pclass:
        X += [r.read(rangebits) for _ in range(cdim[c])]
    if len(X) > MAX_POSTS or len(set(X)) != len(X):
        raise VorbisError(f"{name}: bad Vorbis setup header (floor 1 with {len(X)} posts or repeated X values)")
    if any(b >= nbooks for b in cmaster) or any(b >= nbooks for s in sbooks for b in s):
        raise VorbisError(f"{name}: bad Vorbis setup header (floor 1 book number out of range)")
    order = sorted(range(len(X)), key=lambda k: X[k])
    low, high = [0, 0], [0, 0]
    for j in range(2, len(X)):
        lo = max((k for k in range(j) if X[k] < X[j]), key=lambda k: X[k])
        hi = min((k for k in range(j) if X[k] > X[j]), key=lambda k: X[k])
        low.append(lo)
        high.append(hi)
    return Floor1(partition_class=pclass, class_dims=cdim, class_subclasses=csub, class_masterbook=cmaster,
                  subclass_books=sbooks, multiplier=mult, rangebits=rangebits, X=X, order=order, low=low, high=high)


def _residue(r: BitReader, rtype: int, nbooks: int, name: str) -> Residue:
    begin, end, psize = r.read(24), r.read(24), r.read(24) + 1
    ncls, classbook = r.read(6) + 1, r.read(8)
    cascade = []
    for _ in range(ncls):
        low = r.read(3)
        high = r.read(5) if r.read(1) else 0
        cascade.append(high * 8 + low)
    books = [[(r.read(8) if (cascade[c] >> p) & 1 else -1) for p in range(8)] for c in range(ncls)]
    if classbook >= nbooks or any(b >= nbooks for row in books for b in row):
        raise VorbisError(f"{name}: bad Vorbis setup header (residue book number out of range)")
    return Residue(type=rtype, begin=begin, end=end, partition_size=psize, classifications=ncls, classbook=classbook, books=books)


def _setup(pkt: bytes, ch: int, name: str):
    if pkt[:7] != b"\x05vorbis":
        raise VorbisError(f"{name}: bad Vorbis setup header")
    r = BitReader(pkt[7:])
    try:
        books = [_codebook(r, name, i) for i in range(r.read(8) + 1)]
        for _ in range(r.read(6) + 1):
            if r.read(16) != 0:
                raise VorbisError(f"{name}: bad Vorbis setup header (time domain transform)")
        ftypes, floors = [], []
        for _ in range(r.read(6) + 1):
            t = r.read(16)
            if t == 0:
                raise VorbisError(f"{name}: floor type 0 is not supported (no encoder after Xiph's beta 4 writes it)")
            if t != 1:
                raise VorbisError(f"{name}: bad Vorbis setup header (floor type {t})")
            ftypes.append(t)
            floors.append(_floor1(r, len(books), name))
        residues = []
        for _ in range(r.read(6) + 1):
            t = r.read(16)
            if t > 2:
                raise VorbisError(f"{name}: bad Vorbis setup header (residue type {t})")
            residues.append(_residue(r, t, len(books), name))
        mappings = []
        for _ in range(r.read(6) + 1):
            if r.read(16) != 0:
                raise VorbisError(f"{name}: bad Vorbis setup header (mapping type)")
            submaps = r.read(4) + 1 if r.read(1) else 1
            mag, ang = [], []
            if r.read(1):
                for _ in range(r.read(8) + 1):
                    mag.append(r.read(ilog(ch - 1)))
                    ang.append(r.read(ilog(ch - 1)))
                    if mag[-1] == ang[-1] or mag[-1] >= ch or ang[-1] >= ch:
                        raise VorbisError(f"{name}: bad Vorbis setup header (coupling channels)")
            if r.read(2) != 0:
                raise VorbisError(f"{name}: bad Vorbis setup header (mapping reserved field)")
            mux = [r.read(4) if submaps > 1 else 0 for _ in range(ch)] if submaps > 1 else [0] * ch
            sf, sr = [], []
            for _ in range(submaps):
                r.read(8)
                sf.append(r.read(8))
                sr.append(r.read(8))
            if any(m >= submaps for m in mux) or any(f >= len(floors) for f in sf) or any(x >= len(residues) for x in sr):
                raise VorbisError(f"{name}: bad Vorbis setup header (mapping submaps)")
            mappings.append(Mapping(magnitude=mag, angle=ang, mux=mux, submap_floor=sf, submap_residue=sr))
        modes = []
        for _ in range(r.read(6) + 1):
            bf, wt, tt, mp = r.read(1), r.read(16), r.read(16), r.read(8)
            if wt or tt or mp >= len(mappings):
                raise VorbisError(f"{name}: bad Vorbis setup header (mode)")
            modes.append((bf, mp))
        framing_at = r.pos
        if not r.read(1):
            raise VorbisError(f"{name}: bad Vorbis setup header (framing bit)")
    except EOFError:
        raise VorbisError(f"{name}: bad Vorbis setup header (it ends early)") from None
    return books, ftypes, floors, residues, mappings, modes, 56 + framing_at


@dataclasses.dataclass
class VorbisStream:
    setup: Setup
    pages: Pages
    header_pages: int      # pages holding (parts of) the three header packets
    pkt_len: np.ndarray    # int64 byte length of each audio packet
    pkt_pay: np.ndarray    # int64 payload offset (page bodies concatenated) of each audio packet
    pkt_page: np.ndarray   # int64 page each audio packet ends on
    pkt_blockflag: np.ndarray  # int64 0 short / 1 long
    frames: int            # frames after trimming
    trim_start: int        # frames dropped at the start
    returned: int          # frames before trimming


def _packet_bytes(data, pages, starts, ends, pay_off, k):
    segs = np.arange(starts[k], ends[k] + 1)
    within = np.concatenate([[0], np.cumsum(pages.lacing.astype(np.int64))])
    seg_pay = within[segs]
    seg_file = pages.body[pages.seg_page[segs]] + (seg_pay - pay_off[pages.seg_page[segs]])
    return b"".join(data[f:f + int(pages.lacing[s])].tobytes() for f, s in zip(seg_file, segs))


def parse(data, name: str = "<bytes>") -> VorbisStream:
    """headers, setup and the audio-packet table of a whole Ogg Vorbis file held in memory"""
    data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    if len(data) < 4 or bytes(data[:4]) != b"OggS":
        raise VorbisError(f"{name}: not an Ogg stream (no 'OggS' capture pattern)")
    pages = walk_pages(data, name)
    if len(np.unique(pages.serial)) > 1:
        raise VorbisError(f"{name}: {len(np.unique(pages.serial))} logical streams (chained or multiplexed Ogg is not supported)")
    if int(np.count_nonzero(pages.flags & 2)) > 1:
        raise VorbisError(f"{name}: more than one logical stream (chained Ogg is not supported)")
    starts, ends, plen, ppage, ppay = split_packets(pages)
    pay_off = np.concatenate([[0], np.cumsum(pages.body_len)])  # payload offset of each page's body
    if len(plen) < 3:
        # the first packet may still name another codec
        if len(plen) >= 1:
            _ident(_packet_bytes(data, pages, starts, ends, pay_off, 0), name)
        raise VorbisError(f"{name}: bad or missing Vorbis header packets")
    heads = [_packet_bytes(data, pages, starts, ends, pay_off, k) for k in range(3)]
    ch, rate, bmax, bnom, bmin, bs = _ident(heads[0], name)
    nhdr_pages = int(ppage[2]) + 1
    for i in range(nhdr_pages):
        if not page_crc_ok(data, pages, i):
            raise VorbisError(f"{name}: page {i} at byte offset {int(pages.offset[i])}: header page CRC mismatch")
    vendor, comments = _comment(heads[1], name)
    key = bytes([ch]) + heads[0][28:29] + heads[2]
    parsed = _SETUP_CACHE.get(key)
    if parsed is None:  # files of one encoder setting share their setup header: it is parsed once
        parsed = _setup(heads[2], ch, name)
        if len(_SETUP_CACHE) >= _CACHE_MAX:
            _SETUP_CACHE.clear()
        _SETUP_CACHE[key] = parsed
    books, ftypes, floors, residues, mappings, modes, setup_bits = parsed
    setup = Setup(channels=ch, rate=rate, bitrate_max=bmax, bitrate_nominal=bnom, bitrate_min=bmin, blocksize=bs, vendor=vendor,
                  comments=comments, books=books, floor_types=ftypes, floors=floors, residues=residues, mappings=mappings,
                  modes=modes, setup_bits=setup_bits, key=key)
    # audio packets: drop zero-length ones (they carry nothing) and read each mode number from the first byte
    plen, ppage, ppay = plen[3:], ppage[3:], ppay[3:]
    keep = plen > 0
    plen, ppage, ppay = plen[keep], ppage[keep], ppay[keep]
    if int(ppage[0] if len(ppage) else nhdr_pages) < nhdr_pages - 1:
        raise VorbisError(f"{name}: bad Vorbis header pages")
    first_byte_file = _pay_to_file(pages, pay_off, ppay)
    b0 = data[first_byte_file].astype(np.int64) if len(ppay) else np.zeros(0, np.int64)
    mbits = ilog(len(modes) - 1)
    mode = (b0 >> 1) & ((1 << mbits) - 1)
    bad = np.flatnonzero((b0 & 1) | (mode >= len(modes)))
    if len(bad):
        k = int(bad[0])
        raise VorbisError(f"{name}: page {int(ppage[k])} at byte offset {int(pages.offset[ppage[k]])}: audio packet {k} is not "
                          f"an audio packet or names mode {int(mode[k])} of {len(modes)} (corrupt stream)")
    bflag = np.asarray([m[0] for m in modes], dtype=np.int64)[mode] if len(mode) else np.zeros(0, np.int64)
    nblk = np.where(bflag == 1, bs[1], bs[0])
    ret = np.zeros(len(nblk), dtype=np.int64)
    ret[1:] = nblk[:-1] // 4 + nblk[1:] // 4
    cum = np.cumsum(ret)
    returned = int(cum[-1]) if len(cum) else 0
    trim_start, frames = 0, returned
    if len(ppage):
        # start: the first audio page's granule counts the frames through its last packet; more decoded frames than that means
        # the stream starts part-way (the excess is dropped from the front).  end: the last page's granule is the total.
        first_page = int(ppage[0])
        on_first = np.flatnonzero(ppage == first_page)
        g_first = int(pages.granule[first_page])
        last_page = len(pages.offset) - 1
        g_last = int(pages.granule[last_page])
        if first_page != last_page and g_first >= 0 and int(cum[on_first[-1]]) > g_first:
            trim_start = int(cum[on_first[-1]]) - g_first
        if g_last >= 0 and (pages.flags[last_page] & 4):
            frames = max(0, min(returned, g_last + trim_start) - trim_start)
        else:
            frames = returned - trim_start
    return VorbisStream(setup=setup, pages=pages, header_pages=nhdr_pages, pkt_len=plen, pkt_pay=ppay, pkt_page=ppage,
                        pkt_blockflag=bflag, frames=frames,
                        trim_start=trim_start, returned=returned)


def _pay_to_file(pages, pay_off, pay):
    """file offset of payload offsets (each inside some page body)"""
    pg = np.searchsorted(pay_off, pay, side="right") - 1  # (side="right" skips pages with empty bodies)
    return pages.body[pg] + (pay - pay_off[pg])


def packet_bytes(data, vs: VorbisStream, k: int) -> bytes:
    """audio packet k's bytes, page headers removed (test and debugging helper)"""
    data = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else data
    pay_off = np.concatenate([[0], np.cumsum(vs.pages.body_len)])
    payload = np.concatenate([data[int(b):int(b + n)] for b, n in zip(vs.pages.body, vs.pages.body_len)])
    assert len(payload) == pay_off[-1]
    return payload[int(vs.pkt_pay[k]):int(vs.pkt_pay[k] + vs.pkt_len[k])].tobytes()


# ------------------------------------------------------------------ header-only read (wavio.info, create_dataset counting)
@dataclasses.dataclass
class VorbisInfo:
    channels: int
    sample_rate: int
    blocksize: tuple
    frames: int            # frames the decoder returns (after the granule trims)


def read_header(path: str) -> VorbisInfo:
    """channels, rate, blocksizes and the number of frames the decoder returns, from the host parse alone (pages, headers,
    packet table and the granule trims; nothing is decoded): the same count as ops.vorbis_decode's output, so create_dataset's
    numbering across ranks agrees with what each rank decodes."""
    try:
        raw = np.fromfile(path, dtype=np.uint8)
    except OSError as e:
        raise VorbisError(f"{path}: cannot read the ogg file ({e.strerror or e})") from e
    vs = parse(raw, path)
    return VorbisInfo(channels=vs.setup.channels, sample_rate=vs.setup.rate, blocksize=vs.setup.blocksize, frames=vs.frames)


# ------------------------------------------------------------------ device tables
PRIMARY_BITS = 10
BOOK_INTS = 8       # dims, entries, pbits, nsorted, prim_off, sorted_off, vq_off (float index, -1 none), lookup
FLOOR_INTS = 4 + 32 + 3 * 16 + 16 * 8 + 4 * 68
RES_INTS = 8 + 64 * 8
MAP_INTS = 4 + 2 * 256 + 8 + 2 * 16
HEAD_INTS = 32


def pack_setup(s: Setup):
    """(int32 array, float32 array) the decode kernels read; layout in csrc/vorbis.hip (the H_ / F_ / M_ offsets there).
    Cached per setup (Setup.key): the arrays are shared, not to be written."""
    if s.key and s.key in _PACK_CACHE:
        return _PACK_CACHE[s.key]
    out = _pack_setup(s)
    if s.key:
        if len(_PACK_CACHE) >= _CACHE_MAX:
            _PACK_CACHE.clear()
        _PACK_CACHE[s.key] = out
    return out


_SETUP_CACHE, _PACK_CACHE, _CACHE_MAX = {}, {}, 16


def _pack_setup(s: Setup):
    ints = np.zeros(HEAD_INTS, dtype=np.int64)
    nb, nf, nr, nm, nmode = len(s.books), len(s.floors), len(s.residues), len(s.mappings), len(s.modes)
    book_off = HEAD_INTS
    floor_off = book_off + nb * BOOK_INTS
    res_off = floor_off + nf * FLOOR_INTS
    map_off = res_off + nr * RES_INTS
    mode_off = map_off + nm * MAP_INTS
    tab_off = mode_off + nmode * 4
    ints[:16] = [s.channels, s.blocksize[0], s.blocksize[1], nmode, nf, nr, nm, nb, book_off, floor_off, res_off, map_off,
                 mode_off, ilog(nmode - 1), 0, 0]
    recs = np.zeros(tab_off - HEAD_INTS, dtype=np.int64)
    tabs = []
    floats = []
    fpos = 0
    tpos = tab_off

    def put_tab(arr):
        nonlocal tpos
        o = tpos
        tabs.append(np.asarray(arr, dtype=np.int64))
        tpos += len(arr)
        return o

    for i, b in enumerate(s.books):
        maxlen = max(b.lengths) if any(b.lengths) else 0
        pbits = min(PRIMARY_BITS, max(maxlen, 1))
        prim = np.full(1 << pbits, -1, dtype=np.int64)
        sorted_rows = []
        for e, (ln, code) in enumerate(zip(b.lengths, b.codes)):
            if code is None:
                continue
            rev = int(format(code, f"0{ln}b")[::-1], 2)
            if ln <= pbits:
                prim[rev::1 << ln] = e | (ln << 24)
            sorted_rows.append(((code << (32 - ln)) & 0xFFFFFFFF, ln, e))
        sorted_rows.sort()
        srt = np.asarray([v for row in sorted_rows for v in (row[0] - (1 << 32) if row[0] >= 1 << 31 else row[0],
                                                               row[1] | (row[2] << 8))], dtype=np.int64)
        po = put_tab(prim)
        so = put_tab(srt)
        vq = -1
        if b.lookup_type:
            vq = fpos
            floats.append(b.values.astype(np.float32).reshape(-1))
            fpos += b.values.size
        o = book_off - HEAD_INTS + i * BOOK_INTS
        recs[o:o + BOOK_INTS] = [b.dims, b.entries, pbits, len(sorted_rows), po, so, vq, b.lookup_type]
    for i, f in enumerate(s.floors):
        rec = np.full(FLOOR_INTS, -1, dtype=np.int64)
        rec[:4] = [len(f.partition_class), f.multiplier, f.rangebits, len(f.X)]
        rec[4:4 + len(f.partition_class)] = f.partition_class
        nc = len(f.class_dims)
        rec[36:36 + nc] = f.class_dims
        rec[52:52 + nc] = f.class_subclasses
        rec[68:68 + nc] = f.class_masterbook
        for c in range(nc):
            rec[84 + 8 * c:84 + 8 * c + len(f.subclass_books[c])] = f.subclass_books[c]
        nx = len(f.X)
        rec[212:212 + nx] = f.X
        rec[280:280 + nx] = f.order
        rec[348:348 + nx] = f.low
        rec[416:416 + nx] = f.high
        o = floor_off - HEAD_INTS + i * FLOOR_INTS
        recs[o:o + FLOOR_INTS] = rec
    for i, r in enumerate(s.residues):
        rec = np.full(RES_INTS, -1, dtype=np.int64)
        rec[:8] = [r.type, r.begin, r.end, r.partition_size, r.classifications, r.classbook, s.books[r.classbook].dims, 0]
        for c in range(r.classifications):
            rec[8 + 8 * c:16 + 8 * c] = r.books[c]
        o = res_off - HEAD_INTS + i * RES_INTS
        recs[o:o + RES_INTS] = rec
    for i, m in enumerate(s.mappings):
        rec = np.zeros(MAP_INTS, dtype=np.int64)
        rec[:2] = [len(m.submap_floor), len(m.magnitude)]
        rec[4:4 + len(m.magnitude)] = m.magnitude
        rec[260:260 + len(m.angle)] = m.angle
        rec[516:516 + s.channels] = m.mux
        rec[524:524 + len(m.submap_floor)] = m.submap_floor
        rec[540:540 + len(m.submap_residue)] = m.submap_residue
        o = map_off - HEAD_INTS + i * MAP_INTS
        recs[o:o + MAP_INTS] = rec
    for i, (bf, mp) in enumerate(s.modes):
        o = mode_off - HEAD_INTS + i * 4
        recs[o:o + 2] = [bf, mp]
    # floats: VQ values, then the dB table, then per blocksize (short, long) the IMDCT twiddles and the window slope
    db_off = fpos
    floats.append(inverse_db_table().astype(np.float32))
    fpos += 256
    tw = []
    for n in s.blocksize:
        block = np.concatenate([dct4_tables(n // 2), window_slope(n // 2)]).astype(np.float32)
        tw.append(fpos)
        floats.append(block)
        fpos += len(block)
    ints[16:19] = [db_off, tw[0], tw[1]]
    allints = np.concatenate([ints, recs] + tabs)
    assert allints.min() >= -(1 << 31) and allints.max() < (1 << 31)
    return allints.astype(np.int32), np.concatenate(floats).astype(np.float32)


def dct4_tables(M: int) -> np.ndarray:
    """the tables of csrc/fft_radix2.h's dct4_lds for M coefficients, as (re, im) pairs one after the other (float64):
    pre[t] = e^{-i pi (t + 1/4) / M} and post[t] = e^{-i pi t / M}, t < M / 2; fft[j] = e^{-2 pi i j / (M / 2)}, j < M / 4"""
    t = np.arange(M // 2)
    pre = np.exp(-1j * np.pi * (t + 0.25) / M)
    post = np.exp(-1j * np.pi * t / M)
    fft = np.exp(-2j * np.pi * np.arange(max(M // 4, 1)) / (M // 2))
    return np.concatenate([np.stack([z.real, z.imag], 1).reshape(-1) for z in (pre, post, fft)])


def inverse_db_table() -> np.ndarray:
    """floor1_inverse_dB_table: 1.0649863e-7 * 1.0649863 ** i (float64)"""
    return 1.0649863e-7 * 1.0649863 ** np.arange(256, dtype=np.float64)


def window_slope(m: int) -> np.ndarray:
    """the rising half of a Vorbis window of m samples: sin(pi/2 * sin^2((x + 1/2) / m * pi/2)) (float64)"""
    x = (np.arange(m, dtype=np.float64) + 0.5) / m * (np.pi / 2)
    return np.sin(np.pi / 2 * np.sin(x) ** 2)
