"""Ogg Vorbis stream writer for the tests.  Not an encoder: it lays out chosen Vorbis packets (the fixture's headers and audio
packets, in any order and number) as Ogg pages with chosen page sizes and granule positions, and computes the page CRCs, so a
test can build packets that span pages, long streams, start and end trimming, and corrupt or truncated pages."""
from __future__ import annotations

import os
import struct

import numpy as np

from musicgan_amd.audio import vorbis as V

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "invalid_keypress.ogg")


def fixture_bytes() -> bytes:
    with open(FIXTURE, "rb") as fh:
        return fh.read()


def fixture_packets():
    """(the three header packets, the audio packets) of the fixture"""
    data = fixture_bytes()
    vs = V.parse(data, FIXTURE)
    pages = vs.pages
    starts, ends, _, _, _ = V.split_packets(pages)
    pay_off = np.concatenate([[0], np.cumsum(pages.body_len)])
    heads = [V._packet_bytes(np.frombuffer(data, np.uint8), pages, starts, ends, pay_off, k) for k in range(3)]
    audio = [V.packet_bytes(data, vs, k) for k in range(len(vs.pkt_len))]
    return heads, audio, vs.setup


def page(payload_segments, granule, seq, flags, serial=0x1234):
    lacing = bytes(payload_segments[1])
    body = payload_segments[0]
    hdr = b"OggS" + bytes([0, flags]) + struct.pack("<qII", granule, serial, seq) + b"\0\0\0\0" + bytes([len(lacing)]) + lacing
    crc = V.ogg_crc(hdr + body)
    return hdr[:22] + struct.pack("<I", crc) + hdr[26:] + body


def paginate(packets, granules, max_segments=255, first_seq=0, serial=0x1234, bos=True, eos=True, first_flags=0):
    """packets laid out in pages of at most `max_segments` lacing values (a packet continues on the next page when it does not
    fit); granules[k]: granule position after packet k (-1 for header packets).  A page's granule is that of the last packet
    ending on it, -1 when none ends there."""
    out = []
    segs, body, gran, cont = [], b"", -1, False
    seq = first_seq

    def flush(last=False):
        nonlocal segs, body, gran, cont, seq
        flags = (1 if cont else 0) | (2 if (bos and seq == first_seq) else 0) | (4 if (eos and last) else 0)
        out.append(page((body, segs), gran, seq, flags, serial))
        seq += 1
        segs, body, gran = [], b"", -1

    for k, p in enumerate(packets):
        lac = [255] * (len(p) // 255) + [len(p) % 255]
        pos = 0
        for i, ln in enumerate(lac):
            if len(segs) == max_segments:
                flush()
                cont = i > 0  # the new page starts inside this packet
            segs.append(ln)
            body += p[pos:pos + ln]
            pos += ln
        gran = granules[k]
    flush(last=True)
    return b"".join(out)


def returned_counts(audio_packets, setup):
    """frames each audio packet returns (the first none)"""
    mb = V.ilog(len(setup.modes) - 1)
    ns = [setup.blocksize[setup.modes[(p[0] >> 1) & ((1 << mb) - 1)][0]] for p in audio_packets]
    return [0] + [ns[i - 1] // 4 + ns[i] // 4 for i in range(1, len(ns))]


def stream(audio_packets, heads=None, max_segments=255, end_trim=0, start_trim=0, header_pages_apart=True):
    """a stream of the fixture's headers and `audio_packets`; the last page's granule drops `end_trim` frames, the first audio
    page's granule says `start_trim` frames fewer than its packets return"""
    if heads is None:
        heads, _, _ = fixture_packets()
    setup = V.parse(fixture_bytes(), FIXTURE).setup
    cnt = returned_counts(audio_packets, setup)
    cum, g = [], 0
    for c in cnt:
        g += c
        cum.append(g)
    cum = [c - start_trim for c in cum]
    cum[-1] -= end_trim
    hdr = paginate(heads[:1], [0], 255, 0, eos=False) + paginate(heads[1:], [0, 0], 255, 1, bos=False, eos=False)
    audio = paginate(audio_packets, cum, max_segments, 2, bos=False)
    return hdr + audio


# ------------------------------------------------------------------ a stream writer from chosen parameters
# Not an encoder: it writes identification, comment and setup headers for chosen codebooks, floors, residues, mappings and modes,
# and audio packets that code chosen (or random) symbols with those codebooks, walking the packet syntax of the Vorbis I
# specification in writing order.  Codewords, VQ values and floor neighbours are computed here from the parameters (not by
# musicgan_amd.audio.vorbis), and Spec.setup() hands them to the reader.

class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        assert 0 <= v < (1 << n) or n == 0, (v, n)
        self.bits.extend((v >> i) & 1 for i in range(n))

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[k + i] << i for i in range(8)) for k in range(0, len(b), 8))


def _lowest_free_codewords(lengths):
    """each used entry, in order, takes the lowest-valued codeword of its length that is neither a prefix of an assigned one nor
    has one as a prefix (the specification's section 3.2.1 rule, by search)"""
    taken, out = [], []
    for ln in lengths:
        if ln == 0:
            out.append(None)
            continue
        for v in range(1 << ln):
            if all(not ((tl <= ln and (v >> (ln - tl)) == tv) or (tl > ln and (tv >> (tl - ln)) == v)) for tv, tl in taken):
                break
        else:
            raise ValueError("over-specified lengths")
        taken.append((v, ln))
        out.append(v)
    return out


def f32pack(v: float) -> int:
    """the 32-bit Vorbis float of a dyadic value with at most 21 significant bits"""
    if v == 0:
        return 0
    a = abs(v)
    k = 20 - int(np.floor(np.log2(a)))
    m = a * 2.0 ** k
    assert m == int(m) and m < (1 << 21), v
    e = 788 - k
    assert 0 <= e < 1024
    return (0x80000000 if v < 0 else 0) | (e << 21) | int(m)


class Book:
    def __init__(self, lengths, dims=1, lookup=0, mult=None, minv=0.0, delta=1.0, vbits=None, seq=False, ordered=False):
        self.lengths, self.dims, self.lookup, self.minv, self.delta, self.seq, self.ordered = \
            list(lengths), dims, lookup, minv, delta, seq, ordered
        self.entries = len(self.lengths)
        if ordered:
            assert all(a <= b for a, b in zip(self.lengths, self.lengths[1:])) and 0 not in self.lengths
        self.sparse = 0 in self.lengths
        self.codes = _lowest_free_codewords(self.lengths)
        self.mult = list(mult or [])
        self.values = None
        if lookup:
            n = V.lookup1_values(self.entries, dims) if lookup == 1 else self.entries * dims
            assert len(self.mult) == n, (len(self.mult), n)
            self.vbits = vbits or max(1, max(self.mult).bit_length())
            vals = np.zeros((self.entries, dims))
            for e in range(self.entries):
                last, div = 0.0, 1
                for d in range(dims):
                    off = (e // div) % n if lookup == 1 else e * dims + d
                    vals[e, d] = self.mult[off] * delta + minv + last
                    if seq:
                        last = vals[e, d]
                    div *= n
            self.values = vals

    def used(self):
        return [e for e, ln in enumerate(self.lengths) if ln]

    def write_header(self, w: BitWriter):
        w.put(0x564342, 24)
        w.put(self.dims, 16)
        w.put(self.entries, 24)
        w.put(int(self.ordered), 1)
        if self.ordered:
            cur = self.lengths[0]
            w.put(cur - 1, 5)
            i = 0
            while i < self.entries:
                num = sum(1 for ln in self.lengths[i:] if ln == cur)
                w.put(num, V.ilog(self.entries - i))
                i += num
                cur += 1
        else:
            w.put(int(self.sparse), 1)
            for ln in self.lengths:
                if self.sparse:
                    w.put(int(ln > 0), 1)
                    if ln:
                        w.put(ln - 1, 5)
                else:
                    w.put(ln - 1, 5)
        w.put(self.lookup, 4)
        if self.lookup:
            w.put(f32pack(self.minv), 32)
            w.put(f32pack(self.delta), 32)
            w.put(self.vbits - 1, 4)
            w.put(int(self.seq), 1)
            for m in self.mult:
                w.put(m, self.vbits)

    def write(self, w: BitWriter, e: int):
        ln, code = self.lengths[e], self.codes[e]
        assert ln, e
        for i in range(ln - 1, -1, -1):  # most significant bit first
            w.put((code >> i) & 1, 1)


class Floor:
    def __init__(self, mult, rangebits, partition_class, classes, xs):
        """classes: (dims, subclass bits, master book or -1, [sub books, -1 unused]); xs: the posts after the first two"""
        self.mult, self.rangebits, self.partition_class, self.classes = mult, rangebits, list(partition_class), classes
        self.X = [0, 1 << rangebits] + list(xs)
        assert len(self.X) == 2 + sum(classes[c][0] for c in partition_class) and len(set(self.X)) == len(self.X)
        self.order = sorted(range(len(self.X)), key=lambda k: self.X[k])
        self.low, self.high = [0, 0], [0, 0]
        for j in range(2, len(self.X)):
            below = [k for k in range(j) if self.X[k] < self.X[j]]
            above = [k for k in range(j) if self.X[k] > self.X[j]]
            self.low.append(max(below, key=lambda k: self.X[k]))
            self.high.append(min(above, key=lambda k: self.X[k]))

    @property
    def range(self):
        return [256, 128, 86, 64][self.mult - 1]

    def write_header(self, w):
        w.put(1, 16)
        w.put(len(self.partition_class), 5)
        for c in self.partition_class:
            w.put(c, 4)
        for dims, cbits, master, subs in self.classes:
            w.put(dims - 1, 3)
            w.put(cbits, 2)
            if cbits:
                w.put(master, 8)
            for b in subs:
                w.put(b + 1, 8)
        w.put(self.mult - 1, 2)
        w.put(self.rangebits, 4)
        for x in self.X[2:]:
            w.put(x, self.rangebits)


class Residue:
    def __init__(self, rtype, begin, end, psize, classbook, books):
        self.type, self.begin, self.end, self.partition_size, self.classbook = rtype, begin, end, psize, classbook
        self.books = [list(r) + [-1] * (8 - len(r)) for r in books]
        self.classifications = len(self.books)

    def write_header(self, w):
        w.put(self.type, 16)
        w.put(self.begin, 24)
        w.put(self.end, 24)
        w.put(self.partition_size - 1, 24)
        w.put(self.classifications - 1, 6)
        w.put(self.classbook, 8)
        for row in self.books:
            casc = sum(1 << p for p in range(8) if row[p] >= 0)
            w.put(casc & 7, 3)
            w.put(int(casc > 7), 1)
            if casc > 7:
                w.put(casc >> 3, 5)
        for row in self.books:
            for p in range(8):
                if row[p] >= 0:
                    w.put(row[p], 8)


class Mapping:
    def __init__(self, mux, submap_floor, submap_residue, coupling=()):
        self.mux, self.submap_floor, self.submap_residue = list(mux), list(submap_floor), list(submap_residue)
        self.magnitude = [a for a, _ in coupling]
        self.angle = [b for _, b in coupling]

    def write_header(self, w, ch):
        w.put(0, 16)
        sub = len(self.submap_floor)
        w.put(int(sub > 1), 1)
        if sub > 1:
            w.put(sub - 1, 4)
        w.put(int(bool(self.magnitude)), 1)
        if self.magnitude:
            w.put(len(self.magnitude) - 1, 8)
            for a, b in zip(self.magnitude, self.angle):
                w.put(a, V.ilog(ch - 1))
                w.put(b, V.ilog(ch - 1))
        w.put(0, 2)
        if sub > 1:
            for m in self.mux:
                w.put(m, 4)
        for f, r in zip(self.submap_floor, self.submap_residue):
            w.put(0, 8)
            w.put(f, 8)
            w.put(r, 8)


class Spec:
    """a stream's parameters; headers(), packet() and stream() write it"""

    def __init__(self, channels, blocksize, books, floors, residues, mappings, modes, rate=44100):
        self.channels, self.blocksize, self.books, self.floors = channels, tuple(blocksize), books, floors
        self.residues, self.mappings, self.modes, self.rate = residues, mappings, list(modes), rate

    def headers(self):
        b0, b1 = (int(np.log2(b)) for b in self.blocksize)
        ident = b"\x01vorbis" + struct.pack("<IBIiii", 0, self.channels, self.rate, 0, 128000, 0) + bytes([b0 | (b1 << 4), 1])
        vendor = b"vorbis_writer"
        comment = b"\x03vorbis" + struct.pack("<I", len(vendor)) + vendor + struct.pack("<I", 0) + b"\x01"
        w = BitWriter()
        w.put(len(self.books) - 1, 8)
        for b in self.books:
            b.write_header(w)
        w.put(0, 6)
        w.put(0, 16)
        w.put(len(self.floors) - 1, 6)
        for f in self.floors:
            f.write_header(w)
        w.put(len(self.residues) - 1, 6)
        for r in self.residues:
            r.write_header(w)
        w.put(len(self.mappings) - 1, 6)
        for m in self.mappings:
            m.write_header(w, self.channels)
        w.put(len(self.modes) - 1, 6)
        for bf, mp in self.modes:
            w.put(bf, 1)
            w.put(0, 16)
            w.put(0, 16)
            w.put(mp, 8)
        w.put(1, 1)
        return [ident, comment, b"\x05vorbis" + w.tobytes()]

    def setup(self):
        """the decode setup as the reader reads it, built from these parameters"""
        books = [V.Codebook(dims=b.dims, entries=b.entries, lengths=b.lengths, codes=b.codes, lookup_type=b.lookup,
                            values=b.values) for b in self.books]
        floors = [V.Floor1(partition_class=f.partition_class, class_dims=[c[0] for c in f.classes],
                           class_subclasses=[c[1] for c in f.classes], class_masterbook=[c[2] for c in f.classes],
                           subclass_books=[c[3] for c in f.classes], multiplier=f.mult, rangebits=f.rangebits, X=f.X,
                           order=f.order, low=f.low, high=f.high) for f in self.floors]
        return V.Setup(channels=self.channels, rate=self.rate, bitrate_max=0, bitrate_nominal=128000, bitrate_min=0,
                       blocksize=self.blocksize, vendor="", comments=[], books=books, floor_types=[1] * len(floors),
                       floors=floors, residues=self.residues, mappings=self.mappings, modes=self.modes, setup_bits=0)

    # ---- audio packets
    def packet(self, mode, prev=1, nxt=1, floors=None, rng=None, classify=None, entry=None):
        """one audio packet -> (bytes, bit position where the floors end).  floors: per channel None (unused) or (Y list, the
        subclass chosen per post or None); with `rng` the unlisted choices are random.  classify(j, partition) -> class,
        entry(book, j, position) -> entry: the residue's symbols (random when not given)"""
        rng = rng or np.random.default_rng(0)
        w = BitWriter()
        w.put(0, 1)
        w.put(mode, V.ilog(len(self.modes) - 1))
        bf, mp = self.modes[mode]
        if bf:
            w.put(prev, 1)
            w.put(nxt, 1)
        m = self.mappings[mp]
        n2 = self.blocksize[bf] // 2
        used = []
        for c in range(self.channels):
            f = self.floors[m.submap_floor[m.mux[c]]]
            spec = floors[c] if floors is not None else "random"
            if spec == "random":
                spec = None if rng.random() < 0.2 else self._random_floor(f, rng)
            if spec is None:
                w.put(0, 1)
                used.append(False)
                continue
            used.append(True)
            self._write_floor(w, f, *spec)
        floor_end = len(w.bits)
        nz = list(used)
        for a, b in zip(m.magnitude, m.angle):
            if nz[a] or nz[b]:
                nz[a] = nz[b] = True
        classify = classify or (lambda j, p: int(rng.integers(0, 1 << 30)))
        entry = entry or (lambda book, j, pos: int(rng.choice(self.books[book].used())))
        for s in range(len(m.submap_floor)):
            chans = [c for c in range(self.channels) if m.mux[c] == s]
            r = self.residues[m.submap_residue[s]]
            dnd = [not nz[c] for c in chans]
            if r.type == 2:
                if not all(dnd):
                    self._write_residue(w, r, 1, [False], n2 * len(chans), 1, classify, entry)
            else:
                self._write_residue(w, r, len(chans), dnd, n2, r.type, classify, entry)
        return w.tobytes(), floor_end

    def _random_floor(self, f, rng):
        Y = [int(rng.integers(0, f.range)), int(rng.integers(0, f.range))]
        subs = []
        for c in f.partition_class:
            dims, cbits, _, sb = f.classes[c]
            for _ in range(dims):
                k = int(rng.integers(0, 1 << cbits))
                subs.append(k)
                Y.append(0 if sb[k] < 0 else int(rng.choice(self.books[sb[k]].used())))
        return Y, subs

    def _write_floor(self, w, f, Y, subs=None):
        w.put(1, 1)
        bits = V.ilog(f.range - 1)
        w.put(Y[0], bits)
        w.put(Y[1], bits)
        off = 2
        for c in f.partition_class:
            dims, cbits, master, sb = f.classes[c]
            ks = []
            for j in range(dims):
                if subs is not None:
                    k = subs[off - 2 + j]
                else:  # the first subclass whose book can code the value (or that codes nothing, for 0)
                    k = next(k for k in range(1 << cbits) if (sb[k] < 0 and Y[off + j] == 0) or
                             (sb[k] >= 0 and Y[off + j] < self.books[sb[k]].entries and self.books[sb[k]].lengths[Y[off + j]]))
                ks.append(k)
            if cbits:
                self.books[master].write(w, sum(k << (cbits * j) for j, k in enumerate(ks)))
            for j, k in enumerate(ks):
                if sb[k] >= 0:
                    self.books[sb[k]].write(w, Y[off + j])
                else:
                    assert Y[off + j] == 0
            off += dims

    def _write_residue(self, w, r, vecs, dnd, size, kind, classify, entry):
        begin, end = min(r.begin, size), min(r.end, size)
        cb = self.books[r.classbook]
        cpc, ncls = cb.dims, r.classifications
        parts = max(0, end - begin) // r.partition_size
        if parts == 0:
            return
        cls = {}
        for p in range(8):
            pc = 0
            while pc < parts:
                if p == 0:
                    for j in range(vecs):
                        if dnd[j]:
                            continue
                        digits = [classify(j, pc + i) % ncls if pc + i < parts else 0 for i in range(cpc)]
                        temp = 0
                        for d in digits:
                            temp = temp * ncls + d
                        for i, d in enumerate(digits):
                            cls[j, pc + i] = d
                        cb.write(w, temp)
                for _ in range(cpc):
                    if pc >= parts:
                        break
                    for j in range(vecs):
                        if dnd[j]:
                            continue
                        book = r.books[cls[j, pc]][p]
                        if book < 0:
                            continue
                        bk = self.books[book]
                        off = begin + pc * r.partition_size
                        if kind == 0:
                            for k in range(r.partition_size // bk.dims):
                                bk.write(w, entry(book, j, off + k))
                        else:
                            for k in range(0, r.partition_size, bk.dims):
                                bk.write(w, entry(book, j, off + k))
                    pc += 1

    def stream(self, packets, max_segments=255, end_trim=0, start_trim=0):
        """the headers and `packets` laid out in pages; granules as in stream() above"""
        bfs = [self.modes[(p[0] >> 1) & ((1 << V.ilog(len(self.modes) - 1)) - 1)][0] for p in packets]
        ns = [self.blocksize[b] for b in bfs]
        cnt = [0] + [ns[i - 1] // 4 + ns[i] // 4 for i in range(1, len(ns))]
        cum = list(np.cumsum(cnt) - start_trim)
        cum[-1] -= end_trim
        heads = self.headers()
        return (paginate(heads[:1], [0], 255, 0, eos=False) + paginate(heads[1:], [0, 0], 255, 1, bos=False, eos=False) +
                paginate(packets, [int(c) for c in cum], max_segments, 2, bos=False))


def kraft_lengths(rng, n, maxlen=12):
    """lengths of a complete prefix code of n entries (a random full binary tree), in random order"""
    while True:
        leaves = [0]
        while len(leaves) < n:
            leaves.append(leaves.pop(int(rng.integers(0, len(leaves)))) + 1)
            leaves.append(leaves[-1])
        if max(leaves) <= maxlen:
            if n == 1:
                leaves = [1]
            rng.shuffle(leaves)
            return [int(v) for v in leaves]


def random_spec(rng, channels=2, blocksize=(256, 2048), rtype=2, rate=44100, submaps=1, coupling=None, sparse=False):
    """a random but valid setup: scalar books for the floors and classifications, VQ books of lookup types 1 and 2 (one with
    sequence_p), ordered and sparse length lists"""
    books = []

    def add(b):
        books.append(b)
        return len(books) - 1

    ybook = add(Book(sorted(kraft_lengths(rng, 64, 9)), ordered=True))                 # floor Y values 0-63, ordered lengths
    ylens = kraft_lengths(rng, 32, 8)
    if sparse:
        ylens = ylens + [0] * 8
        rng.shuffle(ylens)
    ybook2 = add(Book(ylens))                                                          # sparse (when asked) floor book
    master = add(Book(kraft_lengths(rng, 64, 10)))                                     # 2 subclass bits x 3 posts
    ncls, cpc = 3, 2
    classbook = add(Book(kraft_lengths(rng, ncls ** cpc, 6), dims=cpc))
    vq1 = add(Book(kraft_lengths(rng, 25, 8), dims=2, lookup=1, mult=[0, 1, 2, 3, 4], minv=-2.0, delta=1.0))
    vq2 = add(Book(kraft_lengths(rng, 16, 6), dims=4, lookup=2, mult=[int(v) for v in rng.integers(0, 8, 64)], minv=-0.5,
                   delta=0.25, vbits=3, seq=True))
    vq3 = add(Book(kraft_lengths(rng, 9, 5), dims=1, lookup=1, mult=list(range(9)), minv=-1.0, delta=0.25, seq=True))
    floors = []
    for b in blocksize:
        rb = int(np.log2(b // 2))
        pclass = [0, 1, 0] if b >= 256 else [0, 1]
        classes = [(3, 2, master, [-1, ybook, ybook2, ybook]), (2, 0, -1, [ybook])]
        nposts = sum(classes[c][0] for c in pclass)
        xs = [int(v) for v in rng.choice(np.arange(1, 1 << rb), nposts, replace=False)]
        floors.append(Floor(int(rng.integers(1, 5)), rb, pclass, classes, xs))
    residues = []
    psize = 8
    for b in blocksize:
        size = b // 2 * (channels if rtype == 2 else 1)
        begin = int(rng.integers(0, 3)) * psize
        end = size - int(rng.integers(0, 3)) * psize
        residues.append(Residue(rtype, begin, end, psize, classbook,
                                [[-1] * 8, [vq1, vq3, -1, vq2], [vq2, -1, vq1, -1, -1, -1, -1, vq3]]))
    if coupling is None:
        coupling = [(0, 1)] if channels >= 2 else []
    mappings = []
    for k in range(2):
        mux = [int(c % submaps) for c in range(channels)]
        mappings.append(Mapping(mux, [k] * submaps, [k] * submaps, coupling))
    return Spec(channels, blocksize, books, floors, residues, mappings, [(0, 0), (1, 1)], rate=rate)


def random_packets(spec, rng, n, long_p=0.7):
    """n packets of random block sizes with consistent window flags"""
    bf = [int(rng.random() < long_p) for _ in range(n)]
    out = []
    for i in range(n):
        prev = bf[i - 1] if i else 1
        nxt = bf[i + 1] if i + 1 < n else 1
        out.append(spec.packet(bf[i], prev, nxt, rng=rng))
    return out
