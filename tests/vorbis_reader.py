"""A plain float64 Vorbis I packet decoder in numpy, written straight from the specification (sections 4.3, 7, 8 and 1.3.2),
for the tests to compare ops.vorbis_decode against.  The headers come from musicgan_amd.audio.vorbis (checked on their own in
test_vorbis_cpu.py); everything after them -- codeword reading, floor 1, residues 0/1/2, coupling, the IMDCT (a direct O(n^2)
sum, no FFT), windows, overlap-add and granule trimming -- is independent of the device code.  Slow: meant for short streams."""
from __future__ import annotations

import numpy as np

from musicgan_amd.audio import vorbis as V


class EOP(Exception):
    pass


class Bits:
    def __init__(self, b: bytes):
        self.v = int.from_bytes(b, "little")
        self.n = 8 * len(b)
        self.pos = 0

    def read(self, k: int) -> int:
        if self.pos + k > self.n:
            self.pos = self.n
            raise EOP
        r = (self.v >> self.pos) & ((1 << k) - 1)
        self.pos += k
        return r


def _code_maps(setup):
    maps = []
    for b in setup.books:
        m = {}
        for e, (ln, code) in enumerate(zip(b.lengths, b.codes)):
            if code is not None:
                m[(ln, code)] = e
        maps.append((m, max(b.lengths) if b.lengths else 0))
    return maps


def read_entry(br: Bits, cmap) -> int:
    """bit by bit: the first bit read is the codeword's most significant"""
    m, maxlen = cmap
    code = 0
    for ln in range(1, maxlen + 1):
        code = (code << 1) | br.read(1)
        e = m.get((ln, code))
        if e is not None:
            return e
    raise EOP  # an invalid codeword ends the packet


def _render_line(x0, y0, x1, y1, v):
    dy = y1 - y0
    adx = x1 - x0
    ady = abs(dy)
    base = int(dy / adx)  # truncation toward zero
    sy = base - 1 if dy < 0 else base + 1
    ady -= abs(base) * adx
    y, err = y0, 0
    if x0 < len(v):
        v[x0] = y
    for x in range(x0 + 1, x1):
        err += ady
        if err >= adx:
            err -= adx
            y += sy
        else:
            y += base
        if x < len(v):
            v[x] = y


def floor1_curve(f, Y, n2):
    """steps 1 and 2 of floor 1 (amplitude synthesis, curve) -> integer curve of n2 bins"""
    rng = [256, 128, 86, 64][f.multiplier - 1]
    nx = len(f.X)
    step2 = [True, True] + [False] * (nx - 2)
    final = list(Y[:2]) + [0] * (nx - 2)
    for i in range(2, nx):
        lo, hi = f.low[i], f.high[i]
        x0, y0, x1, y1 = f.X[lo], final[lo], f.X[hi], final[hi]
        dy = y1 - y0
        adx = x1 - x0
        err = abs(dy) * (f.X[i] - x0)
        off = err // adx
        predicted = y0 - off if dy < 0 else y0 + off
        val = Y[i]
        highroom = rng - predicted
        lowroom = predicted
        room = 2 * min(highroom, lowroom)
        if val:
            step2[lo] = step2[hi] = step2[i] = True
            if val >= room:
                final[i] = val - lowroom + predicted if highroom > lowroom else predicted - val + highroom - 1
            else:
                final[i] = predicted - (val + 1) // 2 if val & 1 else predicted + val // 2
        else:
            final[i] = predicted
    curve = np.zeros(n2, dtype=np.int64)
    hx, lx = 0, 0
    clamp = lambda v: min(max(v, 0), 255)  # noqa: E731  (the endpoints are kept inside the dB table)
    ly = clamp(final[f.order[0]] * f.multiplier)
    hy = ly
    for j in f.order[1:]:
        if step2[j]:
            hy = clamp(final[j] * f.multiplier)
            hx = f.X[j]
            _render_line(lx, ly, hx, hy, curve)
            lx, ly = hx, hy
    if hx < n2:
        _render_line(hx, hy, n2, hy, curve)
    return curve


def _decode_floor(br, f, maps):
    if not br.read(1):
        return None
    rng = [256, 128, 86, 64][f.multiplier - 1]
    bits = V.ilog(rng - 1)
    Y = [br.read(bits), br.read(bits)]
    for c in f.partition_class:
        cdim, cbits = f.class_dims[c], f.class_subclasses[c]
        csub = (1 << cbits) - 1
        cval = read_entry(br, maps[f.class_masterbook[c]]) if cbits else 0
        for _ in range(cdim):
            book = f.subclass_books[c][cval & csub]
            cval >>= cbits
            Y.append(read_entry(br, maps[book]) if book >= 0 else 0)
    return Y


def _decode_residue(br, r, setup, maps, vecs, dnd, n2):
    """vecs: list of arrays (one per channel of the submap) decoded in place; dnd: do-not-decode flags"""
    if r.type == 2:
        if all(dnd):
            return
        inter = np.zeros(n2 * len(vecs))
        _residue_core(br, r, setup, maps, [inter], [False], n2 * len(vecs), 1)
        for j, v in enumerate(vecs):
            v[:] = inter[j::len(vecs)]
        return
    _residue_core(br, r, setup, maps, vecs, dnd, n2, r.type)


def _residue_core(br, r, setup, maps, vecs, dnd, size, kind):
    begin, end = min(r.begin, size), min(r.end, size)
    cpc = setup.books[r.classbook].dims
    nread = end - begin
    parts = nread // r.partition_size
    if nread <= 0 or parts == 0:
        return
    cls = np.zeros((len(vecs), parts + cpc), dtype=np.int64)
    try:
        for p in range(8):
            pc = 0
            while pc < parts:
                if p == 0:
                    for j in range(len(vecs)):
                        if dnd[j]:
                            continue
                        temp = read_entry(br, maps[r.classbook])
                        for i in range(cpc - 1, -1, -1):
                            cls[j, i + pc] = temp % r.classifications
                            temp //= r.classifications
                for _ in range(cpc):
                    if pc >= parts:
                        break
                    for j in range(len(vecs)):
                        if dnd[j]:
                            continue
                        book = r.books[cls[j, pc]][p]
                        if book >= 0:
                            _partition(br, setup.books[book], maps[book], vecs[j], begin + pc * r.partition_size,
                                       r.partition_size, kind)
                    pc += 1
    except EOP:
        pass


def _partition(br, book, cmap, v, off, psize, kind):
    if kind == 0:
        step = psize // book.dims
        for j in range(step):
            e = read_entry(br, cmap)
            v[off + j + np.arange(book.dims) * step] += book.values[e]
    else:
        i = 0
        while i < psize:
            e = read_entry(br, cmap)
            for d in range(book.dims):  # a vector may run past the partition (the specification's loop)
                if off + i < len(v):
                    v[off + i] += book.values[e, d]
                i += 1


def imdct(X):
    """the specification's IMDCT: n/2 coefficients -> n samples, y[i] = sum_k X[k] cos(2 pi / n (i + 1/2 + n/4)(k + 1/2))"""
    n = 2 * len(X)
    i = np.arange(n)[:, None]
    k = np.arange(n // 2)[None, :]
    return np.cos(2 * np.pi / n * (i + 0.5 + n / 4) * (k + 0.5)) @ X


def window(n, bs, blockflag, prev, nxt):
    w = np.zeros(n)
    n0 = bs[0]
    if blockflag and not prev:
        ls, le, ln = n // 4 - n0 // 4, n // 4 + n0 // 4, n0 // 2
    else:
        ls, le, ln = 0, n // 2, n // 2
    if blockflag and not nxt:
        rs, re, rn = 3 * n // 4 - n0 // 4, 3 * n // 4 + n0 // 4, n0 // 2
    else:
        rs, re, rn = n // 2, n, n // 2
    x = np.arange(ls, le)
    w[ls:le] = np.sin(np.pi / 2 * np.sin((x - ls + 0.5) / ln * np.pi / 2) ** 2)
    w[le:rs] = 1.0
    x = np.arange(rs, re)
    w[rs:re] = np.sin(np.pi / 2 * np.sin((x - rs + 0.5) / rn * np.pi / 2 + np.pi / 2) ** 2)
    return w


def decode_packet(pkt: bytes, setup, maps, want_spectrum=False):
    """-> (blockflag, prev, next, windowed time signal (n, channels) float64, bits consumed)"""
    br = Bits(pkt)
    ch = setup.channels
    if br.read(1) != 0:
        raise ValueError("not an audio packet")
    mode = br.read(V.ilog(len(setup.modes) - 1))
    bf, mp = setup.modes[mode]
    n = setup.blocksize[bf]
    prev = nxt = 0
    if bf:
        prev, nxt = br.read(1), br.read(1)
    m = setup.mappings[mp]
    n2 = n // 2
    curves = [None] * ch
    try:
        for c in range(ch):
            sub = m.mux[c]
            f = setup.floors[m.submap_floor[sub]]
            try:
                Y = _decode_floor(br, f, maps)
            except EOP:
                Y = None
            curves[c] = None if Y is None else floor1_curve(f, Y, n2)
    except EOP:
        pass
    used = [cv is not None for cv in curves]
    nz = list(used)
    for a, b in zip(m.magnitude, m.angle):
        if nz[a] or nz[b]:
            nz[a] = nz[b] = True
    spec = np.zeros((ch, n2))
    for s in range(len(m.submap_floor)):
        chans = [c for c in range(ch) if m.mux[c] == s]
        vecs = [np.zeros(n2) for _ in chans]
        _decode_residue(br, setup.residues[m.submap_residue[s]], setup, maps, vecs, [not nz[c] for c in chans], n2)
        for c, v in zip(chans, vecs):
            spec[c] = v
    end_bits = br.pos
    for a, b in reversed(list(zip(m.magnitude, m.angle))):
        M, A = spec[a].copy(), spec[b].copy()
        pos_m = M > 0
        pos_a = A > 0
        newM = np.where(pos_m, np.where(pos_a, M, M + A), np.where(pos_a, M, M - A))
        newA = np.where(pos_m, np.where(pos_a, M - A, M), np.where(pos_a, M + A, M))
        spec[a], spec[b] = newM, newA
    db = V.inverse_db_table()
    for c in range(ch):
        spec[c] = spec[c] * db[np.clip(curves[c], 0, 255)] if used[c] else 0.0
    if want_spectrum:
        return bf, prev, nxt, spec, end_bits
    w = window(n, setup.blocksize, bf, prev, nxt)
    out = np.stack([imdct(spec[c]) * w for c in range(ch)], axis=1)
    return bf, prev, nxt, out, end_bits


def decode_file(data: bytes, return_ends: bool = False, setup=None):
    """-> (frames, channels) float64 after granule trimming [, per audio packet (bits consumed, packet bytes)].  `setup`: the
    decode setup to use instead of the parsed one (vorbis_writer.Spec.setup(): codewords, VQ values and floor neighbours built
    by the writer from its own parameters, not by audio/vorbis.py)"""
    vs = V.parse(data, "<reader>")
    setup = setup or vs.setup
    maps = _code_maps(setup)
    blocks, ends = [], []
    for k in range(len(vs.pkt_len)):
        pkt = V.packet_bytes(data, vs, k)
        bf, prev, nxt, out, eb = decode_packet(pkt, setup, maps)
        blocks.append(out)
        ends.append((eb, len(pkt)))
    ch = setup.channels
    pieces = []
    per_packet = []
    for i in range(1, len(blocks)):
        a, b = blocks[i - 1], blocks[i]
        pn, cn = len(a), len(b)
        cnt = pn // 4 + cn // 4
        out = np.zeros((cnt, ch))
        # previous block from its centre on, current block up to its centre; both placed on the shared time axis
        q = np.arange(cnt)
        ip = pn // 2 + q
        ic = q + cn // 4 - pn // 4
        okp = ip < pn
        okc = (ic >= 0) & (ic < cn)
        out[okp] += a[ip[okp]]
        out[okc] += b[ic[okc]]
        pieces.append(out)
        per_packet.append(cnt)
    pcm = np.concatenate(pieces) if pieces else np.zeros((0, ch))
    # trimming from the granule positions (independent of vorbis.parse's arithmetic)
    cum = np.cumsum([0] + per_packet)  # frames returned through packet k: cum[k]
    pages = vs.pages
    first_page = int(vs.pkt_page[0]) if len(vs.pkt_page) else 0
    last_on_first = max(k for k in range(len(vs.pkt_page)) if vs.pkt_page[k] == first_page) if len(vs.pkt_page) else 0
    start = 0
    last = len(pages.offset) - 1
    if len(vs.pkt_page) and first_page != last and pages.granule[first_page] >= 0 and cum[last_on_first] > pages.granule[first_page]:
        start = int(cum[last_on_first] - pages.granule[first_page])
    end = len(pcm)
    if pages.flags[last] & 4 and pages.granule[last] >= 0:
        end = min(end, int(pages.granule[last]) + start)
    pcm = pcm[start:max(end, start)]
    return (pcm, ends) if return_ends else pcm
