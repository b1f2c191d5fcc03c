"""Test helper: a numpy FLAC reader (RFC 9639), written from the format's field definitions.  It shares nothing with the product's
decoder (flac_core.h) or with tests/flac_writer.py, and musicgan_amd never imports it: it is the independent check of what the GPU
encoder writes.

    r = read(data)                     # -> Stream: STREAMINFO fields, samples (n, channels) int64, one FrameInfo per frame
    r = read(data, expect=pcm)         # the same, checking the stream against `pcm` (fast for long streams, see below)

Every frame's CRC-8 and CRC-16 are checked, and the MD5 of the decoded samples against STREAMINFO's.  All subframe kinds, both Rice
methods, escape partitions, wasted bits and the four stereo assignments are read.  Each frame reports its size in bytes and, per
subframe, its kind, order, wasted bits, Rice method and partition order.

Prediction: FIXED subframes are restored by repeated cumulative sums.  LPC is a recursion; without `expect` it is run sample by
sample.  With `expect` the prediction is formed from the expected samples instead and every restored sample is compared with the
expected one: the decoder's recursion then reproduces `expect` exactly if and only if all of them agree, so the result is the
same while the work is vectorised.  A mismatch raises FlacReadError naming the frame, channel and sample.
"""
from __future__ import annotations

import dataclasses
import hashlib
from typing import List, Optional

import numpy as np


class FlacReadError(AssertionError):
    pass


@dataclasses.dataclass
class SubInfo:
    kind: str          # constant | verbatim | fixed | lpc
    order: int
    wasted: int
    method: Optional[int]   # Rice method (0: 4-bit parameters, 1: 5-bit); None without a residual
    porder: Optional[int]
    escapes: int = 0


@dataclasses.dataclass
class FrameInfo:
    offset: int        # byte offset of the header in the file
    size: int          # bytes, CRC-16 included
    block: int
    assign: str        # independent | left_side | side_right | mid_side
    subs: List[SubInfo]


@dataclasses.dataclass
class Stream:
    rate: int
    channels: int
    bits: int
    total: int
    min_block: int
    max_block: int
    min_frame: int
    max_frame: int
    md5: bytes
    samples: np.ndarray
    frames: List[FrameInfo]


def _crc8(b: bytes) -> int:
    c = 0
    for x in b:
        c ^= x
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _i in range(256):
    _c = _i << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) & 0xFFFF if _c & 0x8000 else (_c << 1) & 0xFFFF
    _CRC16.append(_c)


def _crc16(b: bytes) -> int:
    c = 0
    t = _CRC16
    for x in b:
        c = ((c << 8) & 0xFFFF) ^ t[(c >> 8) ^ x]
    return c


class _Bits:
    """MSB-first reader over bytes, with a table of the next 1 bit for unary runs"""

    def __init__(self, buf: bytes, pos_bits: int):
        self.buf = buf + bytes(8)
        self.pos = pos_bits
        bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8))
        n = len(bits)
        idx = np.full(n + 1, n, dtype=np.int64)
        ones = np.flatnonzero(bits)
        idx[ones] = ones
        self.next_one = np.minimum.accumulate(idx[::-1])[::-1].tolist()
        self.nbits = n

    def get(self, n: int) -> int:
        if n == 0:
            return 0
        p = self.pos
        if p + n > self.nbits:
            raise FlacReadError("read past the end of the stream")
        b0 = p >> 3
        nb = ((p & 7) + n + 7) >> 3
        v = int.from_bytes(self.buf[b0:b0 + nb], "big")
        self.pos = p + n
        return (v >> (8 * nb - (p & 7) - n)) & ((1 << n) - 1)

    def signed(self, n: int) -> int:
        v = self.get(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self) -> int:
        s = self.next_one[min(self.pos, self.nbits)]
        if s >= self.nbits:
            raise FlacReadError("unary run past the end of the stream")
        q = s - self.pos
        self.pos = s + 1
        return q

    def rice(self, count: int, k: int) -> List[int]:
        """`count` Rice codes of parameter k (unfolded to signed)"""
        out = [0] * count
        nxt, buf, p = self.next_one, self.buf, self.pos
        mask = (1 << k) - 1
        for j in range(count):
            s = nxt[p] if p < self.nbits else self.nbits
            if s >= self.nbits:
                raise FlacReadError("Rice code past the end of the stream")
            q = s - p
            p = s + 1
            if k:
                b0 = p >> 3
                r = (int.from_bytes(buf[b0:b0 + 5], "big") >> (40 - (p & 7) - k)) & mask
                p += k
                u = (q << k) | r
            else:
                u = q
            out[j] = (u >> 1) ^ -(u & 1)
        if p > self.nbits:
            raise FlacReadError("Rice code past the end of the stream")
        self.pos = p
        return out


_RATES = [0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000]
_SIZES = [0, 8, 12, 0, 16, 20, 24, 32]
_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _utf8_number(br: _Bits) -> int:
    b0 = br.get(8)
    if b0 < 0x80:
        return b0
    n = 0
    while b0 & (0x80 >> n):
        n += 1
    if n < 2 or n > 7:
        raise FlacReadError("invalid coded number")
    v = b0 & (0x7F >> n)
    for _ in range(n - 1):
        b = br.get(8)
        if b >> 6 != 2:
            raise FlacReadError("invalid coded number continuation")
        v = (v << 6) | (b & 0x3F)
    return v


def _predict(x: np.ndarray, coefs, shift: int, start: int) -> np.ndarray:
    """prediction of x[start:] from the samples before each one (exact, int64 then >> shift)"""
    n = len(x)
    p = np.zeros(n - start, dtype=np.int64)
    for j, c in enumerate(coefs):
        p += int(c) * x[start - 1 - j:n - 1 - j]
    return p >> shift


def _subframe(br: _Bits, bs: int, sbps: int, expect: Optional[np.ndarray], where: str):
    if br.get(1):
        raise FlacReadError(f"{where}: subframe padding bit set")
    t = br.get(6)
    wasted = 0
    if br.get(1):
        wasted = 1 + br.unary()
    b = sbps - wasted
    if b < 1:
        raise FlacReadError(f"{where}: {wasted} wasted bits of {sbps}")
    exp = None if expect is None else expect >> wasted
    if expect is not None and np.any((exp << wasted) != expect):
        raise FlacReadError(f"{where}: {wasted} wasted bits, but the expected samples have fewer zero low bits")
    if t == 0:
        x = np.full(bs, br.signed(b), dtype=np.int64)
        return x << wasted, SubInfo("constant", 0, wasted, None, None)
    if t == 1:
        x = np.array([br.signed(b) for _ in range(bs)], dtype=np.int64)
        return x << wasted, SubInfo("verbatim", 0, wasted, None, None)
    if 8 <= t <= 12:
        kind, order = "fixed", t - 8
    elif t >= 32:
        kind, order = "lpc", t - 31
    else:
        raise FlacReadError(f"{where}: reserved subframe type {t}")
    if order > bs:
        raise FlacReadError(f"{where}: order {order} above the block size {bs}")
    warm = [br.signed(b) for _ in range(order)]
    if kind == "lpc":
        prec = br.get(4) + 1
        if prec == 16:
            raise FlacReadError(f"{where}: invalid coefficient precision")
        shift = br.signed(5)
        if shift < 0:
            raise FlacReadError(f"{where}: negative shift")
        coefs = [br.signed(prec) for _ in range(order)]
    else:
        coefs, shift = _FIXED[order], 0
    method = br.get(2)
    if method > 1:
        raise FlacReadError(f"{where}: reserved residual method {method}")
    porder = br.get(4)
    pn = bs >> porder
    if pn << porder != bs or pn < order:
        raise FlacReadError(f"{where}: partition order {porder} does not fit block {bs} / order {order}")
    pbits, esc = (5, 31) if method else (4, 15)
    res: List[int] = []
    escapes = 0
    for p in range(1 << porder):
        cnt = pn - order if p == 0 else pn
        k = br.get(pbits)
        if k == esc:
            escapes += 1
            w = br.get(5)
            res.extend(br.signed(w) if w else 0 for _ in range(cnt))
        else:
            res.extend(br.rice(cnt, k))
    r = np.array(res, dtype=np.int64)
    if np.any(r >= (1 << 31)) or np.any(r < -(1 << 31)):
        raise FlacReadError(f"{where}: residual outside 32 bits")
    info = SubInfo(kind, order, wasted, method, porder, escapes)
    x = np.zeros(bs, dtype=np.int64)
    x[:order] = warm
    if exp is not None:
        if np.any(x[:order] != exp[:order]):
            i = int(np.flatnonzero(x[:order] != exp[:order])[0])
            raise FlacReadError(f"{where}: warm-up sample {i} is {x[i]}, expected {exp[i]}")
        got = r + _predict(exp, coefs, shift, order)
        bad = np.flatnonzero(got != exp[order:])
        if len(bad):
            i = order + int(bad[0])
            raise FlacReadError(f"{where}: sample {i} decodes to {got[bad[0]]}, expected {exp[i]}")
        return exp << wasted, info
    if kind == "fixed":
        if order == 0:
            x = r.copy()
        else:
            # the order-th difference of x is r: integrate order times from the warm-up samples' differences
            d = [np.array(warm, dtype=np.int64)]
            for _ in range(order - 1):
                d.append(np.diff(d[-1]))
            y = r
            for m in range(order - 1, -1, -1):  # d[m][-1] is the last warm-up value of the m-th difference
                y = int(d[m][-1]) + np.cumsum(y)
            x[order:] = y
    else:
        xl = x.tolist()
        cl = [int(c) for c in coefs]
        rl = r.tolist()
        for i in range(order, bs):
            acc = 0
            for j, c in enumerate(cl):
                acc += c * xl[i - 1 - j]
            xl[i] = rl[i - order] + (acc >> shift)
        x = np.array(xl, dtype=np.int64)
    return x << wasted, info


def _frame(data: bytes, pos: int, bound: int, fi: int, at: int, total: int, rate: int, bits: int, ch: int,
           expect: Optional[np.ndarray]):
    """one frame at byte `pos`, reading at most `bound` bytes: (samples, FrameInfo)"""
    br = _Bits(data[pos:pos + bound], 0)
    where = f"frame {fi} at byte {pos}"
    if br.get(15) != 0x7FFC:
        raise FlacReadError(f"{where}: no sync code")
    blocking = br.get(1)
    bcode, rcode, acode, scode = br.get(4), br.get(4), br.get(4), br.get(3)
    if br.get(1):
        raise FlacReadError(f"{where}: reserved header bit set")
    num = _utf8_number(br)
    if bcode == 0:
        raise FlacReadError(f"{where}: reserved block size code")
    bs = 192 if bcode == 1 else 576 << (bcode - 2) if bcode <= 5 else None
    if bcode == 6:
        bs = br.get(8) + 1
    elif bcode == 7:
        bs = br.get(16) + 1
    elif bcode >= 8:
        bs = 256 << (bcode - 8)
    if rcode < 12:
        frate = _RATES[rcode] or rate
    elif rcode == 12:
        frate = br.get(8) * 1000
    elif rcode == 13:
        frate = br.get(16)
    elif rcode == 14:
        frate = br.get(16) * 10
    else:
        raise FlacReadError(f"{where}: invalid rate code")
    fbits = _SIZES[scode] or bits if scode not in (3,) else None
    hlen = br.pos // 8
    if _crc8(data[pos:pos + hlen]) != br.get(8):
        raise FlacReadError(f"{where}: CRC-8 mismatch")
    if frate != rate or fbits != bits or (acode < 8 and acode + 1 != ch) or (acode >= 8 and ch != 2) or acode > 10:
        raise FlacReadError(f"{where}: header disagrees with STREAMINFO")
    if (blocking and num != at) or (not blocking and num != fi):
        raise FlacReadError(f"{where}: coded number {num}")
    if at + bs > total:
        raise FlacReadError(f"{where}: more samples than STREAMINFO's {total}")
    assign = {8: "left_side", 9: "side_right", 10: "mid_side"}.get(acode, "independent")
    side = {8: 1, 9: 0, 10: 1}.get(acode, -1)
    exp = None
    if expect is not None:
        e = expect[at:at + bs]
        if acode == 8:
            exp = [e[:, 0], e[:, 0] - e[:, 1]]
        elif acode == 9:
            exp = [e[:, 0] - e[:, 1], e[:, 1]]
        elif acode == 10:
            exp = [(e[:, 0] + e[:, 1]) >> 1, e[:, 0] - e[:, 1]]
        else:
            exp = [e[:, c] for c in range(ch)]
    chans, subs = [], []
    for c in range(ch):
        x, info = _subframe(br, bs, bits + (c == side), None if exp is None else exp[c], f"{where}, channel {c}")
        chans.append(x)
        subs.append(info)
    if acode == 8:
        chans[1] = chans[0] - chans[1]
    elif acode == 9:
        chans[0] = chans[0] + chans[1]
    elif acode == 10:
        m, s = chans
        m = (m << 1) | (s & 1)
        chans = [(m + s) >> 1, (m - s) >> 1]
    end = (br.pos + 7) // 8
    if br.pos % 8 and br.get(8 - br.pos % 8):
        raise FlacReadError(f"{where}: non-zero padding")
    size = end + 2
    if _crc16(data[pos:pos + end]) != int.from_bytes(data[pos + end:pos + end + 2], "big"):
        raise FlacReadError(f"{where}: CRC-16 mismatch")
    return np.stack(chans, axis=1), FrameInfo(pos, size, bs, assign, subs)


def read(data: bytes, expect: Optional[np.ndarray] = None, check_md5: bool = True) -> Stream:
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacReadError("no fLaC marker")
    pos = 4
    si = None
    while True:
        last, kind, length = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + length]
        if kind == 0:
            si = body
        pos += 4 + length
        if last:
            break
    if si is None or len(si) != 34:
        raise FlacReadError("no STREAMINFO")
    v = int.from_bytes(si[:18], "big")
    total = v & ((1 << 36) - 1)
    bits = ((v >> 36) & 31) + 1
    ch = ((v >> 41) & 7) + 1
    rate = (v >> 44) & ((1 << 20) - 1)
    max_frame = (v >> 64) & ((1 << 24) - 1)
    min_frame = (v >> 88) & ((1 << 24) - 1)
    max_block = (v >> 112) & 0xFFFF
    min_block = v >> 128
    md5 = si[18:34]
    if expect is not None:
        expect = np.asarray(expect, dtype=np.int64).reshape(total, ch)
    out = np.zeros((total, ch), dtype=np.int64)
    frames: List[FrameInfo] = []
    at = 0
    while pos < len(data):
        if at >= total:
            raise FlacReadError(f"bytes after the last frame at {pos}")
        fi = len(frames)
        # a frame of this encoder is no larger than its verbatim coding: parse within a slice of that size first
        bound = 19 + (ch * (8 + max(max_block, 1) * (bits + 1)) + 7) // 8
        try:
            x, info = _frame(data, pos, bound, fi, at, total, rate, bits, ch, expect)
        except FlacReadError as e:
            if "past the end" not in str(e):
                raise
            x, info = _frame(data, pos, len(data) - pos, fi, at, total, rate, bits, ch, expect)
        out[at:at + info.block] = x
        frames.append(info)
        at += info.block
        pos += info.size
    if at != total:
        raise FlacReadError(f"{at} samples decoded, STREAMINFO says {total}")
    if expect is not None and not np.array_equal(out, expect):
        i = int(np.flatnonzero(np.any(out != expect, axis=1))[0])
        raise FlacReadError(f"sample {i} decodes to {out[i].tolist()}, expected {expect[i].tolist()}")
    if check_md5 and md5 != bytes(16):
        nb = (bits + 7) // 8
        raw = out.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()
        if hashlib.md5(raw).digest() != md5:
            raise FlacReadError("MD5 of the decoded samples does not match STREAMINFO")
    return Stream(rate, ch, bits, total, min_block, max_block, min_frame, max_frame, md5, out, frames)
