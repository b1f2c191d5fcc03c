"""Test helper: a numpy FLAC writer (RFC 9639) in which every coding choice is an explicit knob, per frame and per subframe.

Written from the format's field definitions and sharing nothing with the product's decoder (musicgan_amd never imports it).
A frame is a list of (value, bit count) fields, packed MSB first; the CRC-8 / CRC-16 are computed here from their polynomials.

    data = encode(pcm, sample_rate, bits, frames=[FrameSpec(...), ...])      # -> bytes of a .flac file

`pcm`: int array (samples, channels) of values in the signed `bits`-bit range.  A FrameSpec says how many samples the frame holds
and how it is coded; subframe knobs are SubSpec's (one per channel of the frame's channel assignment).  `plain_frames` builds the
specs of a stream of equal blocks with one coding.
"""
from __future__ import annotations

import dataclasses
import hashlib
import struct
from typing import List, Optional, Sequence

import numpy as np

RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
SIZE_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6, 32: 7}
ASSIGN = {"independent": None, "left_side": 8, "side_right": 9, "mid_side": 10}


@dataclasses.dataclass
class SubSpec:
    kind: str = "lpc"             # constant | verbatim | fixed | lpc
    order: int = 8                # fixed: 0-4, lpc: 1-32
    precision: int = 12           # lpc coefficient bits (1-15)
    shift: Optional[int] = None   # lpc shift (0-15); None: the largest the precision allows
    coefs: Optional[Sequence[int]] = None  # lpc quantised coefficients (first: most recent sample); None: least squares
    wasted: Optional[int] = None  # wasted bits; None: as many as the samples allow (0 for constant)
    method: int = 0               # 0: Rice (4-bit parameters), 1: Rice2 (5-bit)
    porder: int = 0               # partition order
    params: Optional[Sequence[int]] = None  # Rice parameter per partition; None: the cheapest
    escape: Optional[dict] = None  # {partition index: raw width} coded as escape partitions (width None: the smallest that fits)


@dataclasses.dataclass
class FrameSpec:
    size: int
    assign: str = "independent"   # channel assignment for 2 channels
    subs: Optional[List[SubSpec]] = None  # one per channel; None: SubSpec() each
    bs_code: str = "auto"         # auto | 8bit | 16bit
    rate_code: str = "auto"       # auto | streaminfo | khz | hz | 10hz
    bps_code: str = "auto"        # auto | streaminfo


class Bits:
    def __init__(self):
        self.vals: List[np.ndarray] = []
        self.lens: List[np.ndarray] = []

    def put(self, value: int, n: int) -> None:
        if n == 0:
            return
        assert 0 < n <= 64
        self.vals.append(np.array([value & ((1 << n) - 1)], dtype=np.uint64))
        self.lens.append(np.array([n], dtype=np.int64))

    def put_signed(self, value: int, n: int) -> None:
        assert -(1 << (n - 1)) <= value < (1 << (n - 1)) if n else value == 0, (value, n)
        self.put(int(value) & ((1 << n) - 1) if n else 0, n)

    def put_many(self, vals: np.ndarray, lens: np.ndarray) -> None:
        self.vals.append(np.asarray(vals, dtype=np.uint64))
        self.lens.append(np.asarray(lens, dtype=np.int64))

    def nbits(self) -> int:
        return int(sum(int(x.sum()) for x in self.lens))

    def tobytes(self) -> bytes:
        """pack MSB first, zero padded to a whole byte"""
        vals, lens = np.concatenate(self.vals), np.concatenate(self.lens)
        keep = lens > 0
        vals, lens = vals[keep], lens[keep]
        starts = np.cumsum(lens) - lens
        total = int(lens.sum())
        idx = np.repeat(np.arange(len(lens)), lens)
        pos = np.arange(total) - np.repeat(starts, lens)
        sh = (lens[idx] - 1 - pos).astype(np.uint64)
        bits = ((vals[idx] >> sh) & np.uint64(1)).astype(np.uint8)
        return np.packbits(bits).tobytes()


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_T16 = []
for _i in range(256):
    _t = _i << 8
    for _ in range(8):
        _t = ((_t << 1) ^ 0x8005) & 0xFFFF if _t & 0x8000 else (_t << 1) & 0xFFFF
    _T16.append(_t)
_T16 = np.array(_T16, dtype=np.int64)


def crc16_many(frames: Sequence[bytes]) -> List[int]:
    """CRC-16 (poly 0x8005, init 0) of several byte strings at once: each is left-padded with zero bytes to the longest (which a
    CRC with init 0 does not see) and all are run column by column."""
    if not frames:
        return []
    m = max(len(f) for f in frames)
    a = np.zeros((len(frames), m), dtype=np.int64)
    for i, f in enumerate(frames):
        if len(f):
            a[i, m - len(f):] = np.frombuffer(f, dtype=np.uint8)
    c = np.zeros(len(frames), dtype=np.int64)
    for j in range(m):
        c = ((c << 8) & 0xFFFF) ^ _T16[((c >> 8) ^ a[:, j]) & 0xFF]
    return [int(x) for x in c]


def coded_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for n, cap in ((2, 11), (3, 16), (4, 21), (5, 26), (6, 31), (7, 36)):
        if v < (1 << cap):
            out = []
            for _ in range(n - 1):
                out.append(0x80 | (v & 0x3F))
                v >>= 6
            lead = (0xFF << (8 - n)) & 0xFF
            return bytes([lead | v] + out[::-1])
    raise ValueError("number too large")


def zigzag(r: np.ndarray) -> np.ndarray:
    r = r.astype(np.int64)
    return np.where(r >= 0, 2 * r, -2 * r - 1).astype(np.uint64)


def put_residual(w: Bits, res: np.ndarray, bs: int, order: int, sub: SubSpec) -> None:
    w.put(sub.method, 2)
    w.put(sub.porder, 4)
    nparts = 1 << sub.porder
    pn = bs >> sub.porder
    assert pn << sub.porder == bs and pn >= order, (bs, sub.porder, order)
    esc_code = 31 if sub.method else 15
    kmax = esc_code - 1
    at = 0
    for p in range(nparts):
        cnt = pn - order if p == 0 else pn
        part = res[at:at + cnt].astype(np.int64)
        at += cnt
        if sub.escape is not None and p in sub.escape:
            width = sub.escape[p]
            if width is None:  # the smallest signed width that holds every value (0 for an all-zero partition)
                width = 0 if not np.any(part) else int(max(int(part.max()), -int(part.min()) - 1)).bit_length() + 1
            w.put(esc_code, 5 if sub.method else 4)
            w.put(width, 5)
            if width:
                w.put_many(part.astype(np.int64) & ((1 << width) - 1), np.full(cnt, width))
            else:
                assert not np.any(part)
            continue
        u = zigzag(part)
        if sub.params is not None:
            k = int(sub.params[p])
        else:
            costs = [int((u >> np.uint64(k)).sum()) + cnt * (k + 1) for k in range(kmax + 1)]
            k = int(np.argmin(costs))
        assert 0 <= k <= kmax
        w.put(k, 5 if sub.method else 4)
        q = (u >> np.uint64(k)).astype(np.int64)
        low = u & np.uint64((1 << k) - 1)
        val = (np.uint64(1) << np.uint64(k)) | low
        long_run = q + 1 + k > 64
        if not long_run.any():
            w.put_many(val, q + 1 + k)
        else:  # unary runs longer than a field: the zeros in pieces of 32 bits
            for i in range(cnt):
                qi = int(q[i])
                while qi + 1 + k > 64:
                    w.put(0, 32)
                    qi -= 32
                w.put(int(val[i]), qi + 1 + k)


def lpc_coefs(x: np.ndarray, order: int, precision: int, shift: Optional[int]):
    """least-squares predictor of x, quantised to `precision` bits"""
    xf = x.astype(np.float64)
    n = len(xf)
    if n <= order:
        a = np.zeros(order)
    else:
        A = np.stack([xf[order - 1 - j:n - 1 - j] for j in range(order)], axis=1)
        a = np.linalg.lstsq(A, xf[order:], rcond=None)[0]
    cmax = float(np.max(np.abs(a))) if order else 0.0
    lim = (1 << (precision - 1)) - 1
    if shift is None:
        shift = 15
        while shift > 0 and cmax * (1 << shift) > lim:
            shift -= 1
    q = np.clip(np.round(a * (1 << shift)), -lim - 1, lim).astype(np.int64)
    return [int(c) for c in q], shift


def lpc_residual(x: np.ndarray, coefs: Sequence[int], shift: int) -> np.ndarray:
    x = x.astype(np.int64)
    order = len(coefs)
    n = len(x)
    pred = np.zeros(n - order, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * x[order - 1 - j:n - 1 - j]
    return x[order:] - (pred >> shift)


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def put_subframe(w: Bits, x: np.ndarray, sbps: int, sub: SubSpec) -> None:
    x = x.astype(np.int64)
    bs = len(x)
    if sub.wasted is None:
        if sub.kind == "constant" or not np.any(x):
            wasted = 0
        else:
            nz = x[x != 0]
            wasted = int(min(int(np.min((nz & -nz))).bit_length() - 1, sbps - 1))
    else:
        wasted = sub.wasted
    assert not np.any(x & ((1 << wasted) - 1)), "samples not divisible by the wasted bits"
    x = x >> wasted
    b = sbps - wasted
    kind = sub.kind
    if kind == "constant":
        assert np.all(x == x[0])
        t = 0
    elif kind == "verbatim":
        t = 1
    elif kind == "fixed":
        assert 0 <= sub.order <= 4
        t = 8 + sub.order
    else:
        assert 1 <= sub.order <= 32
        t = 32 + sub.order - 1
    w.put(0, 1)
    w.put(t, 6)
    if wasted:
        w.put(1, 1)
        w.put(1, wasted)  # wasted - 1 zeros, then a 1
    else:
        w.put(0, 1)
    if kind == "constant":
        w.put_signed(int(x[0]), b)
        return
    if kind == "verbatim":
        w.put_many(x & ((1 << b) - 1), np.full(bs, b))
        return
    order = sub.order
    for v in x[:order]:
        w.put_signed(int(v), b)
    if kind == "fixed":
        res = lpc_residual(x, FIXED[order], 0) if order else x.copy()
    else:
        if sub.coefs is not None:
            coefs, shift = [int(c) for c in sub.coefs], int(sub.shift or 0)
        else:
            coefs, shift = lpc_coefs(x, order, sub.precision, sub.shift)
        w.put(sub.precision - 1, 4)
        w.put_signed(shift, 5)
        for c in coefs:
            w.put_signed(c, sub.precision)
        res = lpc_residual(x, coefs, shift)
    assert np.all(np.abs(res) < (1 << 31))
    put_residual(w, res, bs, order, sub)


def encode_frame(x: np.ndarray, number: int, blocking: int, rate: int, bps: int, spec: FrameSpec) -> bytes:
    bs, ch = x.shape
    assert spec.size == bs and 1 <= bs <= 65535
    hdr = Bits()
    hdr.put(0xFFF8 | blocking, 16)  # 15-bit sync code 111111111111100, then the blocking bit
    if spec.bs_code == "8bit":
        bcode, bextra = 6, (bs - 1, 8)
    elif spec.bs_code == "16bit":
        bcode, bextra = 7, (bs - 1, 16)
    elif bs == 192:
        bcode, bextra = 1, None
    elif bs in (576, 1152, 2304, 4608):
        bcode, bextra = 2 + [576, 1152, 2304, 4608].index(bs), None
    elif bs in [256 << k for k in range(8)]:
        bcode, bextra = 8 + [256 << k for k in range(8)].index(bs), None
    else:
        bcode, bextra = (6, (bs - 1, 8)) if bs <= 256 else (7, (bs - 1, 16))
    rextra = None
    if spec.rate_code == "streaminfo":
        rcode = 0
    elif spec.rate_code == "khz":
        rcode, rextra = 12, (rate // 1000, 8)
    elif spec.rate_code == "hz":
        assert rate < 65536, "a 16-bit rate field in Hz"
        rcode, rextra = 13, (rate, 16)
    elif spec.rate_code == "10hz":
        rcode, rextra = 14, (rate // 10, 16)
    elif rate in RATE_CODES:
        rcode = RATE_CODES[rate]
    elif rate % 1000 == 0 and rate // 1000 < 256:
        rcode, rextra = 12, (rate // 1000, 8)
    elif rate < 65536:
        rcode, rextra = 13, (rate, 16)
    else:
        rcode, rextra = 14, (rate // 10, 16)
    if rextra is not None and rcode == 12:
        assert rextra[0] * 1000 == rate
    if rextra is not None and rcode == 14:
        assert rextra[0] * 10 == rate
    hdr.put(bcode, 4)
    hdr.put(rcode, 4)
    assign = ASSIGN[spec.assign]
    if assign is not None:
        assert ch == 2
        hdr.put(assign, 4)
    else:
        hdr.put(ch - 1, 4)
    scode = 0 if spec.bps_code == "streaminfo" else SIZE_CODES.get(bps, 0)
    hdr.put(scode, 3)
    hdr.put(0, 1)
    for b in coded_number(number):
        hdr.put(b, 8)
    if bextra:
        hdr.put(*bextra)
    if rextra:
        hdr.put(*rextra)
    head = hdr.tobytes()
    head += bytes([crc8(head)])
    x = x.astype(np.int64)
    if assign == 8:
        chans, side = [x[:, 0], x[:, 0] - x[:, 1]], 1
    elif assign == 9:
        chans, side = [x[:, 0] - x[:, 1], x[:, 1]], 0
    elif assign == 10:
        chans, side = [(x[:, 0] + x[:, 1]) >> 1, x[:, 0] - x[:, 1]], 1
    else:
        chans, side = [x[:, c] for c in range(ch)], -1
    subs = spec.subs or [SubSpec() for _ in range(ch)]
    assert len(subs) == ch
    body = Bits()
    for c in range(ch):
        put_subframe(body, chans[c], bps + (c == side), subs[c])
    return head + body.tobytes()


def streaminfo(min_bs, max_bs, min_fs, max_fs, rate, ch, bps, total, md5: bytes) -> bytes:
    w = Bits()
    w.put(min_bs, 16)
    w.put(max_bs, 16)
    w.put(min_fs, 24)
    w.put(max_fs, 24)
    w.put(rate, 20)
    w.put(ch - 1, 3)
    w.put(bps - 1, 5)
    w.put(total, 36)
    return w.tobytes() + md5


def pcm_md5(pcm: np.ndarray, bps: int) -> bytes:
    nb = (bps + 7) // 8
    b = pcm.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)[:, :nb]
    return hashlib.md5(b.tobytes()).digest()


def metadata_block(kind: int, payload: bytes, last: bool) -> bytes:
    return bytes([(0x80 if last else 0) | kind]) + len(payload).to_bytes(3, "big") + payload


def id3v2(payload_len: int = 30) -> bytes:
    size = payload_len
    ss = bytes([(size >> 21) & 0x7F, (size >> 14) & 0x7F, (size >> 7) & 0x7F, size & 0x7F])
    return b"ID3" + bytes([4, 0, 0]) + ss + bytes(range(payload_len))


def extra_blocks() -> list:
    """(type, payload) of one block of each other kind: PADDING, APPLICATION, SEEKTABLE, VORBIS_COMMENT, CUESHEET, PICTURE"""
    vc = struct.pack("<I", 6) + b"writer" + struct.pack("<I", 1) + struct.pack("<I", 9) + b"TITLE=abc"
    seek = struct.pack(">QQH", 0, 0, 4096) + struct.pack(">QQH", 0xFFFFFFFFFFFFFFFF, 0, 0)
    cue = bytes(128) + (0).to_bytes(8, "big") + bytes([0x80]) + bytes(258) + bytes([1]) + (0).to_bytes(8, "big") + bytes([170]) \
        + bytes(12) + bytes([0]) + bytes(13) + bytes([0])
    pic = struct.pack(">I", 3) + struct.pack(">I", 9) + b"image/png" + struct.pack(">I", 0) + struct.pack(">IIIII", 1, 1, 24, 0, 4) \
        + b"\x89PNG"
    return [(1, bytes(20)), (2, b"TEST" + b"app-data"), (3, seek), (4, vc), (5, cue), (6, pic)]


def encode(pcm: np.ndarray, rate: int, bps: int, frames: Sequence[FrameSpec], *, blocking: int = 0, total_samples=None,
           id3: bool = False, blocks: Sequence = (), md5: bool = True, frame_bytes_out: Optional[list] = None) -> bytes:
    """the whole file.  `blocking` 1: variable blocking (numbers are first samples).  `total_samples`: None = the true count."""
    pcm = np.asarray(pcm)
    if pcm.ndim == 1:
        pcm = pcm[:, None]
    n, ch = pcm.shape
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    assert pcm.min(initial=0) >= lo and pcm.max(initial=0) <= hi
    assert sum(f.size for f in frames) == n
    raw = []
    at = 0
    for i, f in enumerate(frames):
        raw.append(encode_frame(pcm[at:at + f.size], at if blocking else i, blocking, rate, bps, f))
        at += f.size
    crcs = crc16_many(raw)
    out_frames = [r + c.to_bytes(2, "big") for r, c in zip(raw, crcs)]
    if frame_bytes_out is not None:
        frame_bytes_out.extend(out_frames)
    sizes = [len(f) for f in out_frames]
    bss = [f.size for f in frames]
    si = streaminfo(min(bss) if len(bss) == 1 else min(bss[:-1]), max(bss), min(sizes), max(sizes), rate, ch, bps,
                    n if total_samples is None else total_samples, pcm_md5(pcm, bps) if md5 else bytes(16))
    allb = [(0, si)] + list(blocks)
    meta = b"".join(metadata_block(k, p, i == len(allb) - 1) for i, (k, p) in enumerate(allb))
    return (id3v2() if id3 else b"") + b"fLaC" + meta + b"".join(out_frames)


def plain_frames(n: int, block: int = 4096, **kw) -> List[FrameSpec]:
    sizes = [block] * (n // block) + ([n % block] if n % block else [])
    return [FrameSpec(size=s, **kw) for s in sizes]


def biggest_porder(bs: int, order: int, want: int) -> int:
    p = want
    while p > 0 and ((bs >> p) << p != bs or (bs >> p) < order):
        p -= 1
    return p
