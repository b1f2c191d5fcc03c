"""FLAC container metadata (RFC 9639), host only: the STREAMINFO fields and where the audio frames start.

The frames themselves are decoded on the GPU (ops.flac_decode, csrc/flac.hip); this module reads the few hundred bytes in front
of them.  Every failure raises FlacError, a ValueError whose message names the file."""
from __future__ import annotations

import dataclasses

BLOCK_TYPES = {0: "STREAMINFO", 1: "PADDING", 2: "APPLICATION", 3: "SEEKTABLE", 4: "VORBIS_COMMENT", 5: "CUESHEET", 6: "PICTURE"}


class FlacError(ValueError):
    pass


@dataclasses.dataclass
class FlacInfo:
    sample_rate: int
    channels: int
    bits: int
    total_samples: int     # 0: not stored (the stream must be decoded to count)
    min_block: int
    max_block: int
    min_frame: int
    max_frame: int
    md5: bytes
    audio_offset: int      # byte offset of the first frame in the file
    audio_end: int         # byte offset after the last frame (a trailing ID3v1 tag excluded)
    blocks: tuple          # metadata block types in file order


def _id3v2_size(head: bytes) -> int:
    """bytes of a leading ID3v2 tag (header, body and footer), 0 when there is none"""
    if len(head) < 10 or head[:3] != b"ID3" or any(b & 0x80 for b in head[6:10]):
        return 0
    size = (head[6] << 21) | (head[7] << 14) | (head[8] << 7) | head[9]
    return 10 + size + (10 if head[5] & 0x10 else 0)


def parse(data: bytes, name: str = "<bytes>") -> FlacInfo:
    """STREAMINFO and the first frame's offset of a whole FLAC file held in memory (only its metadata is read)."""
    pos = _id3v2_size(data[:10])
    if len(data) < pos + 4:
        raise FlacError(f"{name}: not a FLAC stream (the file ends before the 'fLaC' marker: runs past the end)")
    if data[pos:pos + 4] == b"OggS" or data[:4] == b"OggS":
        raise FlacError(f"{name}: FLAC in an Ogg container is not supported (native .flac streams only)")
    if data[pos:pos + 4] != b"fLaC":
        raise FlacError(f"{name}: not a FLAC stream (no 'fLaC' marker)")
    pos += 4
    info, types = None, []
    while True:
        if pos + 4 > len(data):
            raise FlacError(f"{name}: metadata runs past the end of the file")
        last, kind = data[pos] >> 7, data[pos] & 0x7F
        length = int.from_bytes(data[pos + 1:pos + 4], "big")
        body = data[pos + 4:pos + 4 + length]
        if len(body) != length:
            raise FlacError(f"{name}: metadata block {BLOCK_TYPES.get(kind, kind)} runs past the end of the file")
        if kind == 127:
            raise FlacError(f"{name}: invalid metadata block type 127")
        if not types and kind != 0:
            raise FlacError(f"{name}: the first metadata block is not STREAMINFO")
        if kind == 0:
            if types:
                raise FlacError(f"{name}: a second STREAMINFO block")
            if length != 34:
                raise FlacError(f"{name}: STREAMINFO of {length} bytes (34 expected)")
            info = _streaminfo(body, name)
        types.append(kind)
        pos += 4 + length
        if last:
            break
    end = len(data)
    if end - pos >= 128 and data[end - 128:end - 125] == b"TAG":  # ID3v1 tag after the last frame
        end -= 128
    if end <= pos and info.total_samples != 0:
        raise FlacError(f"{name}: no audio frames (truncated file)")
    return dataclasses.replace(info, audio_offset=pos, audio_end=end, blocks=tuple(types))


def _streaminfo(b: bytes, name: str) -> FlacInfo:
    v = int.from_bytes(b[:18], "big")  # 144 bits: 16 16 24 24 20 3 5 36
    total = v & ((1 << 36) - 1)
    v >>= 36
    bits = (v & 31) + 1
    v >>= 5
    channels = (v & 7) + 1
    v >>= 3
    rate = v & ((1 << 20) - 1)
    v >>= 20
    max_frame = v & ((1 << 24) - 1)
    v >>= 24
    min_frame = v & ((1 << 24) - 1)
    v >>= 24
    max_block = v & 0xFFFF
    min_block = v >> 16
    if bits > 24:
        raise FlacError(f"{name}: {bits}-bit FLAC is not supported (4-24 bits)")
    if bits < 4:
        raise FlacError(f"{name}: invalid STREAMINFO bit depth {bits}")
    if rate == 0:
        raise FlacError(f"{name}: STREAMINFO sample rate 0")
    if min_block < 16 or max_block < min_block:
        # min_block < 16 is allowed only for streams of one frame; the decoder takes each frame's size from its header anyway
        if max_block < 1 or max_block < min_block:
            raise FlacError(f"{name}: invalid STREAMINFO block sizes {min_block}..{max_block}")
    return FlacInfo(sample_rate=rate, channels=channels, bits=bits, total_samples=total, min_block=min_block, max_block=max_block,
                    min_frame=min_frame, max_frame=max_frame, md5=bytes(b[18:34]), audio_offset=0, audio_end=0, blocks=())


def read_header(path: str) -> FlacInfo:
    """metadata of the file at `path`; reads the first bytes and grows the read only as far as the metadata goes"""
    try:
        with open(path, "rb") as fh:
            head = fh.read(1 << 16)
            size = fh.seek(0, 2)
            while True:
                try:
                    info = parse(head, path)
                    break
                except FlacError as e:
                    if len(head) >= size or "past the end" not in str(e):
                        raise
                    fh.seek(len(head))
                    head += fh.read(max(len(head), 1 << 16))
            audio_end = size
            if size - info.audio_offset >= 128:
                fh.seek(size - 128)
                if fh.read(3) == b"TAG":
                    audio_end = size - 128
            return dataclasses.replace(info, audio_end=audio_end)
    except OSError as e:
        raise FlacError(f"{path}: cannot read the flac file ({e.strerror or e})") from e
