"""Minimal audio file IO (the reference uses torchaudio.load/save, functions.py:43,139; torchaudio is not a dependency here).
load() mirrors torchaudio.load(normalize=True): float32 tensor (channels, samples) in [-1, 1] and the sample rate.
Containers: RIFF WAV (scipy), AIFF / AIFF-C and Sun AU with linear PCM (Python's standard library) -- the uncompressed formats
torchaudio's backends read without a codec -- FLAC, whose frames are decoded on the GPU (ops.flac_decode), and Ogg Vorbis
(.ogg / .oga), whose packets are decoded on the GPU (ops.vorbis_decode) to float32, not clipped, as torchaudio returns it.  There
is no CPU decoder for either: reading them without a GPU raises MusicGanHipError.  mp3, Opus, Ogg FLAC and the rest raise.
save() writes 32-bit float WAV, FLAC for a .flac path (encoded on the GPU, ops.flac_encode) or Ogg Vorbis for a .ogg / .oga
path (encoded on the GPU, ops.vorbis_encode; `compression` is the quality, -1 .. 10, default 3, as torchaudio names it).  There
is no CPU encoder for either: writing them without a GPU raises MusicGanHipError and writes nothing."""
from __future__ import annotations

import os

import numpy as np
import torch
from scipy.io import wavfile

from . import flac, vorbis

OGG_EXTS = (".ogg", ".oga")


def _linear_pcm(raw: bytes, width: int, channels: int, what: str) -> np.ndarray:
    """Big-endian signed linear PCM (AIFF, AU) -> (frames, channels) int16 / int32 with the value torchaudio normalises:
    8-bit v -> v * 2^8 (v / 2^7 == that / 2^15), 24-bit v -> v * 2^8 (v / 2^23 == that / 2^31)."""
    if width == 1:
        x = np.frombuffer(raw, dtype=np.int8).astype(np.int16) * 256
    elif width == 2:
        x = np.frombuffer(raw, dtype=">i2").astype(np.int16)
    elif width == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        x = ((b[:, 0] << 24) | (b[:, 1] << 16) | (b[:, 2] << 8)).astype(np.int32)  # sign bit lands in bit 31
    elif width == 4:
        x = np.frombuffer(raw, dtype=">i4").astype(np.int32)
    else:
        raise ValueError(f"{what}: {8 * width}-bit samples are not supported")
    return np.ascontiguousarray(x.reshape(-1, channels))


def _read_frames(path: str, mmap: bool = False):
    """(frames, channels) array as stored (int16 / int32 / uint8 / float32 / float64) and the sample rate."""
    ext = os.path.splitext(path)[1].lower()
    if ext in (".aif", ".aiff", ".aifc"):
        import aifc
        with aifc.open(path, "rb") as f:
            if f.getcomptype() not in (b"NONE", b"sowt"):
                raise ValueError(f"{path}: compressed AIFF-C ({f.getcomptype().decode()}) is not supported")
            raw, width, ch, sr = f.readframes(f.getnframes()), f.getsampwidth(), f.getnchannels(), f.getframerate()
            if f.getcomptype() == b"sowt":  # little-endian 16-bit variant
                return np.ascontiguousarray(np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, ch)), int(sr)
        return _linear_pcm(raw, width, ch, path), int(sr)
    if ext in (".au", ".snd"):
        import sunau
        with sunau.open(path, "rb") as f:
            if f.getcomptype() != "NONE":
                raise ValueError(f"{path}: {f.getcompname()} AU files are not supported (linear PCM only)")
            raw, width, ch, sr = f.readframes(f.getnframes()), f.getsampwidth(), f.getnchannels(), f.getframerate()
        return _linear_pcm(raw, width, ch, path), int(sr)
    if ext == ".flac":
        return load_pcm_device(path).cpu().numpy(), flac.read_header(path).sample_rate
    if ext in OGG_EXTS:
        pcm = load_pcm_device(path)  # parses the file first: a bad stream raises its ValueError before any GPU check
        return pcm.cpu().numpy(), vorbis.read_header(path).sample_rate
    if ext not in (".wav", ".wave", ""):
        raise ValueError(f"{path}: only WAV, AIFF, AU (linear PCM), FLAC and Ogg Vorbis files can be read here; torchaudio's other "
                         f"codec-backed formats (mp3, opus, ...) need a decoder this build does not ship")
    try:
        sr, data = wavfile.read(path, mmap=mmap)
    except ValueError:  # formats scipy cannot map (e.g. 24-bit)
        sr, data = wavfile.read(path)
    if data.ndim == 1:
        data = data[:, None]
    return data, int(sr)


def load(path: str):
    data, sr = _read_frames(path)
    if data.dtype == np.int16:
        x = data.astype(np.float32) / 32768.0
    elif data.dtype == np.int32:
        x = data.astype(np.float32) / 2147483648.0
    elif data.dtype == np.uint8:
        x = (data.astype(np.float32) - 128.0) / 128.0
    else:
        x = data.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x.T)), int(sr)


def load_pcm(path: str, mmap: bool = True):
    """The file's frames as stored: array (frames, channels) of int16 / int32 / uint8 / float32 (a read-only memory map where the
    format allows) and the sample rate -- what `load` normalises and transposes; the device path does both inside the STFT kernel
    (ops.stft_1024_pcm), so a file's bytes travel to the GPU as they are (int16: half of float32's).
    FLAC: decoded on the GPU and COPIED to host memory (not a memory map): int16 up to 16 bits, int32 above, samples
    left-justified as WAV / AIFF store them (load_pcm_device keeps them on the device).  Ogg Vorbis: decoded on the GPU and copied
    to host memory as float32."""
    data, sr = _read_frames(path, mmap=mmap)
    if data.dtype not in (np.int16, np.int32, np.uint8, np.float32):
        data = np.asarray(data, dtype=np.float32)  # (64-bit float files)
    return data, int(sr)


def save(path: str, wav: torch.Tensor, sample_rate: int, bits_per_sample=None, compression=None) -> None:
    """(channels, samples) float tensor -> 32-bit float WAV (what torchaudio.save writes for float32 input).  A path ending in
    .flac (any case) is written as FLAC instead, as torchaudio picks the container from the extension: float32 / float64 / int16
    samples, 16 or 24 bits (default 24 for floats), encoded on the GPU (ops.flac_encode).  `bits_per_sample` is for .flac only.
    A path ending in .ogg or .oga is written as Ogg Vorbis (ops.vorbis_encode) at quality `compression` (-1 .. 10, default 3),
    which is for those paths only."""
    ext = os.path.splitext(path)[1].lower()
    if compression is not None and ext not in OGG_EXTS:
        raise ValueError(f"{path}: compression is only accepted for .ogg / .oga paths (the Vorbis quality)")
    if ext in OGG_EXTS:
        from .. import ops
        from .._lib import MusicGanHipError
        if bits_per_sample is not None:
            raise ValueError(f"{path}: bits_per_sample is only accepted for .flac paths (Vorbis has no bit depth)")
        try:
            ops.vorbis_encode_args(wav, sample_rate, compression)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
        if not torch.cuda.is_available():
            raise MusicGanHipError(f"{path}: Ogg Vorbis is encoded on the GPU and no ROCm GPU is available (there is no CPU "
                                   f"encoder)")
        data = ops.vorbis_encode(wav.detach(), sample_rate, compression, name=path)
        with open(path, "wb") as fh:
            fh.write(data.numpy().tobytes())
        return
    if ext == ".flac":
        from .. import ops
        from .._lib import MusicGanHipError
        try:
            ops.flac_encode_args(wav, sample_rate, bits_per_sample)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None
        if not torch.cuda.is_available():
            raise MusicGanHipError(f"{path}: FLAC is encoded on the GPU and no ROCm GPU is available (there is no CPU encoder)")
        data = ops.flac_encode(wav.detach(), sample_rate, bits_per_sample, name=path)
        with open(path, "wb") as fh:
            fh.write(data.numpy().tobytes())
        return
    if bits_per_sample is not None:
        raise ValueError(f"{path}: bits_per_sample is only accepted for .flac paths (WAV output is 32-bit float)")
    x = wav.detach().to("cpu", torch.float32).numpy()
    wavfile.write(path, int(sample_rate), np.ascontiguousarray(x.T))


def _flac_region(path: str, device):
    """(padded device buffer holding the audio region, its byte count, FlacInfo); the bytes are uploaded as they are"""
    info = flac.read_header(path)  # a bad or missing file raises flac.FlacError (a ValueError naming the path) before any GPU check
    from .. import ops
    from .._lib import MusicGanHipError
    if not torch.cuda.is_available():
        raise MusicGanHipError(f"{path}: FLAC is decoded on the GPU and no ROCm GPU is available (there is no CPU decoder)")
    n = info.audio_end - info.audio_offset
    host = torch.zeros(ops.flac_padded_bytes(n), dtype=torch.uint8)
    with open(path, "rb") as fh:
        fh.seek(info.audio_offset)
        got = fh.readinto(memoryview(host.numpy())[:n])
    if got != n:
        raise flac.FlacError(f"{path}: short read of the audio frames")
    return host.to(device), n, info


def read_vorbis(path: str):
    """(the file's bytes as a uint8 array, its parsed stream): every header checked on the host, before any GPU check; without a
    GPU a valid stream raises MusicGanHipError"""
    try:
        with open(path, "rb") as fh:
            raw = np.fromfile(fh, dtype=np.uint8)
    except OSError as e:
        raise vorbis.VorbisError(f"{path}: cannot read the ogg file ({e.strerror or e})") from e
    vs = vorbis.parse(raw, path)
    if not torch.cuda.is_available():
        from .._lib import MusicGanHipError
        raise MusicGanHipError(f"{path}: Ogg Vorbis is decoded on the GPU and no ROCm GPU is available (there is no CPU decoder)")
    return raw, vs


def load_pcm_device(path: str, device=None) -> torch.Tensor:
    """The file's PCM frames (frames, channels) on the device, with the dtype and values load_pcm gives: a FLAC file is decoded
    there (ops.flac_decode), any other format is read as stored and uploaded."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
    if os.path.splitext(path)[1].lower() == ".flac":
        buf, n, info = _flac_region(path, device)
        from .. import ops
        return ops.flac_decode(buf, info, nbytes=n, name=path)
    if os.path.splitext(path)[1].lower() in OGG_EXTS:
        raw, vs = read_vorbis(path)
        from .. import ops
        return ops.vorbis_decode(torch.from_numpy(raw).to(device), vs, name=path)
    data, _ = load_pcm(path, mmap=False)
    if device is None:
        from .._lib import MusicGanHipError
        raise MusicGanHipError("load_pcm_device needs a ROCm GPU")
    return torch.from_numpy(np.ascontiguousarray(data)).to(device)


def info(path: str):
    """(frames, channels, sample_rate, bits) from the file's headers alone, for every supported format.  A FLAC stream whose
    STREAMINFO does not give the sample count is decoded to count it (on the GPU)."""
    ext = os.path.splitext(path)[1].lower()
    if ext in OGG_EXTS:
        vi = vorbis.read_header(path)
        return vi.frames, vi.channels, vi.sample_rate, 0  # no stored bit depth
    if ext == ".flac":
        fi = flac.read_header(path)
        frames = fi.total_samples
        if frames == 0 and fi.audio_end > fi.audio_offset:
            frames = load_pcm_device(path).shape[0]
        return int(frames), fi.channels, fi.sample_rate, fi.bits
    if ext in (".aif", ".aiff", ".aifc", ".au", ".snd"):
        import aifc
        import sunau
        mod = sunau if ext in (".au", ".snd") else aifc
        with mod.open(path, "rb") as f:
            return int(f.getnframes()), int(f.getnchannels()), int(f.getframerate()), 8 * int(f.getsampwidth())
    if ext not in (".wav", ".wave", ""):
        _read_frames(path)  # raises the unsupported-format error
    return _wav_info(path)


def _wav_info(path: str):
    """RIFF chunks: fmt (channels, rate, bits per sample) and the size of data"""
    import struct
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] not in (b"RIFF", b"RIFX") or head[8:12] != b"WAVE":
            raise ValueError(f"{path}: not a RIFF WAVE file")
        end = "<" if head[:4] == b"RIFF" else ">"
        fmt = None
        while True:
            ck = fh.read(8)
            if len(ck) < 8:
                raise ValueError(f"{path}: no data chunk")
            cid, size = ck[:4], struct.unpack(end + "I", ck[4:])[0]
            if cid == b"fmt ":
                body = fh.read(size + (size & 1))
                _, ch, sr, _, align, bits = struct.unpack(end + "HHIIHH", body[:16])
                fmt = (ch, sr, bits, align)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError(f"{path}: data chunk before fmt")
                ch, sr, bits, align = fmt
                return int(size // align), int(ch), int(sr), int(bits)
            else:
                fh.seek(size + (size & 1), 1)
