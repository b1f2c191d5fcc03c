"""CPU: the test-side FLAC reader (tests/flac_reader.py) against tests/flac_writer.py over every coding knob, the argument checks of
FLAC writing (wavio.save to a .flac path, ops.flac_encode) that need no GPU, the encoder's host size queries, its scratch-free
kernels, and `generate --format`."""
import os

import numpy as np
import pytest
import torch

import flac_reader as R
import flac_writer as W
from test_flac_cpu import _music
from test_flac_gpu import _random_frames, _signal


@pytest.mark.parametrize("seed", range(6))
def test_reader_decodes_the_writer_exactly(seed):
    """channels 1-8, depths 4-24, block sizes 1-8192, every subframe kind, FIXED 0-4 / LPC 1-32, wasted bits, Rice and Rice2,
    escape partitions, all four stereo assignments, rate / depth codes or STREAMINFO; read step by step and against `expect`"""
    rng = np.random.default_rng(100 + seed)
    ch = int(rng.choice([1, 2, 2, 3, 8]))
    bits = int(rng.choice([4, 8, 12, 16, 20, 24]))
    n = int(rng.integers(1, 20000))
    rate = int(rng.choice([44100, 48000, 96000, 12345, 192000, 8000]))
    pcm = _signal(rng, n, ch, bits, wasted=int(rng.integers(0, 3)) if bits > 8 else 0)
    frames = _random_frames(rng, pcm, rate)
    raw = []
    data = W.encode(pcm, rate, bits, frames, frame_bytes_out=raw)
    got = R.read(data)
    assert np.array_equal(got.samples, pcm)
    assert (got.rate, got.channels, got.bits, got.total) == (rate, ch, bits, n)
    assert [f.size for f in got.frames] == [len(r) for r in raw]
    assert [f.block for f in got.frames] == [f.size for f in frames]
    for fr, spec in zip(got.frames, frames):
        assert fr.assign == spec.assign
        for s, ss in zip(fr.subs, spec.subs):
            assert s.kind == ss.kind and (s.kind in ("constant", "verbatim") or (s.order, s.method, s.porder) == (ss.order, ss.method, ss.porder))
            if s.kind not in ("constant", "verbatim"):
                assert s.escapes == len(ss.escape or {})
    assert np.array_equal(R.read(data, expect=pcm).samples, pcm)


def test_reader_catches_a_wrong_sample_a_flipped_bit_and_a_wrong_md5():
    pcm = _music(9000, 2, 16)
    sub = W.SubSpec(kind="lpc", order=8, porder=2)
    data = W.encode(pcm, 44100, 16, W.plain_frames(9000, 4096, assign="mid_side", subs=[sub, sub]))
    bad = pcm.copy()
    bad[5000, 1] += 1
    with pytest.raises(R.FlacReadError, match="frame 1"):
        R.read(data, expect=bad)
    flipped = bytearray(data)
    flipped[len(data) // 2] ^= 4
    with pytest.raises(R.FlacReadError):
        R.read(bytes(flipped))
    md5 = bytearray(data)
    md5[30] ^= 1  # inside STREAMINFO's MD5
    with pytest.raises(R.FlacReadError, match="MD5"):
        R.read(bytes(md5))


@pytest.mark.parametrize("what, kw, match", [
    ("bits 20", dict(bits_per_sample=20), "16 or 24"),
    ("int32", dict(dtype=torch.int32), "int16"),
    ("0 channels", dict(channels=0), "1 to 8 channels"),
    ("9 channels", dict(channels=9), "1 to 8 channels"),
    ("rate 0", dict(rate=0), "sample rate"),
    ("rate 2^20", dict(rate=1 << 20), "sample rate"),
    ("int16 at 24 bits", dict(dtype=torch.int16, bits_per_sample=24), "16 bits"),
])
def test_flac_arguments_are_checked_before_anything_else(tmp_path, monkeypatch, what, kw, match):
    from musicgan_amd import ops
    from musicgan_amd.audio import wavio
    x = torch.zeros(kw.get("channels", 2), 100, dtype=kw.get("dtype", torch.float32))
    for gpu in (False, True):
        monkeypatch.setattr(torch.cuda, "is_available", lambda: gpu)
        path = tmp_path / "a.FLAC"
        with pytest.raises(ValueError, match=match):
            wavio.save(str(path), x, kw.get("rate", 44100), kw.get("bits_per_sample"))
        assert not path.exists()
        with pytest.raises(ValueError, match=match):
            ops.flac_encode(x, kw.get("rate", 44100), kw.get("bits_per_sample"))


def test_flac_without_a_gpu_raises_musicganhiperror_naming_the_path(tmp_path, monkeypatch):
    from musicgan_amd import _lib
    from musicgan_amd.audio import wavio
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    path = tmp_path / "out.flac"
    with pytest.raises(_lib.MusicGanHipError, match="out.flac.*GPU"):
        wavio.save(str(path), torch.zeros(2, 1000), 44100, 16)
    assert not path.exists()


def test_wav_output_is_unchanged_and_refuses_bits_per_sample(tmp_path):
    from scipy.io import wavfile
    from musicgan_amd.audio import wavio
    x = torch.rand(2, 3001) - 0.5
    wavio.save(str(tmp_path / "a.wav"), x, 22050)
    wavfile.write(str(tmp_path / "b.wav"), 22050, np.ascontiguousarray(x.numpy().T))
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    with pytest.raises(ValueError, match="only accepted for .flac"):
        wavio.save(str(tmp_path / "c.wav"), x, 22050, 16)
    assert not (tmp_path / "c.wav").exists()


def test_encoder_size_queries_are_host_callable():
    from musicgan_amd import _lib
    lib = _lib.load()
    for n, ch, bits in ((1, 1, 16), (4096, 2, 16), (4097, 8, 24), (44100 * 600, 2, 16)):
        nframes = (n + 4095) // 4096
        pcm = n * ch * bits // 8
        assert lib.mg_flac_enc_max_bytes(n, ch, bits) >= 42 + pcm + nframes * (16 + ch + 2)
        assert lib.mg_flac_enc_ws_bytes(n, ch) >= nframes * 8
    assert lib.mg_flac_enc_max_bytes(100, 2, 20) == 0 and lib.mg_flac_enc_max_bytes(100, 9, 16) == 0
    assert lib.mg_flac_enc_ws_bytes(0, 2) == 0


def test_flac_encoder_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_usage().items() if "flac_enc" in k}
    assert len(hits) >= 8, sorted(hits)
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)


def test_generate_format_flag():
    from musicgan_amd.__main__ import build_parser
    p = build_parser()
    a = p.parse_args(["generate", "gen.pt", "32", "-o", "o", "--format", "flac"])
    assert a.audio_format == "flac"
    assert p.parse_args(["generate", "gen.pt", "32", "-o", "o"]).audio_format == "wav"
    with pytest.raises(SystemExit):
        p.parse_args(["generate", "gen.pt", "32", "-o", "o", "--format", "mp3"])


def test_generate_refuses_an_unknown_format(tmp_path):
    import musicgan_amd  # (the package's re-exported function: importing the sub-module would rebind the name)
    with pytest.raises(ValueError, match="wav' or 'flac"):
        musicgan_amd.generate(str(tmp_path / "g"), 8, "missing.pt", 1, 1, audio_format="mp3")
    assert not os.path.exists(tmp_path / "g")
