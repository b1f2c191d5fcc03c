"""CPU: FLAC container parsing (audio/flac.py), wavio.info for FLAC / WAV / AIFF, the formats that are refused, the fields of the
hand-derived anchor frame, and the scratch-free FLAC kernels.  Streams come from tests/flac_writer.py."""
import hashlib
import os

import numpy as np
import pytest
import torch

import flac_writer as W

# one 16-sample stereo 16-bit mid/side frame with its STREAMINFO, derived from RFC 9639's field definitions (not with libFLAC):
# mid FIXED order 2, Rice, partition order 1 (partition 0: parameter 2, 6 residuals; partition 1: escape of width 7); side LPC
# order 2, precision 5, shift 2, coefficients (7, -3), 1 wasted bit, Rice2 parameter 3.  The MD5 is that of the decoded PCM.
ANCHOR = bytes.fromhex(
    "664c614380000022001000100000000000000ac442f000000010d8a1f69627c7b29aaa10f00a80962f64fff869a8000f78140384045104800140000001c"
    "00000001c000000000038000000000500000000be7c923880ee354b24380320034a08fd4072d41667b848a7db0bf0a84e")
ANCHOR_L = [1000, 1210, 1390, 1502, 1551, 1500, 1380, 1190, 980, 700, 420, 130, -170, -450, -700, -902]
ANCHOR_R = [800, 1000, 1176, 1300, 1351, 1322, 1200, 1018, 800, 540, 250, -30, -318, -600, -830, -1008]


def _music(n, ch, bits, seed=0):
    rng = np.random.default_rng(seed)
    amp = (1 << (bits - 1)) - 1
    t = np.arange(n)[:, None]
    x = np.sin(t * (0.013 + 0.004 * np.arange(ch))) * 0.5 * amp + rng.normal(0, amp * 0.01 + 1, (n, ch))
    return np.clip(np.round(x), -amp - 1, amp).astype(np.int64)


def test_streaminfo_and_every_metadata_block_behind_an_id3v2_tag(tmp_path):
    from musicgan_amd.audio import flac
    pcm = _music(5000, 2, 16)
    data = W.encode(pcm, 48000, 16, W.plain_frames(5000, 1152), id3=True, blocks=W.extra_blocks())
    info = flac.parse(data, "x.flac")
    assert (info.sample_rate, info.channels, info.bits, info.total_samples) == (48000, 2, 16, 5000)
    assert (info.min_block, info.max_block) == (1152, 1152)
    assert info.blocks == (0, 1, 2, 3, 4, 5, 6)
    assert info.md5 == W.pcm_md5(pcm, 16)
    assert data[info.audio_offset:info.audio_offset + 2] == b"\xff\xf8" and info.audio_end == len(data)
    path = tmp_path / "x.flac"
    path.write_bytes(data)
    assert flac.read_header(str(path)) == info


def test_wavio_info_reads_headers_of_flac_wav_and_aiff(tmp_path):
    import aifc
    from scipy.io import wavfile
    from musicgan_amd.audio import wavio
    pcm = _music(3000, 2, 16)
    (tmp_path / "a.flac").write_bytes(W.encode(pcm, 44100, 16, W.plain_frames(3000, 1024)))
    (tmp_path / "b.flac").write_bytes(W.encode(_music(700, 1, 24), 96000, 24, W.plain_frames(700, 256)))
    wavfile.write(str(tmp_path / "c.wav"), 22050, pcm.astype(np.int16))
    with aifc.open(str(tmp_path / "d.aiff"), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(3)
        f.setframerate(48000)
        f.writeframes(bytes(3 * 123))
    assert wavio.info(str(tmp_path / "a.flac")) == (3000, 2, 44100, 16)
    assert wavio.info(str(tmp_path / "b.flac")) == (700, 1, 96000, 24)
    assert wavio.info(str(tmp_path / "c.wav")) == (3000, 2, 22050, 16)
    assert wavio.info(str(tmp_path / "d.aiff")) == (123, 1, 48000, 24)


def test_refused_streams_raise_value_error_naming_the_file(tmp_path):
    from musicgan_amd.audio import flac, wavio
    bad = tmp_path / "not.flac"
    bad.write_bytes(b"RIFF" + bytes(60))
    with pytest.raises(ValueError, match="not.flac.*not a FLAC stream"):
        wavio.load(str(bad))
    ogg = tmp_path / "ogg.flac"
    ogg.write_bytes(b"OggS" + bytes(60))
    with pytest.raises(ValueError, match="Ogg"):
        wavio.load_pcm(str(ogg))
    # 32-bit: STREAMINFO bits - 1 = 31
    si = W.streaminfo(4096, 4096, 0, 0, 44100, 2, 32, 0, bytes(16))
    deep = tmp_path / "deep.flac"
    deep.write_bytes(b"fLaC" + W.metadata_block(0, si, True) + b"\xff\xf8")
    with pytest.raises(ValueError, match="32-bit"):
        wavio.info(str(deep))
    with pytest.raises(flac.FlacError, match="missing.flac"):
        wavio.load_pcm(str(tmp_path / "missing.flac"))
    trunc = tmp_path / "trunc.flac"
    trunc.write_bytes(ANCHOR[:30])
    with pytest.raises(ValueError, match="past the end"):
        wavio.info(str(trunc))


def test_reading_flac_without_a_gpu_raises_musicganhiperror(tmp_path, monkeypatch):
    from musicgan_amd import _lib
    from musicgan_amd.audio import wavio
    path = tmp_path / "a.flac"
    path.write_bytes(ANCHOR)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for fn in (wavio.load, wavio.load_pcm, wavio.load_pcm_device):
        with pytest.raises(_lib.MusicGanHipError, match="GPU"):
            fn(str(path))


def test_anchor_fields():
    from musicgan_amd.audio import flac
    info = flac.parse(ANCHOR)
    assert (info.sample_rate, info.channels, info.bits, info.total_samples, info.min_block, info.max_block) == (44100, 2, 16, 16, 16, 16)
    pcm = np.stack([ANCHOR_L, ANCHOR_R], axis=1)
    assert info.md5 == hashlib.md5(pcm.astype("<i2").tobytes()).digest()
    frame = ANCHOR[info.audio_offset:]
    assert frame[:2] == b"\xff\xf8"  # fixed blocking
    assert frame[2] >> 4 == 6 and frame[2] & 15 == 9  # block size from an 8-bit field; 44.1 kHz
    assert frame[3] >> 4 == 10 and (frame[3] >> 1) & 7 == 4 and frame[3] & 1 == 0  # mid/side; 16 bits
    assert frame[4] == 0 and frame[5] == 15  # frame number 0; block size - 1
    assert W.crc8(frame[:6]) == frame[6]
    assert W.crc16_many([frame])[0] == 0  # the CRC-16 at the end checks
    assert frame[7] == 0b0_001010_0  # mid: FIXED order 2, no wasted bits


def test_writer_matches_the_anchor_bit_for_bit():
    """the writer's coding of the anchor's PCM with the anchor's knobs gives the anchor's bytes (the two were derived apart)"""
    pcm = np.stack([ANCHOR_L, ANCHOR_R], axis=1)
    subs = [W.SubSpec(kind="fixed", order=2, method=0, porder=1, params=[2, None], escape={1: 7}),
            W.SubSpec(kind="lpc", order=2, precision=5, shift=2, coefs=[7, -3], wasted=1, method=1, porder=0, params=[3])]
    data = W.encode(pcm, 44100, 16, [W.FrameSpec(size=16, assign="mid_side", subs=subs, bs_code="8bit")])
    assert data[42:] == ANCHOR[42:]  # the frame (STREAMINFO differs: the writer fills in the frame sizes)
    assert data[:12] == ANCHOR[:12] and data[18:] == ANCHOR[18:]


def test_flac_kernels_do_not_use_scratch_memory():
    import re
    from musicgan_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_usage().items() if re.search(r"flac_", k)}
    assert len(hits) >= 6, sorted(hits)
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)


def test_flac_entry_points_are_host_callable_size_queries():
    from musicgan_amd import _lib
    lib = _lib.load()
    assert lib.mg_flac_padded_bytes(1) >= 16 + 4
    assert lib.mg_flac_padded_bytes(10000) % 16 == 0 and lib.mg_flac_padded_bytes(10000) >= 10000 + 16
    assert lib.mg_flac_ws_bytes(10000, 100) > 100 * 48
    assert lib.mg_flac_ws_bytes(0, 100) == 0
