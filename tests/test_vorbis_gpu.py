"""GPU: Ogg Vorbis decoding (csrc/vorbis.hip) against the float64 reader (tests/vorbis_reader.py) on the libvorbis fixture and on
streams tests/vorbis_writer.py lays out from its packets (pages of a few segments, packets across pages, start and end trimming,
long streams, a 48 kHz header), corrupt and truncated pages, and wav_to_stft / create_dataset against the same PCM as WAV."""
import struct

import numpy as np
import pytest
import torch

import vorbis_reader as R
import vorbis_writer as W
from musicgan_amd.audio import vorbis as V

pytestmark = pytest.mark.gpu


def _write(tmp_path, data, name="x.ogg"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def _close(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    for c in range(ref.shape[1]):
        tol = 1e-5 * max(float(np.abs(ref[:, c]).max()), 1e-30)
        err = float(np.abs(got[:, c].astype(np.float64) - ref[:, c]).max())
        assert err <= tol, (c, err, tol)


def _stream_at(packets, rate: int, **kw) -> bytes:
    """a stream of `packets` whose identification header names another sample rate"""
    heads, _, _ = W.fixture_packets()
    ident = bytearray(heads[0])
    ident[12:16] = struct.pack("<I", rate)
    return W.stream(packets, heads=[bytes(ident)] + heads[1:], **kw)


def test_fixture_matches_the_reader_and_is_deterministic(tmp_path):
    from musicgan_amd.audio import wavio
    ref = R.decode_file(W.fixture_bytes())
    pcm, sr = wavio.load_pcm(W.FIXTURE)
    assert sr == 44100 and pcm.dtype == np.float32 and pcm.shape == (22050, 2)
    _close(pcm, ref)
    a, b = wavio.load_pcm_device(W.FIXTURE), wavio.load_pcm_device(W.FIXTURE)
    assert a.dtype == torch.float32 and torch.equal(a, b)
    assert torch.equal(a.cpu(), torch.from_numpy(pcm))
    x, sr = wavio.load(W.FIXTURE)
    assert sr == 44100 and torch.equal(x, torch.from_numpy(np.ascontiguousarray(pcm.T)))
    p = _write(tmp_path, W.fixture_bytes(), "y.OGA")
    assert torch.equal(wavio.load_pcm_device(p), a)


@pytest.mark.parametrize("segs,pad,start,end", [(255, 0, 0, 0), (3, 600, 0, 0), (1, 300, 0, 700), (5, 0, 300, 0),
                                                (2, 1000, 0, 1500), (16, 0, 40, 0)])
def test_layouts_and_trimming_match_the_reader(tmp_path, segs, pad, start, end):
    """`pad` bytes after every packet's last bit (a decoder stops reading where the residues end) make packets of several
    segments, which pages of `segs` segments split"""
    from musicgan_amd.audio import wavio
    _, audio, _ = W.fixture_packets()
    data = W.stream([p + bytes(pad) for p in audio], max_segments=segs, start_trim=start, end_trim=end)
    vs = V.parse(data, "s")
    assert vs.trim_start == start and vs.frames == 22464 - start - end
    if pad:
        assert len(vs.pages.offset) > 2 + 26 * (pad // 255) // segs  # packets span pages
    _close(wavio.load_pcm(_write(tmp_path, data))[0], R.decode_file(data))


def test_packet_orders_the_encoder_never_writes(tmp_path):
    """short and long blocks in every order (long -> short -> long, short after silence, silent packets first): the window
    slopes and overlap positions follow each packet's flags and its neighbours' sizes"""
    from musicgan_amd.audio import wavio
    _, audio, _ = W.fixture_packets()
    order = [5, 0, 13, 1, 2, 14, 14, 4, 12, 3, 20, 6, 0, 1, 25, 11]
    data = W.stream([audio[k] for k in order], max_segments=4, end_trim=37)
    _close(wavio.load_pcm(_write(tmp_path, data))[0], R.decode_file(data))


def test_corrupt_and_truncated_pages_raise(tmp_path):
    from musicgan_amd.audio import wavio
    _, audio, _ = W.fixture_packets()
    data = W.stream(audio, max_segments=6)
    vs = V.parse(data, "s")
    k = vs.header_pages + 3
    off = int(vs.pages.body[k]) + 1
    bad = bytearray(data)
    bad[off] ^= 0x10
    with pytest.raises(ValueError, match=f"page {k} at byte offset {int(vs.pages.offset[k])}"):
        wavio.load_pcm_device(_write(tmp_path, bytes(bad)))
    with pytest.raises(ValueError, match="truncated"):
        wavio.load_pcm_device(_write(tmp_path, data[:-5], "t.ogg"))


def test_wav_to_stft_of_ogg_equals_stft_of_its_pcm(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.audio.functions import stft_from_pcm
    from musicgan_amd.audio import wavio
    _, packets, _ = W.fixture_packets()
    data = W.stream(packets + packets[4:] * 3)
    p = _write(tmp_path, data)
    assert torch.equal(audio.wav_to_stft(p).cpu(), stft_from_pcm(wavio.load_pcm_device(p)).cpu())
    p48 = _write(tmp_path, _stream_at(packets + packets[4:] * 3, 48000), "r48.ogg")
    assert wavio.info(p48)[2] == 48000
    with pytest.raises(AssertionError):
        audio.wav_to_stft(p48)
    got = audio.wav_to_stft(p48, resample=True).cpu()
    assert torch.equal(got, stft_from_pcm(wavio.load_pcm_device(p48), sample_rate=48000).cpu())


def _long_stream(reps, rate=44100):
    heads, packets, _ = W.fixture_packets()
    return _stream_at(packets + packets[4:] * reps, rate, max_segments=16)


def test_create_dataset_ogg_equals_wav_byte_for_byte(tmp_path, monkeypatch):
    import musicgan_amd
    from musicgan_amd.audio import wavio
    from test_flac_gpu import _by_source
    for sub in ("wav", "ogg"):
        (tmp_path / sub).mkdir()
    # about 7 s at 44.1 kHz (15 repeats of the fixture's long packets), a shorter one, and a 48 kHz one (resampled)
    for name, reps, rate in (("f0", 14, 44100), ("f1", 6, 44100), ("g0", 14, 48000)):
        p = _write(tmp_path / "ogg", _long_stream(reps, rate), f"{name}.ogg")
        pcm, sr = wavio.load_pcm(p)
        assert sr == rate
        wavio.save(str(tmp_path / "wav" / f"{name}.wav"), torch.from_numpy(np.ascontiguousarray(pcm.T)), sr)
        assert wavio.info(p)[:3] == wavio.info(str(tmp_path / "wav" / f"{name}.wav"))[:3]
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    wav_pat, ogg_pat = str(tmp_path / "wav" / "*.wav"), str(tmp_path / "ogg" / "*.ogg")
    musicgan_amd.create_dataset(wav_pat, str(tmp_path / "out_wav"), resample=True)
    musicgan_amd.create_dataset(ogg_pat, str(tmp_path / "out_ogg"), resample=True)
    a, b = _by_source(wav_pat, tmp_path / "out_wav"), _by_source(ogg_pat, tmp_path / "out_ogg")
    assert sorted(a) == sorted(b) and sum(len(v) for v in a.values()) >= 2
    for stem in a:
        assert a[stem] == b[stem], stem
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("LOCAL_RANK", "0")
        musicgan_amd.create_dataset(ogg_pat, str(tmp_path / "sharded"), resample=True)
    assert _by_source(ogg_pat, tmp_path / "sharded") == b


def test_long_stream_matches_the_reader_in_pieces(tmp_path):
    """a stream of 200 packets decoded on the device against the reader (one run, no dependence on the packet count)"""
    from musicgan_amd.audio import wavio
    data = _long_stream(9)
    _close(wavio.load_pcm(_write(tmp_path, data))[0], R.decode_file(data))
