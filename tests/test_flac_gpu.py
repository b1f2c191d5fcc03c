"""GPU: FLAC decoding (csrc/flac.hip) -- exact round trips of streams written by tests/flac_writer.py over every coding knob,
edge cases, the anchor frame, false sync codes, corrupt and truncated streams, and bit-identity with the same PCM as WAV / AIFF
through wavio.load, load_pcm, wav_to_stft and create_dataset."""
import os

import numpy as np
import pytest
import torch

import flac_writer as W
from test_flac_cpu import ANCHOR, ANCHOR_L, ANCHOR_R, _music

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _just(pcm, bits):
    """the int16 / int32 container values load_pcm gives: samples left-justified"""
    pcm = np.asarray(pcm, dtype=np.int64)
    if bits <= 16:
        return (pcm << (16 - bits)).astype(np.int16)
    return (pcm << (32 - bits)).astype(np.int32)


def _decode(tmp_path, data, name="x.flac"):
    from musicgan_amd.audio import wavio
    path = tmp_path / name
    path.write_bytes(data)
    return wavio.load_pcm(str(path))


def _random_frames(rng, pcm, rate):
    n, ch = pcm.shape
    frames, at = [], 0
    while at < n:
        bs = int(min(n - at, rng.choice([1, 16, 192, 255, 256, 576, 1000, 1152, 4096, 4608, 8192])))
        assign = str(rng.choice(list(W.ASSIGN))) if ch == 2 else "independent"
        subs = []
        for c in range(ch):
            kind = str(rng.choice(["verbatim", "constant", "fixed", "fixed", "lpc", "lpc", "lpc"]))
            seg = pcm[at:at + bs, c]
            if kind == "constant" and (assign != "independent" or np.any(seg != seg[0])):
                kind = "verbatim"
            order = int(rng.integers(0, 5)) if kind == "fixed" else int(rng.integers(1, 33))
            if kind in ("fixed", "lpc") and order > bs:
                kind = "verbatim"
            porder = W.biggest_porder(bs, order, int(rng.integers(0, 16)))
            esc = None
            if rng.random() < 0.25:
                esc = {int(rng.integers(0, 1 << porder)): None}
            subs.append(W.SubSpec(kind=kind, order=order, precision=int(rng.integers(1, 16)) if kind == "lpc" else 12,
                                  method=int(rng.integers(0, 2)), porder=porder, escape=esc))
        frames.append(W.FrameSpec(size=bs, assign=assign, subs=subs, bs_code=str(rng.choice(["auto", "8bit", "16bit"])) if bs <= 256
                                  else str(rng.choice(["auto", "16bit"])), rate_code=str(rng.choice(["auto", "streaminfo", "hz" if rate < 65536 else "10hz"])),
                                  bps_code=str(rng.choice(["auto", "streaminfo"]))))
        at += bs
    return frames


def _signal(rng, n, ch, bits, wasted=0):
    amp = (1 << (bits - 1)) - 1
    t = np.arange(n)[:, None]
    x = np.sin(t * rng.uniform(0.001, 0.2, ch)) * rng.uniform(0.1, 0.9) * amp + rng.normal(0, amp * 0.02 + 1, (n, ch))
    if rng.random() < 0.2:
        x[:, 0] = x[0, 0]  # a constant channel
    x = np.clip(np.round(x), -amp - 1, amp).astype(np.int64)
    if wasted:
        x = (x >> wasted) << wasted
    if ch == 2 and rng.random() < 0.3:
        x[:, 1] = x[:, 0] - rng.integers(-3, 4, n)  # strongly correlated stereo
        x = np.clip(x, -amp - 1, amp)
    return x


@pytest.mark.parametrize("seed", range(12))
def test_round_trip_matrix(tmp_path, seed):
    """channels 1-8, depths 4-24, block sizes 1-8192 (codes auto / 8-bit / 16-bit), rate and depth codes or STREAMINFO, all channel
    assignments, CONSTANT / VERBATIM / FIXED 0-4 / LPC 1-32 (precision 1-15), wasted bits, Rice and Rice2, partition orders up to
    15, escape partitions, fixed and variable blocking, ID3v2 and other metadata blocks"""
    rng = np.random.default_rng(seed)
    ch = [1, 2, 2, 2, 3, 4, 5, 6, 7, 8, 2, 1][seed]
    bits = [4, 8, 12, 16, 16, 20, 24, 13, 17, 5, 24, 21][seed]
    n = int(rng.integers(1, 30000))
    pcm = _signal(rng, n, ch, bits, wasted=int(rng.integers(0, min(3, bits - 1))))
    rate = [44100, 48000, 8000, 96000, 22050, 44100, 192000, 11025, 44100, 32000, 44100, 47999][seed]
    data = W.encode(pcm, rate, bits, _random_frames(rng, pcm, rate), blocking=seed % 2, id3=seed % 3 == 0,
                    blocks=W.extra_blocks() if seed % 4 == 1 else ())
    got, sr = _decode(tmp_path, data)
    assert sr == rate and got.dtype == (np.int16 if bits <= 16 else np.int32)
    assert np.array_equal(got, _just(pcm, bits)), seed


def test_anchor_decodes_to_its_samples(tmp_path):
    got, sr = _decode(tmp_path, ANCHOR)
    assert sr == 44100 and got.dtype == np.int16
    assert got[:, 0].tolist() == ANCHOR_L and got[:, 1].tolist() == ANCHOR_R


def test_edge_cases(tmp_path):
    rng = np.random.default_rng(7)
    # block size 65535 and a last frame of 1 sample
    pcm = _signal(rng, 65536, 2, 16)
    frames = [W.FrameSpec(size=65535, subs=[W.SubSpec(kind="lpc", order=32, porder=0)] * 2), W.FrameSpec(size=1)]
    frames[1].subs = [W.SubSpec(kind="verbatim")] * 2
    got, _ = _decode(tmp_path, W.encode(pcm, 44100, 16, frames, blocking=1), "a.flac")
    assert np.array_equal(got, _just(pcm, 16))
    # unary runs spanning many 64-bit words: Rice parameter 0 for residuals of +-5000
    x = np.zeros((4096, 1), dtype=np.int64)
    x[::7, 0] = 5000
    x[3::11, 0] = -4000
    sub = W.SubSpec(kind="fixed", order=0, porder=0, params=[0])
    got, _ = _decode(tmp_path, W.encode(x, 44100, 16, [W.FrameSpec(size=4096, subs=[sub])]), "b.flac")
    assert np.array_equal(got, _just(x, 16))
    # extreme values at each depth, a 25-bit side channel, 32-bit-overflowing LPC (order 32, precision 15 on a side channel)
    for bits in (4, 8, 12, 16, 20, 24):
        lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
        x = np.array([[hi, lo], [lo, hi], [hi, hi], [lo, lo]] * 300, dtype=np.int64)
        for assign in W.ASSIGN:
            for kind in ("verbatim", "lpc", "fixed"):
                sub = W.SubSpec(kind=kind, order=32 if kind == "lpc" else 4, precision=15, porder=2)
                f = [W.FrameSpec(size=1200, assign=assign, subs=[sub, sub])]
                got, _ = _decode(tmp_path, W.encode(x, 44100, bits, f), f"c{bits}{assign}{kind}.flac")
                assert np.array_equal(got, _just(x, bits)), (bits, assign, kind)
    # total_samples == 0 in STREAMINFO: the decoder counts
    pcm = _signal(rng, 10001, 2, 16)
    data = W.encode(pcm, 44100, 16, W.plain_frames(10001, 1024), total_samples=0)
    got, _ = _decode(tmp_path, data, "d.flac")
    assert np.array_equal(got, _just(pcm, 16))
    from musicgan_amd.audio import wavio
    assert wavio.info(str(tmp_path / "d.flac")) == (10001, 2, 44100, 16)


def test_planted_fake_header_decodes_exactly(tmp_path):
    """a VERBATIM subframe whose samples spell the next frame's header (valid CRC-8, the right number) is a false sync code"""
    rng = np.random.default_rng(3)
    pcm = _signal(rng, 3 * 1024, 1, 16)
    frames = [W.FrameSpec(size=1024, subs=[W.SubSpec(kind="verbatim")]), W.FrameSpec(size=1024, subs=[W.SubSpec(kind="fixed", order=2)]),
              W.FrameSpec(size=1024, subs=[W.SubSpec(kind="verbatim")])]
    raw = []
    W.encode(pcm, 44100, 16, frames, frame_bytes_out=raw)
    head = raw[1][:6]  # frame 1's header: 4 bytes, number 1, CRC-8
    assert W.crc8(head[:5]) == head[5]
    # frame 0's samples 500..502 spell it: its VERBATIM samples start at byte 7 of the frame, so they are byte aligned
    pcm[500:503, 0] = np.frombuffer(head, dtype=">i2").astype(np.int64)
    data = W.encode(pcm, 44100, 16, frames, total_samples=0)
    assert data.count(head) == 2  # the header occurs twice in the stream
    got, _ = _decode(tmp_path, data)
    assert np.array_equal(got, _just(pcm, 16))
    data = W.encode(pcm, 44100, 16, frames)  # with the count in STREAMINFO as well
    got, _ = _decode(tmp_path, data, "y.flac")
    assert np.array_equal(got, _just(pcm, 16))


def test_corrupt_and_truncated_streams_raise_naming_the_frame(tmp_path):
    rng = np.random.default_rng(5)
    pcm = _signal(rng, 8 * 1024, 2, 16)
    raw = []
    data = W.encode(pcm, 44100, 16, W.plain_frames(8 * 1024, 1024), frame_bytes_out=raw)
    start = len(data) - sum(len(r) for r in raw)
    k = 5
    at = start + sum(len(r) for r in raw[:k])
    for where in (len(raw[k]) // 2, 3):  # a bit in the residuals of frame k; a bit in its header
        bad = bytearray(data)
        bad[at + where] ^= 0x10
        with pytest.raises(ValueError, match=f"frame {k} at byte offset {at}"):
            _decode(tmp_path, bytes(bad), f"bad{where}.flac")
    with pytest.raises(ValueError, match="truncated"):
        _decode(tmp_path, data[:at + 100], "cut.flac")
    with pytest.raises(ValueError, match="truncated"):
        _decode(tmp_path, data[:at], "cut2.flac")  # cut at a frame boundary: STREAMINFO's count is not reached


def _same_pcm_files(tmp_path, rng, n, rate=44100):
    """the same stereo PCM as FLAC (16 bit) and WAV, and 24-bit as FLAC and AIFF"""
    import aifc
    from scipy.io import wavfile
    pcm16 = _signal(rng, n, 2, 16)
    pcm24 = _signal(rng, n, 2, 24)
    (tmp_path / "s16.flac").write_bytes(W.encode(pcm16, rate, 16, W.plain_frames(n, 4096, assign="mid_side")))
    wavfile.write(str(tmp_path / "s16.wav"), rate, pcm16.astype(np.int16))
    (tmp_path / "s24.flac").write_bytes(W.encode(pcm24, rate, 24, W.plain_frames(n, 4096)))
    raw = (pcm24.astype(np.int64).reshape(-1) & 0xFFFFFF).astype(">u4").view(np.uint8).reshape(-1, 4)[:, 1:].tobytes()
    with aifc.open(str(tmp_path / "s24.aiff"), "wb") as f:
        f.setnchannels(2)
        f.setsampwidth(3)
        f.setframerate(rate)
        f.writeframes(raw)


def test_flac_is_bit_identical_to_wav_and_aiff(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.audio import wavio
    _same_pcm_files(tmp_path, np.random.default_rng(11), 256 * 700)
    for a, b in (("s16.flac", "s16.wav"), ("s24.flac", "s24.aiff")):
        fa, fb = str(tmp_path / a), str(tmp_path / b)
        xa, sa = wavio.load(fa)
        xb, sb = wavio.load(fb)
        assert sa == sb and torch.equal(xa, xb), a
        pa, _ = wavio.load_pcm(fa)
        pb, _ = wavio.load_pcm(fb)
        assert pa.dtype == pb.dtype and np.array_equal(pa, pb), a
        assert torch.equal(wavio.load_pcm_device(fa).cpu(), torch.from_numpy(np.ascontiguousarray(pb)))
        assert torch.equal(audio.wav_to_stft(fa).cpu(), audio.wav_to_stft(fb).cpu()), a
        assert wavio.info(fa) == wavio.info(fb), a


def _by_source(pattern, out_dir):
    """{source file stem: [bytes of its .pt samples]}: samples are numbered over the files in glob order (create_dataset.py:32),
    which follows each directory's own listing order, so two directories are compared file by file"""
    import glob
    from musicgan_amd import audio, ops
    from musicgan_amd.audio import wavio
    from musicgan_amd.create_dataset import _nb_samples
    got, idx = {}, 0
    for p in glob.glob(pattern):
        frames, _, sr, _ = wavio.info(p)
        if sr != audio.SAMPLE_RATE:
            frames = ops.resample_len(frames, sr, audio.SAMPLE_RATE)
        k = _nb_samples(frames, audio.N_VEC)
        got[os.path.splitext(os.path.basename(p))[0]] = [(out_dir / f"magn_phase_{idx + i}.pt").read_bytes() for i in range(k)]
        idx += k
    assert sorted(f for f in os.listdir(out_dir) if f.endswith(".pt")) == sorted(f"magn_phase_{i}.pt" for i in range(idx))
    return got


def test_create_dataset_flac_equals_wav_byte_for_byte(tmp_path, monkeypatch):
    import shutil
    import musicgan_amd
    from musicgan_amd import audio
    rng = np.random.default_rng(13)
    for sub in ("wav", "flac"):
        (tmp_path / sub).mkdir()
    for i, n in enumerate((256 * 1100, 256 * 530, 256 * 100)):
        _same_pcm_files(tmp_path, rng, n)
        shutil.move(str(tmp_path / "s16.wav"), str(tmp_path / "wav" / f"f{i}.wav"))
        shutil.move(str(tmp_path / "s16.flac"), str(tmp_path / "flac" / f"f{i}.flac"))
    # 48 kHz files, resampled
    for i, n in enumerate((256 * 1200, 256 * 600)):
        _same_pcm_files(tmp_path, rng, n, rate=48000)
        shutil.move(str(tmp_path / "s16.wav"), str(tmp_path / "wav" / f"g{i}.wav"))
        shutil.move(str(tmp_path / "s16.flac"), str(tmp_path / "flac" / f"g{i}.flac"))
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    wav_pat, flac_pat = str(tmp_path / "wav" / "*.wav"), str(tmp_path / "flac" / "*.flac")
    musicgan_amd.create_dataset(wav_pat, str(tmp_path / "out_wav"), resample=True)
    musicgan_amd.create_dataset(flac_pat, str(tmp_path / "out_flac"), resample=True)
    a, b = _by_source(wav_pat, tmp_path / "out_wav"), _by_source(flac_pat, tmp_path / "out_flac")
    assert sorted(a) == sorted(b) and sum(len(v) for v in a.values()) >= 5 and len(a["f2"]) == 0
    for stem in a:
        assert a[stem] == b[stem], stem
    # the side-car of the FLAC run serves what its .pt files hold
    assert audio.has_packed(str(tmp_path / "out_flac"))
    ref_ds, ds = audio.AudioDataset(str(tmp_path / "out_flac")), audio.PackedAudioDataset(str(tmp_path / "out_flac"))
    assert len(ds) == len(ref_ds)
    for i in range(len(ds)):
        assert torch.equal(ds[i].double(), ref_ds[i]), i
    # WORLD_SIZE=2: the counting pass reads FLAC headers only, the numbering is the single-process one
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("LOCAL_RANK", "0")
        musicgan_amd.create_dataset(flac_pat, str(tmp_path / "sharded"), resample=True)
    assert _by_source(flac_pat, tmp_path / "sharded") == b


def test_two_minute_stereo_stream_bit_exact(tmp_path):
    rng = np.random.default_rng(17)
    n = 44100 * 120
    pcm = _music(n, 2, 16, seed=17)
    sub = W.SubSpec(kind="fixed", order=2, porder=4)
    data = W.encode(pcm, 44100, 16, W.plain_frames(n, 4096, assign="mid_side", subs=[sub, sub]))
    got, _ = _decode(tmp_path, data)
    assert len(W.plain_frames(n, 4096)) == 1292
    assert np.array_equal(got, _just(pcm, 16))
