"""GPU: FLAC encoding (csrc/flac_encode.hip) -- round trips over channels x depths x lengths x signals read through the product's
decoder (wavio.load_pcm) and the independent test-side reader (tests/flac_reader.py), STREAMINFO, the codings actually chosen,
compression against tests/flac_writer.py, and the public paths: wavio.save, magn_phase_to_wav, generate and create_dataset."""
import os
import sys

import numpy as np
import pytest
import torch

import flac_reader as R
import flac_writer as W

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_flac import music  # noqa: E402  (the benchmark's music-like signal)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENGTHS = (1, 4095, 4096, 4097, 3 * 4096 + 17, 100_000)
SIGNALS = ("silence", "dc", "square", "noise", "music", "ramp")


def quantise(x, bits):
    """the stated rule: clamp(rint(x 2^(b-1)), -2^(b-1), 2^(b-1) - 1), in x's own precision (an exact power-of-two scaling)"""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(np.int64)
    top = 1 << (bits - 1)
    return np.clip(np.rint(x * x.dtype.type(top)), -top, top - 1).astype(np.int64)


def signal(kind, n, ch, bits, seed=0):
    """(channels, n) float32"""
    rng = np.random.default_rng(seed)
    if kind == "silence":
        return np.zeros((ch, n), np.float32)
    if kind == "dc":
        return np.full((ch, n), 0.25, np.float32) * (1 + np.arange(ch, dtype=np.float32)[:, None]) / ch
    if kind == "square":  # full scale and beyond: clips
        t = np.arange(n)
        return np.stack([np.where((t // (50 + 7 * c)) % 2 == 0, 1.2, -1.2) for c in range(ch)]).astype(np.float32)
    if kind == "noise":
        return rng.uniform(-1, 1, (ch, n)).astype(np.float32)
    if kind == "music":
        cols = [music(n, seed + c // 2)[:, c % 2] for c in range(ch)]
        return (np.stack(cols) / 32768.0).astype(np.float32)
    if kind == "ramp":  # 8 zero low bits: wasted bits
        top = 1 << (bits - 1)
        q = [(((np.arange(n) * (37 + 11 * c)) % (2 * top)) - top) & ~0xFF for c in range(ch)]
        return (np.stack(q) / top).astype(np.float32)
    raise ValueError(kind)


def just(q, bits):
    """what load_pcm returns for q: int16 at 16 bits, int32 left-justified at 24"""
    return q.astype(np.int16) if bits == 16 else (q << 8).astype(np.int32)


def write(tmp_path, x, rate, bits=None, name="x.flac"):
    from musicgan_amd.audio import wavio
    path = tmp_path / name
    wavio.save(str(path), torch.as_tensor(x), rate, bits)
    return path


@pytest.mark.parametrize("ch", (1, 2, 3, 8))
@pytest.mark.parametrize("bits", (16, 24))
@pytest.mark.parametrize("kind", SIGNALS)
def test_round_trip(tmp_path, ch, bits, kind):
    from musicgan_amd.audio import flac, wavio
    for n in LENGTHS:
        x = signal(kind, n, ch, bits, seed=n)
        q = quantise(x, bits).T
        path = write(tmp_path, x, 44100, bits, f"{kind}{n}.flac")
        data = path.read_bytes()
        pcm, sr = wavio.load_pcm(str(path))
        assert sr == 44100 and pcm.dtype == just(q, bits).dtype and np.array_equal(pcm, just(q, bits)), (kind, ch, bits, n)
        r = R.read(data, expect=q)
        info = flac.read_header(str(path))
        assert (info.sample_rate, info.channels, info.bits, info.total_samples) == (44100, ch, bits, n)
        block = n if n <= 4096 else 4096
        assert (info.min_block, info.max_block) == (block, block)
        sizes = [f.size for f in r.frames]
        assert (info.min_frame, info.max_frame) == (min(sizes), max(sizes))
        assert info.md5 == W.pcm_md5(q, bits)
        assert info.blocks == (0,) and info.audio_offset == 42
        assert len(r.frames) == (n + 4095) // 4096 and all(f.block == 4096 for f in r.frames[:-1])
        if kind == "silence":
            assert all(s.kind == "constant" for f in r.frames for s in f.subs)
        if kind == "ramp" and n > 1:
            assert all(s.wasted >= 7 for f in r.frames for s in f.subs if s.kind != "constant")  # mid: (L + R) >> 1


def test_silence_is_constant_and_small(tmp_path):
    path = write(tmp_path, np.zeros((2, 100_000), np.float32), 44100, 16)
    r = R.read(path.read_bytes())
    assert all(s.kind == "constant" for f in r.frames for s in f.subs)
    assert all(f.size <= 16 for f in r.frames)


def test_white_noise_stays_within_its_pcm_size(tmp_path):
    for bits in (16, 24):
        x = signal("noise", 100_000, 2, bits, seed=3)
        data = write(tmp_path, x, 44100, bits).read_bytes()
        nframes = (100_000 + 4095) // 4096
        assert len(data) <= 100_000 * 2 * bits // 8 + 16 * nframes + 42, bits


def test_music_is_mostly_lpc_and_loud_24_bit_uses_rice2(tmp_path):
    x = signal("music", 200_000, 2, 16)
    r = R.read(write(tmp_path, x, 44100, 16).read_bytes(), expect=quantise(x, 16).T)
    kinds = [s.kind for f in r.frames for s in f.subs]
    assert kinds.count("lpc") > 0.5 * len(kinds), kinds
    # loud 24-bit material: residuals around 2^20 need Rice parameters of 15 and more (5-bit fields)
    loud = np.random.default_rng(8).uniform(-0.1, 0.1, (2, 50_000)).astype(np.float32)
    r24 = R.read(write(tmp_path, loud, 44100, 24, "l24.flac").read_bytes(), expect=quantise(loud, 24).T)
    assert all(s.method == 1 for f in r24.frames for s in f.subs), [s for f in r24.frames for s in f.subs]


def test_each_stereo_assignment_is_chosen_where_it_pays(tmp_path):
    """A, B independent noise: L = A, R = A - B makes the side channel B and L the cheap pair; L = A + B, R = A favours S and R;
    R = -L makes the mid channel constant; R = 0 leaves nothing to gain from any transform"""
    n = 40_000
    rng = np.random.default_rng(5)
    a, b = rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, n)
    tune = music(n, 1)[:, 0].astype(np.int64)
    cases = {
        "independent": (tune, np.zeros(n, np.int64)),
        "left_side": (a, a - b),
        "side_right": (a + b, a),
        "mid_side": (tune, -tune),
    }
    for want, (left, right) in cases.items():
        pcm = np.stack([left, right]).astype(np.int16)
        r = R.read(write(tmp_path, torch.from_numpy(pcm), 44100, None, f"{want}.flac").read_bytes(), expect=pcm.T)
        got = [f.assign for f in r.frames]
        assert got.count(want) >= len(got) - 1, (want, got)


def test_compression_against_the_writer_lpc8(tmp_path):
    """60 s of 16-bit stereo music-like signal: no larger than 1.03 x tests/flac_writer.py with LPC order 8 (least squares),
    precision 12, partition order 4, the cheapest Rice parameters, block 4096 (the decode benchmark's encoding)"""
    n = 44100 * 60
    pcm = music(n)
    sub = W.SubSpec(kind="lpc", order=8, precision=12, porder=4)
    ref = W.encode(pcm, 44100, 16, W.plain_frames(n, 4096, assign="mid_side", subs=[sub, sub]))
    ours = write(tmp_path, torch.from_numpy(pcm.T.astype(np.int16).copy()), 44100).read_bytes()
    ratio = len(ours) / len(ref)
    print(f"\nFLAC encode, 60 s 16-bit stereo: {len(ours)} bytes = {len(ours) / (4 * n):.4f} of the PCM, "
          f"{ratio:.4f} of the writer's LPC-8 ({len(ref)} bytes)")
    assert ratio <= 1.03
    R.read(ours, expect=pcm)


def test_magn_phase_to_wav_writes_flac(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.audio import wavio
    from golden_util import load
    mp = torch.from_numpy(load("audio_codec.npz")["inv_in"]).to(DEV)
    wav = audio.magn_phase_to_waveform(mp).cpu().numpy()
    out = str(tmp_path / "x.flac")
    audio.magn_phase_to_wav(mp, out, 44100)
    q = quantise(wav, 24)
    pcm, sr = wavio.load_pcm(out)
    assert sr == 44100 and np.array_equal(pcm[:, 0], just(q, 24))
    R.read((tmp_path / "x.flac").read_bytes(), expect=q[:, None])
    back, _ = wavio.load(out)
    assert float(np.abs(back[0].numpy() - wav.clip(-1, 1)).max()) <= 2.0 ** -23


def test_generate_flac_equals_the_quantised_wav_run(tmp_path):
    import musicgan_amd
    from musicgan_amd.audio import wavio
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    g7 = Generator(8, end_layer=7)
    ck = str(tmp_path / "gen7.pt")
    torch.save(g7.state_dict(), ck)
    torch.manual_seed(21)
    musicgan_amd.generate(str(tmp_path / "w"), 8, ck, 1, 2)
    torch.manual_seed(21)
    musicgan_amd.generate(str(tmp_path / "f"), 8, ck, 1, 2, audio_format="flac")
    assert sorted(os.listdir(tmp_path / "f")) == ["sound_0.flac", "sound_1.flac"]
    assert sorted(os.listdir(tmp_path / "w")) == ["sound_0.wav", "sound_1.wav"]
    for i in range(2):
        w, sr = wavio.load_pcm(str(tmp_path / "w" / f"sound_{i}.wav"))
        f, sr2 = wavio.load_pcm(str(tmp_path / "f" / f"sound_{i}.flac"))
        assert sr == sr2 == 44100 and np.array_equal(f, just(quantise(w, 24), 24)), i


def test_int16_wav_copies_to_flac_and_back_and_create_dataset_agrees(tmp_path, monkeypatch):
    import shutil
    import musicgan_amd
    from scipy.io import wavfile
    from musicgan_amd.audio import wavio
    from test_flac_gpu import _by_source, _signal
    rng = np.random.default_rng(23)
    (tmp_path / "wav").mkdir()
    (tmp_path / "flac").mkdir()
    for i, n in enumerate((256 * 1100, 256 * 530, 256 * 100)):
        wavfile.write(str(tmp_path / "wav" / f"f{i}.wav"), 44100, _signal(rng, n, 2, 16).astype(np.int16))
    for i in range(3):
        src = str(tmp_path / "wav" / f"f{i}.wav")
        pcm, sr = wavio.load_pcm(src)
        dst = str(tmp_path / "flac" / f"f{i}.flac")
        wavio.save(dst, torch.from_numpy(np.array(pcm)).T, sr)  # a transposed (non-contiguous) int16 view
        back, sr2 = wavio.load_pcm(dst)
        assert sr2 == sr and back.dtype == np.int16 and np.array_equal(back, pcm), i
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    wav_pat, flac_pat = str(tmp_path / "wav" / "*.wav"), str(tmp_path / "flac" / "*.flac")
    musicgan_amd.create_dataset(wav_pat, str(tmp_path / "out_wav"))
    musicgan_amd.create_dataset(flac_pat, str(tmp_path / "out_flac"))
    a, b = _by_source(wav_pat, tmp_path / "out_wav"), _by_source(flac_pat, tmp_path / "out_flac")
    assert sorted(a) == sorted(b) and sum(len(v) for v in a.values()) >= 3
    for stem in a:
        assert a[stem] == b[stem], stem
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("LOCAL_RANK", "0")
        musicgan_amd.create_dataset(flac_pat, str(tmp_path / "sharded"))
    assert _by_source(flac_pat, tmp_path / "sharded") == b


def test_encoding_is_deterministic_and_takes_any_layout(tmp_path):
    from musicgan_amd import ops
    x = signal("music", 50_000, 3, 24, seed=4)
    big = torch.zeros(5, 60_000)
    big[1:4, 1000:51_000] = torch.from_numpy(x)
    view = big[1:4, 1000:51_000]  # rows 60 000 apart
    assert not view.is_contiguous()
    a = ops.flac_encode(torch.from_numpy(x).to(DEV), 48000)
    b = ops.flac_encode(torch.from_numpy(x).to(DEV), 48000)
    c = ops.flac_encode(view, 48000)  # a CPU view
    d = ops.flac_encode(big.to(DEV)[1:4, 1000:51_000], 48000)  # the same view on the device
    e = ops.flac_encode(torch.from_numpy(x.T.copy()).T, 48000)  # column-major
    f = ops.flac_encode(torch.from_numpy(x).double(), 48000)  # float64 of the same values
    assert a.dtype == torch.uint8 and a.device.type == "cpu"
    for other in (b, c, d, e, f):
        assert torch.equal(a, other)
    R.read(bytes(a.numpy()), expect=quantise(x, 24).T)
    mono = ops.flac_encode(torch.from_numpy(x[0]), 12345, 16)  # (samples,), a rate outside the header table
    r = R.read(bytes(mono.numpy()), expect=quantise(x[0], 16)[:, None])
    assert r.rate == 12345 and r.channels == 1


def test_non_finite_input_raises_and_writes_nothing(tmp_path):
    from musicgan_amd.audio import wavio
    for bad in (float("nan"), float("inf"), -float("inf")):
        x = torch.zeros(2, 9000)
        x[1, 7000] = bad
        x[1, 8000] = bad
        path = tmp_path / "bad.flac"
        with pytest.raises(ValueError, match=r"bad.flac.*sample 7000 of channel 1"):
            wavio.save(str(path), x.to(DEV), 44100)
        assert not path.exists()
