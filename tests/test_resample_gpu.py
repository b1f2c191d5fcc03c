"""GPU: polyphase resampling (mg_resample_pcm) -- audio.resample against the float64 restatement of
torchaudio.functional.resample, the fused PCM path against its composition, physical checks on sines, and the `resample` option
of wav_to_stft and create_dataset."""
import glob
import os

import numpy as np
import pytest
import torch

from test_resample_cpu import PAIRS, full_kernel, resample_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("orig,new", PAIRS)
def test_resample_matches_float64_torchaudio_form(orig, new):
    from musicgan_amd import audio
    o, n, w, _ = full_kernel(orig, new)
    rng = np.random.default_rng(orig + new)
    for length in (1, 7, 2 * w, o * n + 3, orig * 3 // 2 + 17):
        for rows in (1, 3):
            x = (rng.random((rows, length), dtype=np.float32) * 2 - 1) * 0.7
            if rows == 1:
                x = x[0]
            got = audio.resample(torch.from_numpy(x).to(DEV), orig, new)
            want = resample_f64(x, orig, new)
            assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape, (length, rows)
            err = float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want))) if want.size else 0.0
            assert err <= 1e-6 * float(np.abs(x).max()), (orig, new, length, rows, err)


def test_resample_of_strided_rows_and_leading_dims():
    """(..., time): leading dimensions flattened, rows read through their stride (a slice along time is not copied)"""
    from musicgan_amd import audio
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((2, 3, 5000), dtype=np.float32) - 0.5).to(DEV)
    view = x[..., 100:4100]
    got = audio.resample(view, 48000, 44100)
    assert tuple(got.shape) == (2, 3, 3675)
    want = audio.resample(view.contiguous(), 48000, 44100)
    assert torch.equal(got, want)
    assert torch.equal(got[1, 2], audio.resample(view[1, 2].contiguous(), 48000, 44100))
    assert audio.resample(torch.zeros(4, 0, device=DEV), 48000, 44100).shape == (4, 0)


def test_fused_pcm_path_is_bit_identical_to_the_composition():
    """ops.resample_pcm: normalisation + mono mean on load, the same bits as resample(pcm_to_mono(pcm))"""
    from musicgan_amd import audio, ops
    rng = np.random.default_rng(11)
    frames = 48000 * 2 + 33
    cases = {
        "i16x2": rng.integers(-32768, 32767, (frames, 2), dtype=np.int16),
        "i32x1": rng.integers(-2 ** 31, 2 ** 31 - 1, (frames, 1), dtype=np.int32),
        "u8x2": rng.integers(0, 255, (frames, 2), dtype=np.uint8),
        "f32x2": (rng.random((frames, 2), dtype=np.float32) - 0.5),
    }
    for orig in (48000, 22050, 96000):
        for name, pcm in cases.items():
            dev = torch.from_numpy(pcm).to(DEV)
            got = ops.resample_pcm(dev, orig, 44100)
            want = audio.resample(ops.pcm_to_mono(dev), orig, 44100)
            assert torch.equal(got, want), (orig, name)
    dev = torch.from_numpy(cases["i16x2"]).to(DEV)
    assert torch.equal(ops.resample_pcm(dev, 44100, 44100), ops.pcm_to_mono(dev))


@pytest.mark.parametrize("orig", [48000, 96000, 32000, 22050, 16000])
def test_sine_at_1khz_arrives_as_the_ideal_44k1_sine(orig):
    from musicgan_amd import audio
    t = np.arange(2 * orig) / orig
    x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    y = audio.resample(torch.from_numpy(x).to(DEV), orig, 44100).cpu().numpy().astype(np.float64)
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 44100)
    err = np.max(np.abs(y - ideal)[1000:-1000])
    assert err <= 1e-3, err


def test_tone_above_the_new_nyquist_is_removed():
    from musicgan_amd import audio
    t = np.arange(2 * 96000) / 96000
    x = np.sin(2 * np.pi * 30000.0 * t).astype(np.float32)
    y = audio.resample(torch.from_numpy(x).to(DEV), 96000, 44100).cpu().numpy()
    assert np.max(np.abs(y[1000:-1000])) <= 1e-2


def test_wav_to_stft_with_resampling(tmp_path):
    from scipy.io import wavfile
    from musicgan_amd import audio
    from oracle import audio as OA
    rng = np.random.default_rng(17)
    pcm48 = rng.integers(-20000, 20000, (48000 + 4321, 2), dtype=np.int16)
    p48 = str(tmp_path / "a48.wav")
    wavfile.write(p48, 48000, pcm48)
    got = audio.wav_to_stft(p48, resample=True)
    mono = (pcm48.astype(np.float32) / 32768.0).T.mean(axis=0, dtype=np.float32)
    want = OA.stft(resample_f64(mono, 48000, 44100).astype(np.float32))
    assert tuple(got.shape) == want.shape
    err = float(np.max(np.abs(got.cpu().numpy() - want)))
    assert err <= 1e-5 * float(np.abs(want).max()), err
    with pytest.raises(AssertionError, match="Audio sample rate must be 44100Hz"):
        audio.wav_to_stft(p48)
    p44 = str(tmp_path / "a44.wav")
    wavfile.write(p44, 44100, pcm48)
    a, b = audio.wav_to_stft(p44, resample=True), audio.wav_to_stft(p44)
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def _composition(path):
    """the public-API composition create_dataset(resample=True) must reproduce, sample for sample"""
    from musicgan_amd import audio, ops
    from musicgan_amd.audio import wavio
    pcm, sr = wavio.load_pcm(path)
    mono = ops.pcm_to_mono(torch.from_numpy(np.ascontiguousarray(pcm)).to(DEV))
    c = audio.stft_from_waveform(audio.resample(mono, sr, audio.SAMPLE_RATE))
    if c.shape[1] - 1 < audio.N_VEC:
        return None
    return audio.stft_to_stacked_phase_magn(c).double().cpu()


def test_create_dataset_resamples_and_numbers_like_the_composition(tmp_path, monkeypatch):
    from scipy.io import wavfile
    import musicgan_amd
    from musicgan_amd import audio
    from musicgan_amd.audio import wavio
    rng = np.random.default_rng(23)
    wav_dir = tmp_path / "wav"
    wav_dir.mkdir()
    # a: 48 kHz stereo int16, 2 samples; b: too short only after resampling; c: 22.05 kHz mono, 1; d: 44.1 kHz, 1
    wavfile.write(str(wav_dir / "a.wav"), 48000, rng.integers(-30000, 30000, (256 * 1140, 2), dtype=np.int16))
    wavfile.write(str(wav_dir / "b.wav"), 48000, rng.integers(-30000, 30000, (256 * 540, 1), dtype=np.int16))
    wavio.save(str(wav_dir / "c.wav"), torch.rand(1, 256 * 300, generator=torch.Generator().manual_seed(1)) - 0.5, 22050)
    wavio.save(str(wav_dir / "d.wav"), torch.rand(2, 256 * 530, generator=torch.Generator().manual_seed(2)) - 0.5, 44100)
    assert 1 + 256 * 540 // 256 - 1 >= audio.N_VEC  # b would make a sample at its own rate
    per_file = {os.path.basename(p): _composition(p) for p in glob.glob(str(wav_dir / "*.wav"))}
    assert {k: 0 if v is None else v.shape[0] for k, v in per_file.items()} == {"a.wav": 2, "b.wav": 0, "c.wav": 1, "d.wav": 1}
    # samples are numbered in glob order (the reference's create_dataset.py:32), the skipped file takes no index
    want = torch.cat([v for v in per_file.values() if v is not None])
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    single = tmp_path / "single"
    with pytest.raises(AssertionError, match="Audio sample rate must be 44100Hz"):
        musicgan_amd.create_dataset(str(wav_dir / "*.wav"), str(tmp_path / "refused"))
    musicgan_amd.create_dataset(str(wav_dir / "*.wav"), str(single), resample=True)
    names = sorted(f for f in os.listdir(single) if f.endswith(".pt"))
    assert names == sorted(f"magn_phase_{i}.pt" for i in range(4))
    for i in range(4):
        assert torch.equal(torch.load(str(single / f"magn_phase_{i}.pt")), want[i]), i
    assert audio.has_packed(str(single))
    ref_ds, ds = audio.AudioDataset(str(single)), audio.PackedAudioDataset(str(single))
    assert len(ds) == len(ref_ds) == 4
    for i in range(4):
        assert torch.equal(ds[i].double(), ref_ds[i]), i
    # WORLD_SIZE=2: the global numbering counts each file's samples from its resampled length
    sharded = tmp_path / "sharded"
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("LOCAL_RANK", "0")
        musicgan_amd.create_dataset(str(wav_dir / "*.wav"), str(sharded), resample=True)
    assert sorted(f for f in os.listdir(sharded) if f.endswith(".pt")) == names
    for name in names:
        assert torch.equal(torch.load(str(single / name)), torch.load(str(sharded / name))), name
