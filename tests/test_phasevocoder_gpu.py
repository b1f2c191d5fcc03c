"""GPU: the phase vocoder (csrc/phasevocoder.hip, musicgan_amd.pv_ops, audio.phase_vocoder / time_stretch / pitch_shift, the
stretch / pitch variants of create_dataset) against the float64 restatement in tests/phasevocoder_ref.py.

Tolerance (the parity table's convention, fitted to nothing): against `exact(float64)` the device may be off by
max(4 x own, 1e-6 x max|ref|), own = the largest distance of `mixed` (abs / angle in float32 by torch, the rest in float64) from the
float64 run on the same input.  Each test prints its figures before it asserts.  References are computed once per input."""
import math
import os
import sys
import wave
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phasevocoder_ref as R  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _tile():
    from musicgan_amd import pv_ops
    return pv_ops.TIME_TILE


SHAPES = [(1, 1, 2), (4, 9, 10), (5, 1, 1), (37, 11, 10), (130, 53, 50), (64, 2, 1), (64, 1, 2), (64, 8, 1), (16, 1, 8),
          (1536, 17, 18), (8192, 9, 10), (8192, 5, 4)]
TILE_SHAPES = ["tile-1", "tile", "tile+1", "2tile+3"]     # T around the kernel's time tile, at 9/10
CASES = [(k, s) for s in SHAPES + TILE_SHAPES for k in ("random", "tonal")] + [("silence", (37, 11, 10)), ("silence", (130, 53, 50))]


def _resolve(shape):
    if isinstance(shape, str):
        t = _tile()
        return {"tile-1": t - 1, "tile": t, "tile+1": t + 1, "2tile+3": 2 * t + 3}[shape], 9, 10
    return shape


def _id(case):
    kind, shape = case
    return f"{kind}-{shape}" if isinstance(shape, str) else f"{kind}-{shape[0]}-{shape[1]}_{shape[2]}"


# ---------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_parity(case):
    from musicgan_amd import audio
    kind, shape = case
    frames, p, q = _resolve(shape)
    X, ref, own, tol = R.case(kind, frames, p, q)
    got = audio.phase_vocoder(X.to(DEV), Fraction(p, q))
    assert tuple(got.shape) == (512, math.ceil(frames * q / p)) == tuple(ref.shape)
    assert got.dtype == torch.complex64 and got.is_cuda
    err = float((got.cpu().to(torch.complex128) - ref).abs().max())
    print(f"PARITY {kind} T={frames} {p}/{q}: err {err:.3e}, own {own:.3e}, tol {tol:.3e}, max|ref| {float(ref.abs().max()):.3f}")
    assert bool(torch.isfinite(torch.view_as_real(got)).all())
    assert err <= tol


def test_rate_forms_agree():
    """an int, a Fraction and a float name the same rate"""
    from musicgan_amd import audio, pv_ops
    X = R.random_spectrum(64, 1064).to(DEV)
    a = audio.phase_vocoder(X, 2)
    assert torch.equal(a, audio.phase_vocoder(X, Fraction(2))) and torch.equal(a, audio.phase_vocoder(X, 2.0))
    assert torch.equal(a, audio.phase_vocoder(X.cpu(), 2)) and torch.equal(a, pv_ops.phase_vocoder(X, 4, 2))
    assert torch.equal(audio.phase_vocoder(X, 0.9), audio.phase_vocoder(X, Fraction(9, 10)))


# ---------------------------------------------------------------- 2. rate 1 is the identity
@pytest.mark.parametrize("frames", [5, 130])
def test_rate_one_is_the_identity(frames):
    from musicgan_amd import audio
    X, ref, own, tol = R.case("random", frames, 1, 1)
    got = audio.phase_vocoder(X.to(DEV), 1)
    err = float((got.cpu().to(torch.complex128) - X.to(torch.complex128)).abs().max())
    print(f"IDENTITY T={frames}: err {err:.3e}, own {own:.3e}, tol {tol:.3e}")
    assert got.shape == X.shape and err <= tol


# ---------------------------------------------------------------- 3. what it means
def _peak_hz(wav, sample_rate=44100):
    spec = torch.fft.rfft(wav.double().cpu()).abs()
    return float(spec.argmax()) * sample_rate / wav.numel(), sample_rate / wav.numel()


def test_a_sinusoid_keeps_or_moves_its_pitch():
    from musicgan_amd import audio
    n_in = 2 * 44100
    x = (0.5 * torch.sin(2 * math.pi * 440.0 * torch.arange(n_in, dtype=torch.float64) / 44100.0)).float().to(DEV)
    frames = 1 + n_in // 256
    for rate in (Fraction(4, 5), Fraction(5, 4)):
        y = audio.time_stretch(x, rate)
        n = math.ceil(frames / rate)
        hz, width = _peak_hz(y)
        print(f"TIME STRETCH {rate}: {y.numel()} samples, peak {hz:.2f} Hz (bin width {width:.3f} Hz)")
        assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (256 * (n - 1),)
        assert abs(hz - 440.0) <= width
    for steps, want in ((12, 880.0), (-12, 220.0)):
        y = audio.pitch_shift(x, steps)
        hz, width = _peak_hz(y)
        print(f"PITCH SHIFT {steps:+d}: {y.numel()} samples, peak {hz:.2f} Hz (bin width {width:.3f} Hz)")
        assert tuple(y.shape) == (n_in,) and abs(hz - want) <= width


# ---------------------------------------------------------------- 4. the waveform calls are their compositions
def test_waveform_calls_are_their_compositions():
    from musicgan_amd import audio
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(256 * 40 + 17, generator=g) - 0.5).to(DEV)
    for rate in (Fraction(9, 10), 1.25):
        want = audio.istft(audio.phase_vocoder(audio.stft_from_waveform(x), rate))
        assert torch.equal(audio.time_stretch(x, rate), want)
    assert torch.equal(audio.time_stretch(x.cpu(), Fraction(9, 10)), audio.time_stretch(x, Fraction(9, 10)))
    for steps in (1, -3.5, 12):
        f = audio.pitch_ratio(steps)
        y = audio.resample(audio.time_stretch(x, 1 / f), f.numerator, f.denominator)
        want = torch.zeros_like(x)
        m = min(x.numel(), y.numel())
        want[:m] = y[:m]
        got = audio.pitch_shift(x, steps)
        assert got.shape == x.shape and torch.equal(got, want), steps
    with pytest.raises(ValueError):
        audio.time_stretch(x[:256 * 6], 4)    # 7 frames -> n = 2: istft's error


# ---------------------------------------------------------------- 5. create_dataset
def _corpus(folder):
    from musicgan_amd.audio import wavio
    g = torch.Generator().manual_seed(11)
    folder.mkdir()
    pcm = ((torch.rand(5 * 44100, 2, generator=g) - 0.5) * 30000).to(torch.int16).numpy()
    with wave.open(str(folder / "a.wav"), "wb") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())
    wavio.save(str(folder / "b.wav"), torch.rand(1, 4 * 48000, generator=g) - 0.5, 48000)
    wavio.save(str(folder / "c.wav"), torch.rand(1, 44100, generator=g) - 0.5, 44100)
    return [(str(folder / "a.wav"), 5 * 44100, 44100), (str(folder / "b.wav"), 4 * 48000, 48000), (str(folder / "c.wav"), 44100, 44100)]


def _pts(d):
    return sorted((f for f in os.listdir(d) if f.endswith(".pt")), key=lambda f: int(f[len("magn_phase_"):-3]))


def test_create_dataset_with_variants(tmp_path, monkeypatch):
    import musicgan_amd
    from musicgan_amd import audio, ops, pv_ops
    from musicgan_amd.audio import wavio
    from musicgan_amd.create_dataset import check_variants, variant_counts
    import glob as _glob
    made = {f[0]: f for f in _corpus(tmp_path / "wav")}
    files = [made[p] for p in _glob.glob(str(tmp_path / "wav" / "*.wav"))]   # create_dataset numbers the files in glob order
    assert len(files) == 3
    short = [i for i, f in enumerate(files) if f[0].endswith("c.wav")][0]
    stretch, pitch = (Fraction(9, 10),), (1,)
    rates, ratios = check_variants(stretch, pitch)
    per_file = [variant_counts(ops.resample_len(n, sr, 44100) if sr != 44100 else n, 512, rates, ratios) for _, n, sr in files]
    total = sum(sum(c) for c in per_file)
    print(f"CREATE DATASET: samples per file and variant {per_file}")
    assert per_file[short] == [0, 0, 0] and all(c >= 1 for i, cs in enumerate(per_file) if i != short for c in cs)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    plain, full, sharded = tmp_path / "plain", tmp_path / "full", tmp_path / "sharded"
    glob = str(tmp_path / "wav" / "*.wav")
    musicgan_amd.create_dataset(glob, str(plain), resample=True)
    musicgan_amd.create_dataset(glob, str(full), resample=True, stretch=stretch, pitch=pitch)
    assert _pts(full) == [f"magn_phase_{i}.pt" for i in range(total)]
    assert _pts(plain) == [f"magn_phase_{i}.pt" for i in range(sum(c[0] for c in per_file))]
    idx = idx_plain = 0
    for (path, _, sr), counts in zip(files, per_file):
        # the original's samples: bit for bit the plain run's (the container names its file, so the tensors are compared)
        for _ in range(counts[0]):
            a, b = torch.load(str(full / f"magn_phase_{idx}.pt")), torch.load(str(plain / f"magn_phase_{idx_plain}.pt"))
            assert a.dtype == torch.float64 and tuple(a.shape) == (2, 512, 512) and torch.equal(a, b), (path, idx)
            idx, idx_plain = idx + 1, idx_plain + 1
        if not sum(counts):
            continue
        pcm = wavio.load_pcm_device(path, torch.device(DEV))
        X = audio.functions.stft_from_pcm(pcm, sample_rate=sr)
        mono = ops.pcm_to_mono(pcm) if sr == 44100 else ops.resample_pcm(pcm, sr, 44100)
        f = ratios[0][1]
        shifted = ops.stft_1024(ops.resample_rows(mono[None, :], f.numerator, f.denominator)[0].contiguous())
        for spec, count in ((pv_ops.phase_vocoder(X, 9, 10), counts[1]),
                            (pv_ops.phase_vocoder(shifted, f.denominator, f.numerator), counts[2])):
            want = audio.stft_to_stacked_phase_magn(spec).double().cpu()
            assert want.shape[0] == count
            for s in range(count):
                assert torch.equal(torch.load(str(full / f"magn_phase_{idx}.pt")), want[s]), (path, idx)
                idx += 1
    assert idx == total
    # two ranks into one directory: the same files
    for rank in (1, 0):
        monkeypatch.setenv("RANK", str(rank))
        monkeypatch.setenv("WORLD_SIZE", "2")
        monkeypatch.setenv("LOCAL_RANK", "0")
        musicgan_amd.create_dataset(glob, str(sharded), resample=True, stretch=stretch, pitch=pitch)
    assert _pts(sharded) == _pts(full)
    for n in _pts(full):
        assert torch.equal(torch.load(str(sharded / n)), torch.load(str(full / n))), n


# ---------------------------------------------------------------- 6. determinism and memory
def test_two_runs_and_a_replayed_graph_are_bit_identical():
    from musicgan_amd import audio
    X = R.tonal_spectrum(2 * _tile() + 3, 1000 + 2 * _tile() + 3).to(DEV)
    a = audio.phase_vocoder(X, Fraction(9, 10))
    b = audio.phase_vocoder(X, Fraction(9, 10))
    assert torch.equal(a, b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = audio.phase_vocoder(X, Fraction(9, 10))
    c.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, c)


def test_call_does_not_synchronise():
    from musicgan_amd import audio
    X = R.random_spectrum(130, 1130).to(DEV)
    audio.phase_vocoder(X, Fraction(53, 50))   # warm-up: library load, workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = audio.phase_vocoder(X, Fraction(53, 50))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(torch.view_as_real(out)).all())


def test_body_on_poisoned_memory():
    """under poison.rule pointed at pv_ops: no guard band damaged by any launch, no argument changed, the workspace poisoned again
    before every call, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import audio, pv_ops
    g = torch.Generator().manual_seed(6)
    wav = torch.rand(256 * 24 + 5, generator=g) - 0.5

    def run(p):
        p.a = audio.phase_vocoder(R.random_spectrum(37, 1037).to(DEV), Fraction(11, 10))
        p.b = audio.phase_vocoder(R.random_spectrum(1, 1001).to(DEV), Fraction(1, 2))
        p.c = audio.time_stretch(wav.to(DEV), Fraction(4, 5))
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=pv_ops, inplace={})
    for a, b in ((r0.a, r1.a), (r0.b, r1.b), (r0.c, r1.c)):
        assert torch.equal(a, b)
    names = [name for name, _, _ in r1.calls]
    assert names.count("phase_vocoder") == 3, names
    print(f"POISON phase vocoder: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")
