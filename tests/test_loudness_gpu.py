"""GPU: loudness and true peak (csrc/loudness.hip) against the float64 numpy restatement of tests/loudness_ref.py -- the K-weighted
segment energies around every boundary of the chunked filter state, the gates, true peak against the float64 evaluation of the same
bank, normalisation, and the way from a generated image to a file and back through the `loudness` sub-command.

Bounds.  Segment energies: 1e-9 relative per segment -- both sides are float64, a segment has at most 4 800 terms and the filter's
gain is below 1e3, so rounding stays near 1e-12; a dropped or mis-powered carry is off by parts in a thousand.  Integrated loudness:
1e-6 LU (the energies' error is ~4e-9 LU; the slack is for log10).  True peak: 1e-6 max|x|, what tests/test_resample_gpu.py grants
`resample_rows` against its float64 form, because it is the same sum."""
import functools
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _chunk():
    from musicgan_amd import loud_ops
    return loud_ops.CHUNK


@functools.lru_cache(maxsize=None)
def _noise(channels, length, seed):
    rng = np.random.default_rng(seed)
    x = (rng.random((channels, length), dtype=np.float32) - 0.5) * (0.1 + 0.8 * rng.random((channels, 1), dtype=np.float32))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _gate_case(name):
    parts = R.SHORT_GATES[name] if name in R.SHORT_GATES else R.TECH3341[name]
    x = R.stereo_sine(48000, parts)
    x.setflags(write=False)
    return x, R.segment_energies(x, 48000)


def _check_energies(x, fs, what):
    from musicgan_amd import loud_ops
    want = R.segment_energies(x, fs)
    got = loud_ops.segment_energies(torch.from_numpy(np.array(x)).to(DEV), fs)
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape, (what, tuple(got.shape), want.shape)
    if want.size == 0:
        return 0.0
    assert want.min() > 0, what
    err = float(np.max(np.abs(got.cpu().numpy() - want) / want))
    print(f"ENERGY {what}: {want.shape[1]} segments, worst relative error {err:.2e}")
    assert err <= 1e-9, (what, err)
    return err


LENGTHS_48K = ["chunk-1", "chunk", "chunk+1", "3chunk+17", "4seg",                  # below 100 ms there is no segment: S is empty
               "16seg-1", "16seg", "16seg+1", "5seg+chunk-1", "300chunk+5"]           # 16 seg = 75 chunks; 300 chunks: two per thread


def _length(name):
    c, seg = _chunk(), 4800
    return {"chunk-1": c - 1, "chunk": c, "chunk+1": c + 1, "3chunk+17": 3 * c + 17, "4seg": 4 * seg, "16seg-1": 16 * seg - 1,
            "16seg": 16 * seg, "16seg+1": 16 * seg + 1, "5seg+chunk-1": 5 * seg + c - 1, "300chunk+5": 300 * c + 5}[name]


@pytest.mark.parametrize("name", LENGTHS_48K)
def test_segment_energies_at_lengths_around_the_chunk(name):
    from musicgan_amd import audio
    length = _length(name)
    x = _noise(2, length, 7)
    _check_energies(x, 48000, name)
    want = R.loudness(x, 48000)
    got = audio.loudness(torch.from_numpy(np.array(x)).to(DEV), 48000, return_details=True)
    lufs, top, n_abs, n_rel = (float(v) for v in got)
    assert (int(n_abs), int(n_rel)) == (want["n_abs"], want["n_rel"])
    if length < 4 * 4800:
        assert lufs == -math.inf and top == -math.inf and n_abs == 0 and n_rel == 0
    else:
        assert abs(lufs - want["lufs"]) <= 1e-6 and abs(top - want["momentary_max"]) <= 1e-6


@pytest.mark.parametrize("fs", [8000, 10240, 96000])
def test_segment_energies_when_segments_are_shorter_than_equal_to_and_longer_than_a_chunk(fs):
    """seg = 800 (a chunk meets two or three segments), 1024 (every boundary is both a chunk's and a segment's), 9600"""
    _check_energies(_noise(2, 3 * fs + 77, fs), fs, f"{fs} Hz")


def test_slow_state_of_the_high_pass_stage_is_carried():
    """2 s of a 40 Hz sine: next to the high-pass corner the slow state carried over the chunk boundaries is most of the output"""
    t = np.arange(2 * 48000) / 48000.0
    x = (0.5 * np.sin(2 * np.pi * 40.0 * t)).astype(np.float32)[None, :]
    _check_energies(x, 48000, "40 Hz sine")


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_segment_energies_of_white_noise_at_44k1(channels):
    _check_energies(_noise(channels, 66163, 100 + channels), 44100, f"noise x{channels}")


def test_too_short_and_silent_signals_measure_minus_infinity():
    from musicgan_amd import audio
    for x in (torch.rand(2, 4 * 4800 - 1) - 0.5, torch.zeros(2, 48000), torch.zeros(1, 0), torch.rand(3)):
        got = [float(v) for v in audio.loudness(x.to(DEV), 48000, return_details=True)]
        assert got[0] == -math.inf and got[2] == 0 and got[3] == 0, got
    x = torch.rand(4 * 4800 - 1) - 0.5
    got = audio.loudness(x, 48000)                       # a CPU tensor is moved to the device
    assert got.is_cuda and got.dtype == torch.float64 and got.dim() == 0 and float(got) == -math.inf


@pytest.mark.parametrize("name", sorted(R.SHORT_GATES))
def test_gates_on_shortened_tech_3341_cases(name):
    from musicgan_amd import audio
    x, energies = _gate_case(name)
    want = R.gate(energies, 48000)
    assert len(want["l"]) == 37 and want["n_rel"] == 23 and abs(want["lufs"] - (-23.568)) <= 1e-3, want
    # no block within 1e-3 LU of either gate: a flipped decision cannot hide in the tolerance
    finite = want["l"][np.isfinite(want["l"])]
    assert np.abs(finite - (-70.0)).min() > 1e-3 and np.abs(finite - want["gamma"]).min() > 1e-3
    lufs, top, n_abs, n_rel = (float(v) for v in audio.loudness(torch.from_numpy(np.array(x)).to(DEV), 48000,
                                                                 return_details=True))
    print(f"GATES {name}: {lufs:.9f} LUFS (reference {want['lufs']:.9f}), blocks {n_abs:.0f} / {n_rel:.0f}")
    assert (n_abs, n_rel) == (want["n_abs"], want["n_rel"])
    assert abs(lufs - want["lufs"]) <= 1e-6 and abs(top - want["momentary_max"]) <= 1e-6


def test_tech_3341_case_3_in_full():
    """80 s: 3750 chunks per channel, fifteen to a thread of the carry -- every level of it is at work"""
    from musicgan_amd import audio
    x, energies = _gate_case(3)
    want = R.gate(energies, 48000)
    _check_energies(x, 48000, "Tech 3341 case 3")
    got = float(audio.loudness(torch.from_numpy(np.array(x)).to(DEV), 48000))
    print(f"TECH3341 case 3: {got:.9f} LUFS (reference {want['lufs']:.9f})")
    assert abs(got - want["lufs"]) <= 1e-6 and abs(got - (-23.0)) <= 0.1


def test_channel_weights_of_a_surround_layout():
    from musicgan_amd import audio
    x, w = _noise(5, 48000 + 321, 55), (1.0, 1.0, 1.0, 1.41, 1.41)
    want = R.loudness(x, 48000, w)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    got = float(audio.loudness(xd, 48000, channel_weights=w))
    assert abs(got - want["lufs"]) <= 1e-6, (got, want["lufs"])
    assert abs(float(audio.loudness(xd, 48000)) - R.loudness(x, 48000)["lufs"]) <= 1e-6
    assert abs(got - float(audio.loudness(xd, 48000))) > 1e-3   # the weights matter


def test_runs_are_bit_identical_and_strides_do_not_matter():
    from musicgan_amd import audio, loud_ops
    x = torch.from_numpy(np.array(_noise(2, 300 * _chunk() + 5, 7))).to(DEV)
    a, b = loud_ops.segment_energies(x, 48000), loud_ops.segment_energies(x, 48000)
    assert torch.equal(a, b)
    ra, rb = audio.loudness(x, 48000, return_details=True), audio.loudness(x, 48000, return_details=True)
    assert all(torch.equal(u, v) for u, v in zip(ra, rb))
    assert torch.equal(audio.true_peak(x), audio.true_peak(x))
    wide = torch.zeros(2, x.shape[1] + 100, device=DEV)
    wide[:, 50:-50] = x
    rows = wide[:, 50:-50]                               # a row stride that is not the length
    frames = x.t().contiguous().t()                      # channels interleaved in memory
    for view in (rows, frames):
        assert not view.is_contiguous()
        assert torch.equal(audio.loudness(view, 48000), ra[0]) and torch.equal(audio.true_peak(view), audio.true_peak(x))
        assert torch.equal(audio.normalize_loudness(view, 48000), audio.normalize_loudness(x, 48000))


def _peak_inputs():
    rng = np.random.default_rng(3)
    first, last = np.zeros((1, 5000), np.float32), np.zeros((1, 5000), np.float32)
    first[0, 0], last[0, -1] = 0.75, -0.75
    sample = (rng.random((1, 4097), dtype=np.float32) - 0.5) * 0.01
    sample[0, 2048] = 0.9                                 # the first sample of the second tile
    two = (rng.random((2, 3000), dtype=np.float32) - 0.5) * 0.2
    two[1, 1500:1504] = (0.6, 0.7, 0.7, 0.6)
    return {"impulse at 0": first, "impulse at L-1": last, "one sample": np.full((1, 1), -0.3, np.float32),
            "sine at fs/4": R.quarter_rate_sine(4000).astype(np.float32)[None, :], "an original sample": sample,
            "peak in the second channel": two, "noise": (rng.random((2, 2 * 2048 + 7), dtype=np.float32) - 0.5)}


@pytest.mark.parametrize("name", ["impulse at 0", "impulse at L-1", "one sample", "sine at fs/4", "an original sample",
                                  "peak in the second channel", "noise"])
def test_true_peak_against_the_float64_bank(name):
    from musicgan_amd import audio
    x = _peak_inputs()[name]
    xd = torch.from_numpy(x).to(DEV)
    got = audio.true_peak(xd if name != "one sample" else xd[0])
    assert got.is_cuda and got.dtype == torch.float32 and got.dim() == 0
    want, top = R.true_peak(x), float(np.abs(x).max())
    print(f"TRUE PEAK {name}: {float(got):.9f} (float64 {want:.9f}, sample peak {top:.9f})")
    assert abs(float(got) - want) <= 1e-6 * top, (name, float(got), want)
    # the same sums in the same order as the resampler: the largest of its outputs and of the samples, bit for bit
    assert torch.equal(got, torch.maximum(xd.abs().max(), audio.resample(xd, 1, 4).abs().max()))
    if name == "sine at fs/4":
        assert abs(R.db(top) - (-3.0103)) <= 1e-3 and abs(R.db(float(got))) <= 0.1
    if name in ("impulse at 0", "impulse at L-1", "one sample", "an original sample"):
        assert float(got) == top
    if name == "peak in the second channel":
        assert float(got) > top and float(audio.true_peak(xd[0])) < 0.5 * float(got) and torch.equal(audio.true_peak(xd[1]), got)


def test_normalisation_reaches_the_target_or_the_ceiling():
    from musicgan_amd import audio
    x = torch.from_numpy(np.array(_noise(2, 48000 + 321, 9))).to(DEV)
    out, gain = audio.normalize_loudness(x, 48000, target_lufs=-23.0, peak_dbtp=-1.0, return_gain=True)
    assert gain.is_cuda and gain.dtype == torch.float32 and gain.dim() == 0 and out.dtype == torch.float32 and out.shape == x.shape
    assert torch.equal(out, x * gain)
    got = float(audio.loudness(out, 48000))
    print(f"NORMALISE noise: gain {float(gain):.6f}, {got:.6f} LUFS, peak {R.db(float(audio.true_peak(out))):.3f} dBTP")
    assert abs(got - (-23.0)) <= 1e-4 and float(audio.true_peak(out)) < 10 ** (-1.0 / 20)          # the ceiling does not bind
    assert abs(float(gain) - 10 ** ((-23.0 - float(audio.loudness(x, 48000))) / 20)) <= 1e-6 * float(gain)
    # sparse impulses: all crest and no loudness, the ceiling binds
    y = torch.zeros(2, 48000, device=DEV)
    y[0, 1000::7919], y[1, 3000::6007] = 0.05, -0.04
    out, gain = audio.normalize_loudness(y, 48000, target_lufs=-14.0, peak_dbtp=-3.0, return_gain=True)
    assert torch.equal(out, y * gain)
    ceiling = 10 ** (-3.0 / 20)
    peak, lufs = float(audio.true_peak(out)), float(audio.loudness(out, 48000))
    print(f"NORMALISE impulses: gain {float(gain):.6f}, {lufs:.3f} LUFS, peak {peak:.9f} (ceiling {ceiling:.9f})")
    # two float32 roundings (the gain, the product) and the 1e-6 of the bank's float32 sum
    assert peak <= ceiling * (1 + 1e-6 + 2.0 ** -22) and peak >= ceiling * (1 - 1e-6 - 2.0 ** -22) and lufs < -14.0 - 1.0
    # silence and signals too short to measure come back unchanged
    for z in (torch.zeros(2, 48000, device=DEV), torch.rand(1000, device=DEV) - 0.5):
        out, gain = audio.normalize_loudness(z, 48000, return_gain=True)
        assert float(gain) == 1.0 and torch.equal(out, z) and out.shape == z.shape


def test_from_an_image_to_a_file_and_back(tmp_path, capsys):
    """Four blocks need 700 ms: the image is (1, 2, 512, 128), 32 512 samples (a (1, 2, 512, 8) image gives 40 ms, which has no
    loudness -- it comes back with the gain 1, byte for byte).  The waveform of a random image is all crest: at -14 LUFS its true
    peak would be +1.0 dBTP, so under the default ceiling of -1 dBTP the file lands on the ceiling at -16.0 LUFS (measured on an
    MI355X); the target itself is checked with the ceiling raised to +3 dBTP, which a float32 WAV holds."""
    from musicgan_amd import audio
    from musicgan_amd.__main__ import main
    from musicgan_amd.audio import wavio
    g = torch.Generator().manual_seed(12)
    for width in (8, 128):
        img = (torch.rand(1, 2, 512, width, generator=g) * 2 - 1).to(DEV)
        plain, none, loud, capped = (str(tmp_path / f"{n}{width}.wav") for n in ("plain", "none", "loud", "capped"))
        audio.magn_phase_to_wav(img, plain, 44100)
        audio.magn_phase_to_wav(img, none, 44100, loudness=None)
        audio.magn_phase_to_wav(img, loud, 44100, loudness=-14, peak_dbtp=3.0)
        audio.magn_phase_to_wav(img, capped, 44100, loudness=-14)
        assert open(plain, "rb").read() == open(none, "rb").read()
        assert torch.equal(audio.magn_phase_to_waveform(img), audio.magn_phase_to_waveform(img, loudness=None, peak_dbtp=-1.0))
        if width == 8:
            assert open(plain, "rb").read() == open(loud, "rb").read()
    wav, sr = wavio.load(loud)
    assert sr == 44100 and tuple(wav.shape) == (1, 256 * 127)
    lufs, peak = float(audio.loudness(wav, sr)), float(audio.true_peak(wav))
    print(f"FILE: {lufs:.6f} LUFS, {R.db(peak):.3f} dBTP; before: {float(audio.loudness(wavio.load(plain)[0], sr)):.3f} LUFS")
    assert abs(lufs - (-14.0)) <= 1e-3 and R.db(peak) <= 3.0
    wav_c, _ = wavio.load(capped)
    lufs_c, peak_c = float(audio.loudness(wav_c, sr)), float(audio.true_peak(wav_c))
    print(f"FILE under the default ceiling: {lufs_c:.6f} LUFS, {R.db(peak_c):.6f} dBTP")
    assert lufs_c < -14.0 and abs(peak_c / 10 ** (-1.0 / 20) - 1) <= 1e-6 + 2.0 ** -22   # on the ceiling, as in the test above
    ref = R.loudness(wav.numpy(), sr)
    assert abs(lufs - ref["lufs"]) <= 1e-6 and abs(peak - R.true_peak(wav.numpy())) <= 1e-6 * float(wav.abs().max())
    # the sub-command prints and writes the same numbers
    capsys.readouterr()
    out_json = str(tmp_path / "r.json")
    main(["loudness", str(tmp_path / "*128.wav"), "-o", out_json])
    printed = capsys.readouterr().out
    rows = json.load(open(out_json))
    assert [os.path.basename(r["path"]) for r in rows] == ["capped128.wav", "loud128.wav", "none128.wav", "plain128.wav"]
    rows = rows[1:]
    assert rows[0]["integrated_lufs"] == lufs and rows[0]["true_peak_dbtp"] == 20.0 * math.log10(peak)
    assert rows[0]["sample_rate"] == 44100 and rows[0]["channels"] == 1 and rows[1] == {**rows[2], "path": rows[1]["path"]}
    line = [ln for ln in printed.splitlines() if ln.endswith("loud128.wav")][0].split()
    assert [float(v) for v in line[:3]] == [round(rows[0][k], 3) for k in ("integrated_lufs", "momentary_max_lufs", "true_peak_dbtp")]


def test_body_on_poisoned_memory():
    """under poison.rule pointed at loud_ops: no guard band damaged by any launch, no argument changed, the workspace poisoned again
    before every call, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import audio, loud_ops
    x = torch.from_numpy(np.array(_noise(2, 5 * 4800 + _chunk() - 1, 7)))
    y = torch.from_numpy(_peak_inputs()["noise"])

    def run(p):
        p.a = audio.loudness(x.to(DEV), 48000, return_details=True)
        p.b = audio.true_peak(y.to(DEV))
        p.c = audio.normalize_loudness(x.to(DEV), 48000, return_gain=True)
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=loud_ops, inplace={})
    for a, b in zip(r0.a + (r0.b,) + r0.c, r1.a + (r1.b,) + r1.c):
        assert torch.equal(a, b)
    names = [name for name, _, _ in r1.calls]
    assert {"segment_energies", "gate", "true_peak", "normalize"} <= set(names), names
    print(f"POISON loudness: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")
