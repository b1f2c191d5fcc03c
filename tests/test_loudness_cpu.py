"""CPU: the host side of the loudness feature -- the K-weighting coefficients against the table of ITU-R BS.1770-4 and against the
numpy restatement, the restatement itself against EBU Tech 3341, the command line, the argument errors (raised before anything
touches a device) and the C ABI's new entries."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402


def test_coefficients_at_48k_are_the_table_of_bs1770():
    from musicgan_amd import audio
    (b1, a1), (b2, a2) = audio.kweighting_coefficients(48000)
    for got in (b1, a1, b2, a2):
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == (3,)
    assert np.max(np.abs(b1 - R.BS1770_SHELF_B)) <= 1e-12
    assert a1[0] == 1.0 and np.max(np.abs(a1[1:] - R.BS1770_SHELF_A)) <= 1e-12
    assert list(b2) == [1.0, -2.0, 1.0]
    assert a2[0] == 1.0 and np.max(np.abs(a2[1:] - R.BS1770_HIGHPASS_A)) <= 1e-12


@pytest.mark.parametrize("fs", [48000, 44100, 22050])
def test_coefficients_equal_the_restatement(fs):
    from musicgan_amd import audio
    for (b, a), (rb, ra) in zip(audio.kweighting_coefficients(fs), R.coefficients(fs)):
        assert np.max(np.abs(b - rb)) <= 1e-12 and np.max(np.abs(a - ra)) <= 1e-12


@pytest.mark.parametrize("case", sorted(R.TECH3341))
def test_restatement_meets_ebu_tech_3341(case):
    got = R.loudness(R.stereo_sine(48000, R.TECH3341[case]), 48000)["lufs"]
    print(f"Tech 3341 case {case}: {got:.3f} LUFS")
    assert abs(got - (-23.0)) <= 0.1, got


def test_restatement_reads_the_peak_between_the_samples():
    """a sine at fs / 4 whose samples all fall 45 degrees off its crests: the sample peak is 3.01 dB low, the interpolated one is
    not (the ends are faded over 500 samples: a sine that starts at once overshoots there, by 0.10 dB with this bank)"""
    x = R.quarter_rate_sine(4000)
    assert abs(R.db(np.abs(x).max()) - (-3.0103)) <= 1e-3
    assert abs(R.db(R.true_peak(x))) <= 0.1


def test_generate_flags_reach_generate_as_keywords(monkeypatch):
    from musicgan_amd import __main__ as cli
    import musicgan_amd
    assert callable(musicgan_amd.generate)                 # the package binds the name `generate` to the function ...
    G = sys.modules["musicgan_amd.generate"]               # ... and this is the module that the command line looks it up in
    calls = []
    monkeypatch.setattr(G, "generate", lambda *a, **k: calls.append((a, k)))
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-14", "--true-peak", "-1"])
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-23.5"])
    cli.main(["generate", "g.pt", "8", "-o", "out"])
    assert calls[0] == (("out", 8, "g.pt", 10, 5), {"loudness": -14.0, "peak_dbtp": -1.0})
    assert calls[1] == (("out", 8, "g.pt", 10, 5), {"loudness": -23.5})
    assert calls[2] == (("out", 8, "g.pt", 10, 5), {})


def test_loudness_subcommand_dispatches(monkeypatch):
    from musicgan_amd import __main__ as cli
    import importlib
    L = importlib.import_module("musicgan_amd.loudness")
    calls = []
    monkeypatch.setattr(L, "loudness", lambda *a, **k: calls.append((a, k)))
    cli.main(["loudness", "x/*.wav", "-o", "r.json"])
    cli.main(["loudness", "x/*.wav"])
    assert calls == [(("x/*.wav",), {"output": "r.json"}), (("x/*.wav",), {})]


def test_argument_errors_are_raised_before_the_device_is_touched():
    from musicgan_amd import audio
    x = torch.zeros(2, 100)
    with pytest.raises(ValueError, match="channels"):
        audio.loudness(torch.zeros(9, 100), 48000)
    with pytest.raises(ValueError, match="channels"):
        audio.true_peak(torch.zeros(9, 100))
    for rate in (0, -48000, 44100.0, True):
        with pytest.raises(ValueError, match="sample_rate"):
            audio.loudness(x, rate)
        with pytest.raises(ValueError, match="sample_rate"):
            audio.normalize_loudness(x, rate)
        with pytest.raises(ValueError, match="sample_rate"):
            audio.kweighting_coefficients(rate)
    ints = torch.zeros(2, 100, dtype=torch.int16)
    for call in (lambda: audio.loudness(ints, 48000), lambda: audio.true_peak(ints), lambda: audio.normalize_loudness(ints, 48000)):
        with pytest.raises(ValueError, match="floating-point"):
            call()
    with pytest.raises(ValueError, match="target_lufs"):
        audio.normalize_loudness(x, 48000, target_lufs=math.nan)
    with pytest.raises(ValueError, match="peak_dbtp"):
        audio.normalize_loudness(x, 48000, peak_dbtp=math.inf)
    with pytest.raises(ValueError, match="target_lufs"):
        audio.magn_phase_to_waveform(torch.zeros(1, 2, 512, 8), loudness=math.nan)
    with pytest.raises(ValueError, match="one weight per channel"):
        audio.loudness(x, 48000, channel_weights=(1.0, 1.0, 1.41))
    with pytest.raises(ValueError, match="not negative"):
        audio.loudness(x, 48000, channel_weights=(1.0, -1.0))
    with pytest.raises(ValueError, match="waveform"):
        audio.loudness(torch.zeros(1, 2, 100), 48000)
    with pytest.raises(ValueError, match="at least one sample"):
        audio.true_peak(torch.zeros(2, 0))


def test_generate_checks_its_targets_first(tmp_path):
    import musicgan_amd
    with pytest.raises(ValueError, match="target_lufs"):
        musicgan_amd.generate(str(tmp_path / "out"), 8, "missing.pt", 1, 1, loudness=math.nan)


def test_wrappers_refuse_cpu_tensors_loudly():
    from musicgan_amd import _lib, loud_ops
    x = torch.zeros(2, 100)
    with pytest.raises(_lib.MusicGanHipError):
        loud_ops.segment_energies(x, 48000)
    with pytest.raises(_lib.MusicGanHipError):
        loud_ops.true_peak(x)
    with pytest.raises(_lib.MusicGanHipError):
        loud_ops.gate(torch.zeros(2, 8, dtype=torch.float64), 48000)
    with pytest.raises(_lib.MusicGanHipError):
        loud_ops.normalize(x, torch.zeros(4, dtype=torch.float64), torch.ones(1), -14.0, -1.0)


def test_abi_has_the_loudness_entries():
    import test_abi
    from musicgan_amd import _lib, loud_ops
    test_abi.test_library_builds_loads_and_exports_every_declared_symbol()
    names = {"mg_loudness_chunk", "mg_loudness_ws_bytes", "mg_loudness_energy", "mg_loudness_gate", "mg_true_peak_ws_bytes",
             "mg_true_peak", "mg_loudness_normalize"}
    assert names <= set(test_abi.declared_symbols()) and names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.mg_loudness_chunk() == loud_ops.CHUNK
    # host-side size queries: 4 float64 per chunk, 1 per chunk and segment, per channel (+ 16 bytes of slack); 1 float per 2048 samples
    seg, length = 4800, 48000 * 2 + 17
    nseg = length // seg
    nch = -(-nseg * seg // loud_ops.CHUNK)
    assert lib.mg_loudness_ws_bytes(2, length, seg) == 2 * nch * 32 + 2 * (nch + nseg) * 8 + 16
    assert lib.mg_loudness_ws_bytes(9, length, seg) == 0 and lib.mg_loudness_ws_bytes(2, length, 0) == 0
    assert lib.mg_true_peak_ws_bytes(2, 2049) == 2 * 2 * 4 and lib.mg_true_peak_ws_bytes(2, 0) == 0
