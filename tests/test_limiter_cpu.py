"""CPU: the host side of the limiter -- the numpy restatement's own properties (tests/limiter_ref.py), the argument errors (raised
before anything touches a device), the command line and the C ABI's new entries."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as LR  # noqa: E402


def _spiky(length, seed, spikes=12):
    rng = np.random.default_rng(seed)
    x = 0.1 * rng.standard_normal((2, length))
    x[rng.integers(0, 2, spikes), rng.integers(0, length, spikes)] += 2.0 * rng.standard_normal(spikes)
    return x.astype(np.float32)


@pytest.mark.parametrize("A", [0, 1, 37, 220])
def test_reference_properties_on_seeded_inputs(A):
    """g <= r, q <= h (to one rounding), |y| <= c (1 + 2^-23), and the start-of-file rule: the file behaves as if A silent samples came before it"""
    from musicgan_amd import lim_ops
    assert lim_ops.TILE == 2048
    x, c, rho, G = _spiky(1500, 10 + A), 10 ** (-1 / 20), math.exp(-1 / 300.0), 1.7
    m = LR.envelope(x)
    cur = LR.gain_curve(m, G, c, A, rho)
    assert cur["h"].shape == cur["q"].shape == (1500 + A,) and cur["g"].shape == cur["r"].shape == (1500,)
    assert (cur["r"] < 1).sum() >= 5 and np.all(cur["g"] <= cur["r"]) and np.all(cur["g"] > 0)
    # the k = 0 term of the release enters by selection: d >= 1 - h exactly, and q = 1 - d <= h up to the one rounding of 1 - h
    # (below h = 1/2 the difference 1 - h is not exact; 1 - d is, for d in [1/2, 1])
    assert np.all(cur["d"] >= 1.0 - cur["h"]) and np.all(cur["q"] <= cur["h"] + 2.0 ** -54)
    y, g = LR.limit(x, G, c, A, rho)
    assert np.abs(y).max() <= c * (1 + 2.0 ** -23) and np.abs(x * G).max() > 2 * c
    # the same file with A samples of silence written in front of it, limited with a rule that starts at its first sample
    # (d = 0 before it, nothing dropped): the outputs after the silence are the file's
    padded = np.concatenate([np.zeros(A), m])
    r = LR.required_gain(padded, G, c)
    ext = np.concatenate([r, np.ones(A)])
    h = np.lib.stride_tricks.sliding_window_view(ext, A + 1).min(axis=1)
    d, state = np.empty(h.shape[0]), 0.0
    for i, u in enumerate(1.0 - h):
        state = max(u, rho * state)
        d[i] = state
    q = 1.0 - d
    mean = np.array([q[max(0, i - A):i + 1].sum() / (A + 1) for i in range(A, A + 1500)])
    assert np.max(np.abs(np.minimum(r[A:], mean) - g)) <= 1e-14       # the two sums add in different orders
    # a spike at sample 0 is met by a gain that has already fallen: the look-ahead reaches back before the file
    spike = np.zeros((1, 400), np.float32)
    spike[0, 0] = 4.0
    _, g0 = LR.limit(spike, 1.0, c, A, rho)
    assert g0[0] <= c / 4.0 * (1 + 1e-12)


def test_reference_passes_through_below_the_ceiling():
    x = _spiky(900, 3)
    G = 0.5 * 10 ** (-1 / 20) / LR.envelope(x).max()
    y, g = LR.limit(x, G, 10 ** (-1 / 20), 220, math.exp(-1 / 2205.0))
    assert np.all(g == 1.0) and np.array_equal(y, (x.astype(np.float64) * G).astype(np.float32))
    y, g = LR.limit(np.zeros((2, 50), np.float32), 3.0, 0.5, 7, 0.9)
    assert np.all(g == 1.0) and not y.any()


@pytest.mark.parametrize("rho", [math.exp(-1 / 2205.0), math.exp(-1 / 44.1), 0.5])
def test_closed_form_of_the_release_equals_the_recurrence(rho):
    x = _spiky(3000, 21)
    cur = LR.gain_curve(LR.envelope(x), 2.0, 0.8, 64, rho)
    closed = LR.release_closed_form(cur["h"], rho, cur["h"].shape[0] - 1)
    assert np.max(np.abs((1.0 - closed) - cur["q"])) <= 1e-12


def test_reference_envelope_counts_both_sides_of_a_sample():
    """an impulse: the interpolated points 4n - 3 .. 4n + 3 belong to sample n, so its two neighbours see the bank's side lobes"""
    x = np.zeros((1, 64), np.float32)
    x[0, 30] = 1.0
    m, u = LR.envelope(x), np.abs(LR.interpolate4(x))[0]
    assert m[30] == 1.0 and m[29] == u[4 * 29 - 3:4 * 29 + 4].max() and m[31] == u[4 * 31 - 3:4 * 31 + 4].max()
    assert m[29] == u[119] and m[31] == u[121] and 0.8 < m[29] < 1.0   # the points next to the impulse: 4 * 30 -+ 1
    assert LR.envelope(np.stack([x[0] * 0.5, np.roll(x[0], 5)]))[35] == 1.0          # the maximum over the channels


def test_argument_errors_are_raised_before_the_device_is_touched(tmp_path):
    import musicgan_amd
    from musicgan_amd import audio
    x = torch.zeros(2, 100)
    for kw in ({"attack_ms": -1.0}, {"attack_ms": 60.0}, {"attack_ms": math.nan}, {"release_ms": 0.0}, {"release_ms": -5.0},
               {"ceiling_dbtp": math.inf}, {"gain_db": math.nan}, {"attack_ms": "5"}):
        with pytest.raises(ValueError):
            audio.limit(x, 44100, **kw)
    with pytest.raises(ValueError, match="sample_rate"):
        audio.limit(x, 44100.0)
    with pytest.raises(ValueError, match="channels"):
        audio.limit(torch.zeros(9, 100), 44100)
    with pytest.raises(ValueError, match="floating-point"):
        audio.limit(torch.zeros(2, 100, dtype=torch.int16), 44100)
    with pytest.raises(ValueError, match="waveform"):
        audio.limit(torch.zeros(1, 2, 100), 44100)
    for passes in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="passes"):
            audio.normalize_loudness(x, 44100, limiter=True, passes=passes)
    with pytest.raises(ValueError, match="attack_ms"):
        audio.normalize_loudness(x, 44100, limiter=True, attack_ms=100.0)
    with pytest.raises(ValueError, match="limiter needs loudness"):
        audio.magn_phase_to_waveform(torch.zeros(1, 2, 512, 8), limiter=True)
    with pytest.raises(ValueError, match="limiter needs loudness"):
        audio.magn_phase_to_wav(torch.zeros(1, 2, 512, 8), str(tmp_path / "x.wav"), 44100, limiter=True)
    with pytest.raises(ValueError, match="attack_ms"):
        audio.magn_phase_to_waveform(torch.zeros(1, 2, 512, 8), loudness=-14, limiter=True, attack_ms=-2.0)
    with pytest.raises(ValueError, match="limiter needs loudness"):
        musicgan_amd.generate(str(tmp_path / "out"), 8, "missing.pt", 1, 1, limiter=True)
    with pytest.raises(ValueError, match="release_ms"):
        musicgan_amd.generate(str(tmp_path / "out"), 8, "missing.pt", 1, 1, loudness=-14, limiter=True, limiter_release=0.0)
    assert not (tmp_path / "out").exists()


def test_defaults_are_five_and_fifty_milliseconds():
    from musicgan_amd import lim_ops
    c, A, rho = lim_ops.check_arguments(44100)
    assert (c, A, rho) == (10 ** (-1 / 20), 220, math.exp(-1 / 2205.0))
    assert (c, A) == LR.parameters(44100)[:2] and abs(rho - LR.parameters(44100)[2]) <= 2.0 ** -52   # two libraries' exp
    assert lim_ops.check_arguments(48000, -3.0, 0.0, 1.0) == (10 ** (-3 / 20), 0, math.exp(-1 / 48.0))
    assert lim_ops.check_arguments(44100, attack_ms=2047 / 44.1)[1] == lim_ops.MAX_LOOKAHEAD


def test_wrappers_refuse_cpu_tensors_loudly():
    from musicgan_amd import _lib, lim_ops
    x, one = torch.zeros(2, 100), torch.ones(1, dtype=torch.float64)
    with pytest.raises(_lib.MusicGanHipError):
        lim_ops.envelope(x)
    with pytest.raises(_lib.MusicGanHipError):
        lim_ops.limit(x, one, 0.9, 220, 0.999)
    with pytest.raises(_lib.MusicGanHipError):
        lim_ops.trim(x, torch.ones(1), 0.9)
    with pytest.raises(_lib.MusicGanHipError):
        lim_ops.pregain(torch.zeros(4, dtype=torch.float64), -14.0)


def test_generate_flags_reach_generate_as_keywords(monkeypatch):
    from musicgan_amd import __main__ as cli
    import musicgan_amd  # noqa: F401
    G = sys.modules["musicgan_amd.generate"]
    calls = []
    monkeypatch.setattr(G, "generate", lambda *a, **k: calls.append((a, k)))
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-14", "--limiter", "--limiter-attack", "2.5"])
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-14", "--limiter", "--limiter-release", "20"])
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-14", "--limiter"])
    cli.main(["generate", "g.pt", "8", "-o", "out", "--loudness", "-14"])
    assert calls[0] == (("out", 8, "g.pt", 10, 5), {"loudness": -14.0, "limiter": True, "limiter_attack": 2.5})
    assert calls[1] == (("out", 8, "g.pt", 10, 5), {"loudness": -14.0, "limiter": True, "limiter_release": 20.0})
    assert calls[2] == (("out", 8, "g.pt", 10, 5), {"loudness": -14.0, "limiter": True})
    assert calls[3] == (("out", 8, "g.pt", 10, 5), {"loudness": -14.0})
    for bad in (["--limiter"], ["--limiter-attack", "2"], ["--true-peak", "-1", "--limiter"]):
        with pytest.raises(SystemExit):
            cli.main(["generate", "g.pt", "8", "-o", "out", *bad])
    assert len(calls) == 4


def test_abi_has_the_limiter_entries():
    import test_abi
    from musicgan_amd import _lib, lim_ops
    test_abi.test_library_builds_loads_and_exports_every_declared_symbol()
    names = {"mg_limiter_tile", "mg_limiter_ws_bytes", "mg_limiter_envelope", "mg_limiter", "mg_limiter_trim", "mg_limiter_pregain"}
    assert names <= set(test_abi.declared_symbols()) and names <= set(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.mg_limiter_tile() == lim_ops.TILE
    # host-side size query: a float32 per sample, a float64 per tile of L + A positions and per position, each rounded up to 16 bytes
    up = lambda n: -(-n // 16) * 16
    length, A = 3 * lim_ops.TILE + 17, 220
    tiles = -(-(length + A) // lim_ops.TILE)
    assert lib.mg_limiter_ws_bytes(2, length, A) == up(4 * length) + up(8 * tiles) + 8 * (length + A) + 16
    assert lib.mg_limiter_ws_bytes(9, length, A) == 0 and lib.mg_limiter_ws_bytes(2, length, lim_ops.MAX_LOOKAHEAD + 1) == 0
    assert lib.mg_limiter_ws_bytes(2, length, -1) == 0 and lib.mg_limiter_ws_bytes(1, 0, 0) == 16
