"""CPU: the polyphase resampling bank the library builds on the host (mg_resample_bank) against a float64 restatement of
torchaudio.functional.resample's kernel in its full form, the output length, and the `--resample` flag of `create_dataset`.
`full_kernel` / `resample_f64` are the float64 reference the GPU tests (test_resample_gpu.py) compare against."""
import math
import sys

import numpy as np
import pytest

# (orig, new): the rates of common corpora into 44.1 kHz, and one upward pair out of it
PAIRS = [(48000, 44100), (96000, 44100), (22050, 44100), (32000, 44100), (16000, 44100), (8000, 44100), (88200, 44100),
         (192000, 44100), (44100, 48000)]


def full_kernel(orig: int, new: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """torchaudio's _get_sinc_resample_kernel (sinc_interp_hann) in float64: (o, n, w, h[n, 2w + o])."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    w = math.ceil(lowpass_filter_width * o / base)
    idx = np.arange(-w, w + o, dtype=np.float64)[None, :] / o
    t = np.arange(0, -n, -1, dtype=np.float64)[:, None] / n + idx
    t *= base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        h = np.where(t == 0, 1.0, np.sin(t) / t)
    return o, n, w, h * (window * (base / o))


def resample_f64(x: np.ndarray, orig: int, new: int) -> np.ndarray:
    """torchaudio.functional.resample(x, orig, new) in float64: (..., L) -> (..., ceil(n L / o))."""
    x = np.asarray(x, dtype=np.float64)
    if orig == new:
        return x
    o, n, w, h = full_kernel(orig, new)
    lead, length = x.shape[:-1], x.shape[-1]
    xp = np.pad(x.reshape(-1, length), ((0, 0), (w, w + o)))
    frames = np.lib.stride_tricks.sliding_window_view(xp, 2 * w + o, axis=1)[:, ::o]  # (rows, T, 2w + o)
    y = np.einsum("rtk,pk->rtp", frames, h).reshape(xp.shape[0], -1)
    return y[:, :-(-n * length // o)].reshape(*lead, -1)


@pytest.mark.parametrize("orig,new", PAIRS)
def test_bank_is_the_significant_part_of_torchaudios_kernel(orig, new):
    from musicgan_amd import ops
    o, n, w, h = full_kernel(orig, new)
    taps, start = ops.resample_bank_host(orig, new)
    taps, start = taps.numpy().astype(np.float64), start.numpy()
    assert taps.shape == (n, 2 * w + 1) and start.shape == (n,)
    # the compact window of phase p starts at floor(o p / n) of torchaudio's row
    assert np.array_equal(start, (o * np.arange(n)) // n)
    for p in range(n):
        inside = np.zeros(2 * w + o, dtype=bool)
        inside[start[p]:start[p] + 2 * w + 1] = True
        assert np.max(np.abs(taps[p] - h[p, inside])) <= 1e-7, p
        assert np.all(np.abs(h[p, ~inside]) <= 1e-30), p  # (o = 1: the window is the whole row)
        assert abs(taps[p].sum() - 1.0) <= 1e-3, p


def test_significant_taps_per_phase():
    """at most 2w + 1 taps of a row are above a rounding of zero; the counts of the rates the docs quote"""
    want = {48000: 14, 96000: 27, 32000: 13, 192000: 53}
    for orig, count in want.items():
        o, n, w, h = full_kernel(orig, 44100)
        sig = (np.abs(h) > 1e-30).sum(axis=1)
        assert sig.max() == count <= 2 * w + 1, orig


@pytest.mark.parametrize("orig,new", PAIRS + [(44100, 44100), (1, 3), (7, 5)])
def test_output_length(orig, new):
    from musicgan_amd import ops
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    for length in (0, 1, 7, 2 * o, o * n + 3, 10 * 60 * orig + 17, 2 ** 40 + 5):
        assert ops.resample_len(length, orig, new) == -(-n * length // o), length


def test_equal_rates_bank_is_one_unit_tap():
    from musicgan_amd import ops
    taps, start = ops.resample_bank_host(44100, 44100)
    assert taps.tolist() == [[1.0]] and start.tolist() == [0]


def test_bad_arguments_raise():
    from musicgan_amd import audio, ops
    import torch
    with pytest.raises(ValueError):
        ops.resample_bank_host(0, 44100)
    with pytest.raises(ValueError):
        ops.resample_bank_host(48000, 44100, lowpass_filter_width=0)
    with pytest.raises(ValueError):
        ops.resample_len(10, -1, 44100)
    x = torch.zeros(10)
    for bad in ((0, 44100), (48000, -44100), (48000.5, 44100), (48000, 44100.25)):
        with pytest.raises(ValueError):
            audio.resample(x, *bad)
    with pytest.raises(ValueError):
        audio.resample(x, 48000, 44100, resampling_method="sinc_interp_kaiser")
    with pytest.raises(ValueError):
        audio.resample(x, 48000, 44100, lowpass_filter_width=0)
    assert audio.resample(x, 48000, 48000) is x  # equal rates: the input itself, as torchaudio returns it


def test_float64_restatement_against_a_direct_sum():
    """resample_f64 (stride tricks) against the definition summed term by term, on a short signal"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal(301)
    o, n, w, h = full_kernel(48000, 44100)
    xp = np.concatenate([np.zeros(w), x, np.zeros(w + o)])
    want = [sum(xp[(m // n) * o + k] * h[m % n, k] for k in range(2 * w + o)) for m in range(-(-n * x.size // o))]
    assert np.allclose(resample_f64(x, 48000, 44100), want, rtol=0, atol=1e-12)


def test_cli_resample_flag_reaches_create_dataset(monkeypatch):
    from musicgan_amd.__main__ import main
    import musicgan_amd.create_dataset  # noqa: F401
    mod = sys.modules["musicgan_amd.create_dataset"]
    calls = []
    monkeypatch.setattr(mod, "create_dataset", lambda *a, **k: calls.append((a, k)))
    main(["create_dataset", "x/*.wav", "-o", "d", "--resample"])
    main(["create_dataset", "x/*.wav", "-o", "d"])
    assert calls == [(("x/*.wav", "d"), {"resample": True}), (("x/*.wav", "d"), {})]


def test_resample_kernels_do_not_use_scratch_memory():
    """every instantiation of resample_k keeps its taps and staged loads in registers (tests/test_build.py's rule)"""
    import re
    from musicgan_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_usage().items() if re.search(r"resample_k", k)}
    assert len(hits) >= 4
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)
