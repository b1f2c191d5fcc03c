"""CPU: the phase-locked vocoder's definition (tests/phasevocoder_lock_ref.py) -- the peak / region rule on hand-made frames, rate 1,
the composed maps against the sequential run, the audible claim -- and the argument checks and command line of `phase_lock`."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phasevocoder_lock_ref as L  # noqa: E402
import phasevocoder_ref as R  # noqa: E402


def _frame(values: dict) -> np.ndarray:
    mag = np.zeros(512)
    for k, v in values.items():
        mag[k] = v
    return mag


# ---------------------------------------------------------------- 1. peaks and regions
def test_a_plateau_has_one_peak_its_lowest_bin():
    mag = _frame({98: 1.0, 99: 2.0, 100: 3.0, 101: 3.0, 102: 3.0, 103: 2.0})
    assert list(np.flatnonzero(L.peaks(mag))) == [100]
    assert (L.regions(L.peaks(mag)) == 100).all()
    # two bins apart the plateau's upper end is still no peak (the rule looks two bins down), three bins apart it is one
    assert list(np.flatnonzero(L.peaks(_frame({100: 3.0, 101: 1.0, 102: 3.0})))) == [100]
    assert list(np.flatnonzero(L.peaks(_frame({100: 3.0, 101: 1.0, 102: 1.0, 103: 3.0})))) == [100, 103]


def test_peaks_at_the_first_and_the_last_bin():
    mag = _frame({0: 2.0, 1: 1.0, 510: 1.0, 511: 2.0})
    assert list(np.flatnonzero(L.peaks(mag))) == [0, 511]
    P = L.regions(L.peaks(mag))
    assert (P[:256] == 0).all() and (P[256:] == 511).all()     # 255: 255 against 256 bins away; 256: 256 against 255
    # below the first peak and above the last one
    P = L.regions(L.peaks(_frame({200: 1.0, 300: 1.0})))
    assert (P[:251] == 200).all() and (P[251:] == 300).all()


def test_a_tie_between_two_peaks_goes_to_the_lower():
    P = L.regions(L.peaks(_frame({10: 1.0, 20: 5.0})))
    assert P[15] == 10 and P[14] == 10 and P[16] == 20
    P = L.regions(L.peaks(_frame({10: 5.0, 13: 5.0})))        # equal heights, three bins apart: two peaks
    assert list(P[10:14]) == [10, 10, 13, 13]


def test_a_frame_of_zeros_has_no_peak_and_keeps_every_bin():
    assert not L.peaks(np.zeros(512)).any()
    assert (L.regions(L.peaks(np.zeros(512))) == np.arange(512)).all()


# ---------------------------------------------------------------- 2. rate 1
@pytest.mark.parametrize("kind", ["random", "tonal", "silence"])
def test_rate_one_reproduces_the_input(kind):
    X = R.MAKERS[kind](130, 1130)
    ref = L.mixed_locked(X, 1, 1).out
    err = float(np.abs(ref - X.numpy().astype(np.complex128)).max())
    print(f"LOCKED IDENTITY {kind}: err {err:.3e}, max|X| {float(X.abs().max()):.3f}")
    assert ref.shape == tuple(X.shape) and err <= 1e-6 * float(X.abs().max())


# ---------------------------------------------------------------- 3. composed maps
@pytest.mark.parametrize("kind", ["random", "quantised", "zero"])
@pytest.mark.parametrize("rate", [(9, 10), (3, 1), (1, 3)])
def test_composed_maps_match_the_sequential_run(kind, rate):
    """tolerance: L.state_bound -- (n sequential + n + tiles composed additions) x ulp(max|s|), see its docstring; m4 is equal"""
    from musicgan_amd import pv_ops
    p, q = rate
    n = 2 * pv_ops.LOCK_TILE + 37
    X = L.MAKERS[kind](L.frames_for(n, p, q), 77)
    ref = L.mixed_locked(X, p, q)
    s_max = float(np.abs(ref.s).max())
    for tile in (16, pv_ops.LOCK_TILE):
        S, M4 = L.composed(ref.P, ref.c, tile)
        err, tol = float(np.abs(S - ref.s).max()), L.state_bound(ref.s.shape[0], tile, max(s_max, 1.0))
        print(f"COMPOSED {kind} {p}/{q} tile {tile}: n {ref.s.shape[0]}, err {err:.3e}, tol {tol:.3e}, max|s| {s_max:.1f}")
        assert err <= tol and (M4 == ref.m4).all()


# ---------------------------------------------------------------- 4. what it is for
@pytest.mark.parametrize("rate", [(3, 4), (11, 10)])
def test_locking_takes_the_warble_out_of_a_glide(rate):
    wav = L.glide()
    own = L.ripple(wav)
    locked, unlocked = L.ripple(L.stretch_locked(wav, *rate)), L.ripple(L.stretch_unlocked(wav, *rate))
    print(f"RIPPLE {rate[0]}/{rate[1]}: input {own:.4f}, locked {locked:.4f}, unlocked {unlocked:.4f} ({unlocked / locked:.1f} x)")
    assert locked <= 2 * own
    assert unlocked >= 10 * locked


# ---------------------------------------------------------------- 5. arguments and the command line
def test_command_line():
    from musicgan_amd.__main__ import _MODES, build_parser
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"]
    kwargs = _MODES["create_dataset"][4]
    base = ["create_dataset", "in/*.wav", "-o", "out"]
    a = build_parser().parse_args(base)
    assert a.phase_lock is False and "phase_lock" not in kwargs(a)
    a = build_parser().parse_args(base + ["--stretch", "9/10"])
    assert kwargs(a) == {"stretch": (Fraction(9, 10),)}
    a = build_parser().parse_args(base + ["--stretch", "9/10", "--phase-lock"])
    assert kwargs(a) == {"stretch": (Fraction(9, 10),), "phase_lock": True}
    a = build_parser().parse_args(base + ["--pitch", "-1,1", "--phase-lock", "--preserve-transients", "--component", "harmonic"])
    assert kwargs(a) == {"pitch": (Fraction(-1), Fraction(1)), "phase_lock": True, "preserve_transients": True, "component": "harmonic"}


def test_create_dataset_refuses_phase_lock_without_a_variant():
    from musicgan_amd.create_dataset import check_phase_lock, create_dataset
    for kw in (dict(phase_lock=True), dict(phase_lock=True, component="harmonic"), dict(phase_lock=1, stretch=(2,))):
        with pytest.raises(ValueError):   # before the glob, the output directory or the device
            create_dataset("/nonexistent/*.wav", "/nonexistent/out", **kw)
    with pytest.raises(ValueError):
        check_phase_lock(True)
    check_phase_lock(True, rates=(Fraction(9, 10),))
    check_phase_lock(True, ratios=((1, Fraction(53, 50)),))
    check_phase_lock(False)


def test_a_lock_that_is_no_bool_raises_before_any_device_call(monkeypatch):
    import inspect
    from musicgan_amd import _lib, audio, pv_ops

    def no_device(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "load", no_device)
    X = R.random_spectrum(8, 1008)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            pv_ops.phase_vocoder(X, 9, 10, lock=bad)
        with pytest.raises(ValueError):
            audio.phase_vocoder(X, Fraction(9, 10), phase_lock=bad)
        with pytest.raises(ValueError):
            audio.time_stretch(torch.zeros(4096), Fraction(9, 10), phase_lock=bad)
        with pytest.raises(ValueError):
            audio.pitch_shift(torch.zeros(4096), 1, phase_lock=bad)
        with pytest.raises(ValueError):
            audio.functions.retime_preserving_transients(X, Fraction(9, 10), phase_lock=bad)
    monkeypatch.undo()
    with pytest.raises(_lib.MusicGanHipError):   # the arguments are fine: no device, and no CPU path
        pv_ops.phase_vocoder(X, 9, 10, lock=True)
    assert inspect.signature(pv_ops.phase_vocoder).parameters["lock"].default is False
    for f in (audio.phase_vocoder, audio.time_stretch, audio.pitch_shift, audio.functions.retime_preserving_transients):
        assert inspect.signature(f).parameters["phase_lock"].default is False
    assert pv_ops.LOCK_TILE >= 16


def test_the_library_sizes_and_refuses_like_the_unlocked_entry():
    import ctypes
    from musicgan_amd import _build, _lib, pv_ops
    _build.build()
    lib = _lib.load()
    tile = pv_ops.LOCK_TILE
    for frames, p, q in ((1, 1, 1), (231, 9, 10), (103360, 9, 10), (64, 8, 1)):
        n = int(lib.mg_phase_vocoder_len(frames, p, q))
        want = 8 * 512 * frames + 18 * 512 * n + 20 * 512 * -(-n // tile)
        assert int(lib.mg_phase_vocoder_locked_ws_bytes(frames, p, q)) == want, (frames, p, q)
    ptr = ctypes.c_void_p(4096)    # never dereferenced: every call below is refused on its arguments
    for frames, p, q in ((0, 1, 1), (8, 0, 1), (8, 1, 0), (8, 9, 1), (8, 1, 9), (2 ** 31, 1, 1)):
        assert int(lib.mg_phase_vocoder_locked_ws_bytes(frames, p, q)) == int(lib.mg_phase_vocoder_ws_bytes(frames, p, q)) == 0
        assert lib.mg_phase_vocoder_locked(ptr, ptr, ptr, 1 << 40, frames, p, q, None) == lib.mg_phase_vocoder(
            ptr, ptr, ptr, 1 << 40, frames, p, q, None) != 0, (frames, p, q)
    assert lib.mg_phase_vocoder_locked(None, ptr, ptr, 1 << 40, 8, 1, 1, None) != 0
    assert lib.mg_phase_vocoder_locked(ptr, ptr, ptr, 16, 8, 1, 1, None) == lib.mg_phase_vocoder(ptr, ptr, ptr, 16, 8, 1, 1, None) != 0
