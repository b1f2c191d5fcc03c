"""CPU: the float64 yardstick of tests/melspec_ref.py against hand-computed values, every host-side refusal of mel_ops.mel_power,
mel_ops.logmel_pool, audio.mel_spectrogram, metrics.WaveLogMel, `evaluate_mel_waveform` and `evaluate_audio` -- each raised
before a device is touched, so they all run without one --, and the command line of the two drivers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import melspec_ref as R  # noqa: E402


# ------------------------------------------------------------------ the reference
def test_reference_unit_sine_at_bin_100_has_the_closed_form_power():
    """a unit sine exactly on bin 100: |X|^2 = (A / 2 * sum w)^2 / sum w^2 = 0.25 * 512^2 / 384 in every interior frame"""
    n = np.arange(4096)
    x = np.sin(2 * np.pi * 100 * n / 1024).astype(np.float32)
    p = R.power_of_bins(R.stft(x))
    assert p.shape == (512, 17)
    want = 0.25 * 512 ** 2 / 384
    assert abs(want - 170.66667) < 1e-5
    for t in range(2, 15):                                                # frames 2 .. 14 lie inside the signal
        assert abs(p[100, t] - want) < 1e-5 * want, (t, p[100, t])
        assert p[:98, t].max() < 1e-9 * want and p[103:, t].max() < 1e-9 * want   # Hann: three bins wide
    one = np.zeros((1, 512), dtype=np.float32)
    one[0, 100] = 2.0
    s = R.mel_power(x[None], one, [100], [101])
    assert s.shape == (1, 1, 17) and abs(s[0, 0, 8] - 2 * want) < 1e-4


def test_reference_frames_reflect_and_the_float32_chain_is_float32():
    x = np.arange(1024, dtype=np.float32)
    f = R.frames(x)
    assert f.shape == (5, 1024)                                           # T = 1 + 1024 // 256
    assert f[0, 0] == 512 and f[0, 511] == 1 and f[0, 512] == 0           # reflect padding by 512, the edge sample not repeated
    assert f[2, 0] == 0 and f[2, 1023] == 1023                            # the only interior frame
    assert f[4, 511] == 1023 and f[4, 512] == 1022
    w = np.ones((2, 512), dtype=np.float32)
    got = R.mel_power_f32(x[None] / 1024, w, [0, 7], [512, 7])
    assert got.dtype == np.float32 and (got[0, 1] == 0).all() and not np.signbit(got[0, 1]).any()   # an empty band: +0.0
    ref = R.mel_power(x[None] / 1024, w, [0, 7], [512, 7])
    assert ref.dtype == np.float64 and np.abs(got[0, 0] - ref[0, 0]).max() < 1e-4 * ref[0, 0].max()
    assert abs(float((R.window() ** 2).sum()) - 1.0) < 1e-12


def test_reference_window_hop_and_tail_arithmetic():
    assert R.frame_count(130816) == 512 and R.frame_count(130815) == 511 and R.frame_count(256 * 15 + 1) == 16
    assert R.window_count(512, 512, 512) == 1 and R.window_count(511, 512, 512) == 0
    assert R.window_count(17, 16, 16) == 1                               # the tail frame is dropped
    assert R.window_count(512, 64, 32) == 15 and R.window_count(1535, 512, 512) == 2
    power = np.arange(2 * 3 * 17, dtype=np.float64).reshape(2, 3, 17) + 1.0
    rows = R.logmel_pool(power, 8, 4, 2, 0.5)
    assert rows.shape == (2 * 3, 3 * 2)                                   # W = (17 - 8) // 4 + 1 = 3 windows per row
    # row b W + n, column m P + j: the mean over frames n hop + j win / P .. + win / P - 1
    b, n, m, j = 1, 2, 1, 1
    want = np.log(power[b, m, 8 + 4:8 + 8] + 0.5).mean()
    assert abs(rows[b * 3 + n, m * 2 + j] - want) < 1e-15


# ------------------------------------------------------------------ refusals, all before a device is looked at
def _args(bands=4):
    lo = torch.zeros(bands, dtype=torch.int32)
    hi = torch.full((bands,), 512, dtype=torch.int32)
    return dict(wave=torch.zeros(2, 1024), weight=torch.zeros(bands, 512), lo=lo, hi=hi)


def test_mel_power_refuses_bad_arguments_on_the_host():
    from musicgan_amd import _lib, mel_ops
    good = _args()
    bad = [dict(wave=torch.zeros(1024)), dict(wave=torch.zeros(2, 512)), dict(wave=torch.zeros(0, 1024)),
           dict(wave=torch.zeros(2, 2048)[:, ::2]),                      # samples of a row not contiguous
           dict(wave=torch.zeros(1024, 2).t()),
           dict(weight=torch.zeros(4, 511)), dict(weight=torch.zeros(512)), dict(**_args(257)),   # M > 256
           dict(lo=torch.tensor([0, 0, 9, 0], dtype=torch.int32), hi=torch.tensor([1, 1, 8, 1], dtype=torch.int32)),   # lo > hi
           dict(hi=torch.tensor([1, 1, 513, 1], dtype=torch.int32)),     # hi > 512
           dict(lo=torch.tensor([0, -1, 0, 0], dtype=torch.int32)),
           dict(lo=torch.zeros(4, dtype=torch.int64)), dict(hi=torch.zeros(3, dtype=torch.int32)), dict(lo=[0, 0, 0, 0]),
           dict(wave=torch.zeros(2, 1024, dtype=torch.float64)), dict(weight=torch.zeros(4, 512, dtype=torch.float16)),
           dict(out=torch.zeros(2, 4, 4)), dict(out=torch.zeros(2, 4, 5, dtype=torch.float64))]
    for kw in bad:
        with pytest.raises(ValueError):
            mel_ops.mel_power(**{**good, **kw})
    with pytest.raises(_lib.MusicGanHipError):                            # everything right but the device: no fallback
        mel_ops.mel_power(**good)
    assert mel_ops.mel_frames(130816) == 512 and mel_ops.mel_frames(1024) == 5


def test_logmel_pool_refuses_bad_arguments_on_the_host():
    from musicgan_amd import _lib, mel_ops
    power = torch.ones(2, 4, 17)
    good = dict(power=power, win=16, hop=16, pools=4, floor=1e-6)
    bad = [dict(power=torch.ones(4, 17)), dict(power=torch.ones(2, 257, 17)), dict(power=torch.ones(2, 4, 0)),
           dict(pools=3),                                                # P does not divide win
           dict(win=18, pools=2),                                        # T < win
           dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan")),
           dict(win=0), dict(hop=0), dict(pools=0), dict(win=16.0), dict(hop=True),
           dict(power=power.double()), dict(out=torch.zeros(1, 16)), dict(out=torch.zeros(2, 16, dtype=torch.float64))]
    for kw in bad:
        with pytest.raises(ValueError):
            mel_ops.logmel_pool(**{**good, **kw})
    with pytest.raises(_lib.MusicGanHipError):
        mel_ops.logmel_pool(**good)
    assert mel_ops.pool_windows(17, 16, 16) == 1 and mel_ops.pool_windows(15, 16, 16) == 0 and mel_ops.pool_windows(512, 64, 32) == 15


def test_mel_spectrogram_and_wavelogmel_refuse_on_the_host():
    from musicgan_amd import audio, metrics
    for bad in (torch.zeros(512), torch.zeros(2, 3, 100), torch.zeros(1024, dtype=torch.int16), torch.zeros(0, 1024), [0.0] * 1024):
        with pytest.raises(ValueError):
            audio.mel_spectrogram(bad)
    for kw in (dict(n_mels=0), dict(n_mels=400), dict(f_min=9000.0, f_max=8000.0), dict(f_max=30000.0)):
        with pytest.raises(ValueError):
            audio.mel_spectrogram(torch.zeros(1024), **kw)               # the bank is refused before a device is looked at
    assert "mel_spectrogram" in audio.__all__ and "torchaudio is not installed" in audio.mel_spectrogram.__doc__
    wl = metrics.WaveLogMel()
    assert (wl.bands, wl.pools, wl.window, wl.hop, wl.floor, wl.dims) == (64, 32, 512, 512, 1e-6, 2048)
    assert tuple(wl.weight.shape) == (64, 512) and wl.windows(130816) == 1 and wl.windows(130816 + 512 * 256) == 2
    for kw in (dict(pools=3), dict(pools=0), dict(window=0), dict(hop=0), dict(floor=0.0), dict(bands=400), dict(f_min=-1.0)):
        with pytest.raises(ValueError):
            metrics.WaveLogMel(**kw)
    for bad in (torch.zeros(130816), torch.zeros(1, 1000), torch.zeros(0, 130816)):
        with pytest.raises(ValueError):
            wl(bad)


# ------------------------------------------------------------------ the drivers
def test_evaluate_mel_waveform_refusals_before_any_work():
    """evaluate_mel keeps its parameter list (tests/test_logmel_cpu.py pins it), so the waveform rows are a function of their own
    beside it, with the same parameters and `griffin_lim`; it refuses every level but 7 before any work"""
    import inspect
    import musicgan_amd
    fn = musicgan_amd.__getattr__("evaluate_mel_waveform")
    plain = musicgan_amd.__getattr__("evaluate_mel")
    assert callable(plain) and musicgan_amd.evaluate_mel is plain and fn is sys.modules["musicgan_amd.evaluate_mel"].evaluate_mel_waveform
    assert list(inspect.signature(fn).parameters) == list(inspect.signature(plain).parameters) + ["griffin_lim"]
    assert inspect.signature(fn).parameters["griffin_lim"].default == 0
    missing = ("/nonexistent/gen.pt", 8, "/nonexistent/data")
    for kw in (dict(level=6), dict(level=4), dict(level=8), dict(griffin_lim=-1), dict(griffin_lim=1.5), dict(griffin_lim=True),
               dict(metrics=("swd",)), dict(metrics=()), dict(nb_images=3), dict(metrics=("prdc",), nb_images=7), dict(batch_size=0)):
        with pytest.raises(ValueError):
            fn(*missing, **kw)
    with pytest.raises(TypeError):
        plain(*missing, griffin_lim=8)                                    # Griffin-Lim has no meaning without the waveform


def test_evaluate_audio_refusals_before_any_work():
    import inspect
    import musicgan_amd
    fn = musicgan_amd.__getattr__("evaluate_audio")
    assert musicgan_amd.evaluate_audio is fn
    sig = inspect.signature(fn)
    assert list(sig.parameters)[:3] == ["real_path", "fake_path", "metrics"] and sig.parameters["metrics"].default == ("fd",)
    for name, default in (("nb_windows", 8192), ("seed", 0), ("resample", False), ("output", None)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    for kw in (dict(metrics=("fid",)), dict(metrics=()), dict(metrics=("fd", "fd")), dict(metrics=("swd",)), dict(nb_windows=0),
               dict(nb_windows=3), dict(metrics=("prdc",), nb_windows=7), dict(metrics=("ndb",), nb_windows=7)):
        with pytest.raises(ValueError):
            fn("/nonexistent/*.wav", "/nonexistent/*.flac", **kw)


def test_the_parser_takes_both_drivers_and_hands_over_the_keywords(monkeypatch):
    import importlib
    from musicgan_amd.__main__ import _FEATURE_MODES, _FILE_SET_MODES, _all_modes, build_parser, main
    assert list(_FILE_SET_MODES) == ["evaluate_audio"] and list(_FEATURE_MODES) == ["evaluate_mel"]
    assert "evaluate_audio" in _all_modes()
    p = build_parser()
    a = p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data", "--waveform", "--griffin-lim", "8"])
    kw = _FEATURE_MODES["evaluate_mel"][4](a)
    assert a.waveform and kw == dict(level=7, nb_images=8192, batch_size=16, seed=0, output=None, griffin_lim=8)
    plain = _FEATURE_MODES["evaluate_mel"][4](p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data"]))
    assert "waveform" not in plain and "griffin_lim" not in plain        # without the flags: the call of before
    with pytest.raises(SystemExit):
        main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--griffin-lim", "8"])   # needs --waveform
    a = p.parse_args(["evaluate_audio", "real/*.flac", "gen/*.wav", "--metrics", "fd,kid,nn,prdc,ndb", "--resample", "-n", "100",
                      "--seed", "3", "-o", "out.json"])
    _, _, _, pos, kw = _FILE_SET_MODES["evaluate_audio"]
    assert pos(a) == ("real/*.flac", "gen/*.wav")
    assert kw(a) == dict(nb_windows=100, seed=3, output="out.json", metrics=("fd", "kid", "nn", "prdc", "ndb"), resample=True)
    assert kw(p.parse_args(["evaluate_audio", "a", "b"])) == dict(nb_windows=8192, seed=0, output=None)
    for bad in ("fid", "swd", "fd,fd"):
        with pytest.raises(SystemExit):
            p.parse_args(["evaluate_audio", "a", "b", "--metrics", bad])
    seen = []
    for mode, name in (("evaluate_mel", "evaluate_mel"), ("evaluate_mel", "evaluate_mel_waveform"), ("evaluate_audio", "evaluate_audio")):
        module = importlib.import_module(f"musicgan_amd.{mode}")
        monkeypatch.setattr(module, name, lambda *args, _name=name, **kwargs: seen.append((_name, args, kwargs)))
    main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--waveform", "--metrics", "kid"])
    main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--waveform", "--griffin-lim", "8"])
    main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--metrics", "kid"])
    main(["evaluate_audio", "a/*.wav", "b/*.ogg", "--metrics", "nn"])
    base = dict(level=7, nb_images=8192, batch_size=16, seed=0, output=None)
    assert seen == [("evaluate_mel_waveform", ("gen.pt", 32, "data"), dict(base, metrics=("kid",))),
                    ("evaluate_mel_waveform", ("gen.pt", 32, "data"), dict(base, griffin_lim=8)),
                    ("evaluate_mel", ("gen.pt", 32, "data"), dict(base, metrics=("kid",))),
                    ("evaluate_audio", ("a/*.wav", "b/*.ogg"), dict(nb_windows=8192, seed=0, output=None, metrics=("nn",)))]


def test_the_abi_declares_and_binds_the_two_entry_points():
    from musicgan_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "musicgan_hip.h")).read()
    for name in ("mg_mel_power", "mg_logmel_pool"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
