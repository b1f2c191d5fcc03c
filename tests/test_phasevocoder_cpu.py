"""No GPU: the restatement of the phase vocoder against itself (the literal torchaudio form and the mod-2 pi form agree in float64),
the host arithmetic (output length, pitch ratios, per-file sample counts), every argument error, the command line, the C ABI and
the build's register report for csrc/phasevocoder.hip."""
import math
import os
import re
import sys
from fractions import Fraction

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import phasevocoder_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 2), (4, 9, 10), (5, 1, 1), (37, 11, 10), (130, 53, 50), (64, 2, 1), (64, 1, 2), (64, 8, 1), (16, 1, 8),
          (1536, 17, 18), (8192, 9, 10), (8192, 5, 4)]


@pytest.mark.parametrize("frames,p,q", SHAPES, ids=[f"{t}-{p}_{q}" for t, p, q in SHAPES])
@pytest.mark.parametrize("kind", ["random", "tonal"])
def test_literal_and_mod_2pi_forms_agree_in_float64(kind, frames, p, q):
    X = R.MAKERS[kind](frames, 1000 + frames)
    a, b = R.literal(X, p, q, torch.float64), R.exact(X, p, q, torch.float64)
    assert a.shape == b.shape == (512, R.out_len(frames, p, q)) and b.dtype == torch.complex128
    err = float((a - b).abs().max())
    bound = 1e-9 if frames <= 130 else 1e-6
    print(f"LITERAL vs EXACT {kind} T={frames} {p}/{q}: {err:.3e} (bound {bound:.0e}, max|ref| {float(b.abs().max()):.3f})")
    assert err <= bound


@pytest.mark.parametrize("kind", ["random", "tonal"])
def test_what_float32_accumulation_costs(kind):
    """context for the GPU tolerance at T = 8192: the float32 arithmetic of abs / angle alone (`mixed`) against forms that also
    accumulate in float32 -- both of the latter must stand outside the tolerance 4 x own"""
    X = R.MAKERS[kind](8192, 1000 + 8192)
    ref = R.exact(X, 9, 10, torch.float64)
    own = float((R.mixed(X, 9, 10).to(torch.complex128) - ref).abs().max())
    e32 = float((R.exact(X, 9, 10, torch.float32).to(torch.complex128) - ref).abs().max())
    lit = float((R.literal(X, 9, 10, torch.float32).to(torch.complex128) - ref).abs().max())
    print(f"ACCUMULATION {kind} T=8192 9/10: mixed {own:.3e}, all-float32 mod-2pi form {e32:.3e}, literal float32 {lit:.3e}")
    assert e32 > 4 * own and lit > 4 * own


def test_rate_one_is_the_identity_in_float64():
    """5e-15 at T = 5.  At T = 130 no float64 running sum can hold that figure: the partial sums of 130 deviations of up to pi reach
    tens of radians, where one rounding is 2e-15 to 4e-15 rad, times magnitudes of 4 (measured: 1.2e-13).  There the bound is the
    worst case of the arithmetic: T additions, each off by at most half an ulp of a partial sum below pi T, plus T times the
    3 x 6.2e-17 by which three float64 quarter turns differ from 3 pi / 2, times the largest magnitude."""
    X = R.random_spectrum(5, 1005)
    err = float((R.exact(X, 1, 1, torch.float64) - X.to(torch.complex128)).abs().max())
    print(f"IDENTITY T=5: {err:.3e}")
    assert err <= 5e-15
    X = R.random_spectrum(130, 1130)
    err = float((R.exact(X, 1, 1, torch.float64) - X.to(torch.complex128)).abs().max())
    half_ulp = 2.0 ** (math.ceil(math.log2(math.pi * 130)) - 53)
    bound = float(X.abs().max()) * 130 * (half_ulp + 3 * 6.2e-17)
    print(f"IDENTITY T=130: {err:.3e} (worst case of the float64 sum {bound:.3e})")
    assert err <= bound


def test_output_length():
    from musicgan_amd import pv_ops
    for p, q in ((1, 2), (2, 1), (5, 4), (1, 8)):   # rates whose float form is exact: torchaudio's arange(0, T, rate)
        for frames in (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 130, 1000, 1537):
            assert pv_ops.phase_vocoder_len(frames, p, q) == len(torch.arange(0, frames, p / q)) == R.out_len(frames, p, q)
    for p, q in ((9, 10), (11, 10), (53, 50), (17, 18)):
        for frames in (1, 2, 9, 10, 11, 37, 130, 8192, 103360, 2 ** 31 - 1, 2 ** 31):
            assert pv_ops.phase_vocoder_len(frames, p, q) == -((-frames * q) // p)
    lib = __import__("musicgan_amd._lib", fromlist=["load"]).load()
    assert lib.mg_phase_vocoder_len(0, 1, 1) == -1 and lib.mg_phase_vocoder_len(10, 0, 1) == -1
    assert lib.mg_phase_vocoder_len(10, 9, 1) == -1 and lib.mg_phase_vocoder_len(10, 1, 9) == -1
    assert lib.mg_phase_vocoder_len(2 ** 60, 4, 1) == -1 and lib.mg_phase_vocoder_len(2 ** 60 - 1, 4, 1) == 2 ** 58
    assert lib.mg_phase_vocoder_ws_bytes(10, 9, 1) == 0
    tiles = -(-R.out_len(1000, 9, 10) // pv_ops.TIME_TILE)
    assert lib.mg_phase_vocoder_ws_bytes(1000, 9, 10) == 512 * 1000 * 8 + 512 * tiles * 8


def test_tile_constant_is_the_kernels():
    from musicgan_amd import pv_ops
    src = open(os.path.join(ROOT, "musicgan_amd", "csrc", "phasevocoder.hip")).read()
    assert int(re.search(r"constexpr int TILE = (\d+);", src).group(1)) == pv_ops.TIME_TILE


def test_pitch_ratio():
    from musicgan_amd import audio
    worst = 0.0
    for n in range(-12, 13):
        f = audio.pitch_ratio(n)
        assert isinstance(f, Fraction) and f.denominator <= 64
        worst = max(worst, abs(1200 * math.log2(f) - 100 * n))
    print(f"PITCH RATIO: at most {worst:.3f} cents off for -12 .. 12")
    assert worst <= 2.0
    assert audio.pitch_ratio(12) == Fraction(2, 1) and audio.pitch_ratio(-12) == Fraction(1, 2)
    assert audio.pitch_ratio(0) == Fraction(1, 1) and audio.pitch_ratio(1.0) == audio.pitch_ratio(1)
    assert audio.pitch_ratio(1).numerator <= 128   # the resampler's reduced input step


def test_argument_errors_need_no_device():
    from musicgan_amd import audio, pv_ops
    from musicgan_amd.create_dataset import check_variants, create_dataset
    X = torch.zeros(512, 8, dtype=torch.complex64)
    for rate in (0.1, 8.5, Fraction(1, 9), 9, 0, -1, True, "1", float("nan")):
        with pytest.raises(ValueError):
            audio.phase_vocoder(X, rate)
        with pytest.raises(ValueError):
            audio.time_stretch(torch.zeros(4096), rate)
    with pytest.raises(ValueError):
        audio.phase_vocoder(torch.zeros(511, 8, dtype=torch.complex64), 1)
    with pytest.raises(ValueError):
        audio.phase_vocoder(torch.zeros(512, 0, dtype=torch.complex64), 1)
    with pytest.raises(ValueError):
        audio.phase_vocoder(torch.zeros(512, 8), 1)
    with pytest.raises(ValueError):
        audio.time_stretch(torch.zeros(2, 4096), 1)
    with pytest.raises(ValueError):
        audio.pitch_shift(torch.zeros(4096), 37)    # 2^(37/12) > 8
    for bad in ((0, 1, 1), (8, 0, 1), (8, 1, 0), (8, 9, 1), (8, 1, 9), (2 ** 60, 4, 1), (8, 2 ** 31, 2 ** 31)):
        with pytest.raises(ValueError):
            pv_ops.phase_vocoder_len(*bad)
        with pytest.raises(ValueError):
            pv_ops.check_arguments(*bad)
    assert pv_ops.as_rate(0.9) == Fraction(9, 10) and pv_ops.as_rate(2) == 2 and pv_ops.as_rate(1 / 3) == Fraction(1, 3)
    for kw in (dict(stretch=(1,)), dict(stretch=(1.0,)), dict(pitch=(0,)), dict(pitch=(0.0,)), dict(stretch=(0.9, Fraction(9, 10))),
               dict(pitch=(1, 1.0)), dict(stretch=(9,)), dict(stretch=(0.1,)), dict(pitch=(40,)), dict(pitch=(-40,))):
        with pytest.raises(ValueError):
            check_variants(**kw)
        with pytest.raises(ValueError):   # before the glob, the output directory or the device
            create_dataset("/nonexistent/*.wav", "/nonexistent/out", **kw)
    rates, ratios = check_variants((Fraction(9, 10), 1.1), (-1, 1))
    assert rates == (Fraction(9, 10), Fraction(11, 10)) and [f for _, f in ratios] == [Fraction(50, 53), Fraction(53, 50)]


def test_sample_counts_by_host_arithmetic():
    from musicgan_amd.create_dataset import _nb_samples, check_variants, variant_counts
    rates, ratios = check_variants((Fraction(9, 10), 2), (1, -12))
    for length in (44100, 44100 * 4, 44100 * 5, 256 * 512, 256 * 512 - 1, 256 * 1024 + 255):
        got = variant_counts(length, 512, rates, ratios)
        t = 1 + length // 256
        want = [_nb_samples(length, 512)]
        for p, q in ((9, 10), (2, 1)):
            n = -((-t * q) // p)
            want.append(0 if n < 512 else (n - 1) // 512)
        for P, Q in ((53, 50), (1, 2)):
            t1 = 1 + (-((-length * Q) // P)) // 256
            n = -((-t1 * P) // Q)
            want.append(0 if n < 512 else (n - 1) // 512)
        assert got == want, (length, got, want)
    assert variant_counts(44100 * 5, 512) == [_nb_samples(44100 * 5, 512)]


def test_command_line():
    from musicgan_amd.__main__ import _MODES, build_parser
    kwargs = _MODES["create_dataset"][4]
    a = build_parser().parse_args(["create_dataset", "in/*.wav", "-o", "out", "--stretch", "9/10,1.1", "--pitch", "-1,1"])
    assert a.stretch == (Fraction(9, 10), Fraction(11, 10)) and a.pitch == (Fraction(-1), Fraction(1))
    assert kwargs(a) == {"stretch": a.stretch, "pitch": a.pitch}
    a = build_parser().parse_args(["create_dataset", "in/*.wav", "-o", "out", "--pitch", "-0.5", "--resample"])
    assert kwargs(a) == {"resample": True, "pitch": (Fraction(-1, 2),)}
    for argv, want in ((["create_dataset", "in/*.wav", "-o", "out"], {}),
                       (["create_dataset", "in/*.wav", "-o", "out", "--resample"], {"resample": True})):
        a = build_parser().parse_args(argv)
        assert kwargs(a) == want and _MODES["create_dataset"][3](a) == ("in/*.wav", "out")
    for bad in ("9/0", "fast", "1,,2"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["create_dataset", "in/*.wav", "-o", "out", "--stretch", bad])


def test_abi_and_registers():
    from musicgan_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "musicgan_hip.h")).read()
    _build.build()
    lib = _lib.load()
    for name in ("mg_phase_vocoder_len", "mg_phase_vocoder_ws_bytes", "mg_phase_vocoder"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    usage = {k: v for k, v in _build.resource_usage().items() if re.search(r"pv_(polar|tile_sums|row_scan|finish)", k)}
    assert len(usage) == 4, sorted(usage)
    for name, u in usage.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)
