"""No GPU: the restatement of the harmonic / percussive separation against a brute-force reading of its definition, the selection
network and the index reflection of csrc/hpss_select.h compiled for the host, the overlap-add re-timing at rate 1, the host
arithmetic (output lengths, per-file sample counts), every argument error, the command line, the C ABI and the build's register
report for csrc/hpss.hip."""
import ctypes
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from musicgan_amd import hpss_ops  # the module under test: without it nothing here can pass

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpss_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = [(31, 31), (3, 63), (63, 3), (17, 9)]
assert all(hpss_ops.MIN_KERNEL <= length <= hpss_ops.MAX_KERNEL for kernel in KERNELS for length in kernel)


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: f"{k[0]}x{k[1]}")
@pytest.mark.parametrize("frames", [1, 5, 40])
def test_reference_medians_are_the_sorted_reflected_windows(frames, kernel):
    """T = 1 and 5 are shorter than half of most windows: the reflection folds several times"""
    X = R.random_spectrum(frames, 2000 + frames)
    H, P = R.medians(X, *kernel)
    Hb, Pb = R.brute(X, *kernel)
    assert H.dtype == np.float32 and H.shape == (512, frames) == P.shape
    assert np.array_equal(H.view(np.uint32), Hb.view(np.uint32)) and np.array_equal(P.view(np.uint32), Pb.view(np.uint32))


def test_reference_masks():
    X, ref = R.case("random", 40)
    assert np.abs(ref["mask_h"] + ref["mask_p"] - 1.0).max() <= 4e-16           # margins 1: the masks sum to 1
    assert np.abs(ref["harmonic"] + ref["percussive"] - X.to(torch.complex128).numpy()).max() <= 4e-15
    wide = R.separate(X, (31, 31), 2.0, (2.0, 3.0))
    assert (wide["mask_h"] <= ref["mask_h"]).all() and (wide["mask_p"] <= ref["mask_p"]).all()
    hard = R.separate(X, (31, 31), math.inf, (1.0, 1.0))
    assert set(np.unique(hard["mask_h"])) <= {0.0, 1.0} and np.array_equal(hard["mask_h"], (ref["H"] > ref["P"]).astype(np.float64))
    quiet = R.separate(R.silent_spectrum(5, 0))
    assert (quiet["mask_h"] == 0.5).all() and (quiet["mask_p"] == 0.5).all() and (quiet["harmonic"] == 0).all()
    assert (R.separate(R.silent_spectrum(5, 0), margin=(2.0, 1.0))["mask_h"] == 0.0).all()
    one = R.separate(X, (31, 31), 1.0, (1.0, 1.0))
    assert np.abs(one["mask_h"] - ref["H"].astype(np.float64) / (ref["H"].astype(np.float64) + ref["P"])).max() <= 1e-15


def test_selection_network_and_reflection_compiled_for_the_host(tmp_path):
    """csrc/hpss_select.h by g++: the middle one of 31 and of 63 keys against numpy's sort for random keys, keys of two and of five
    values (ties; by the 0-1 principle a selection network is right when it is right on every 0-1 input, of which 2^20 are drawn
    here) and for float bit patterns; shorter windows padded as the kernel pads them; the reflection against folding step by step"""
    csrc = os.path.join(ROOT, "musicgan_amd", "csrc")
    shim = tmp_path / "shim.cpp"
    shim.write_text('#define HPSS_FN static inline\n#include "hpss_select.h"\n'
                    'template <int N> static void run(const uint32_t* keys, uint32_t* out, long n, int L) { for (long i = 0; i < n; ++i) {'
                    ' uint32_t a[N]; const int pad = (N - 1 - L) / 2; for (int j = 0; j < N - 1; ++j) { const int w = j - pad;'
                    ' a[j] = w < 0 ? hpss::KEY_MIN : (w < L ? keys[L * i + w] : hpss::KEY_MAX); } out[i] = hpss::median<N>(a); } }\n'
                    'extern "C" void median32_n(const uint32_t* keys, uint32_t* out, long n, int L) { run<32>(keys, out, n, L); }\n'
                    'extern "C" void median64_n(const uint32_t* keys, uint32_t* out, long n, int L) { run<64>(keys, out, n, L); }\n'
                    'extern "C" long long reflect1(long long j, long long n) { return hpss::reflect(j, n); }\n')
    so = str(tmp_path / "shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", csrc, str(shim), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.reflect1.restype = ctypes.c_longlong
    lib.reflect1.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
    rng = np.random.default_rng(3)
    n = 1 << 20
    floats = np.abs(rng.standard_normal((n, 31))).astype(np.float32)
    floats[:64, :7] = 0.0
    floats[64:128, 3:30] = np.inf

    def check(fn, keys):
        keys = np.ascontiguousarray(keys)
        out = np.empty(keys.shape[0], dtype=np.uint32)
        fn(keys.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), ctypes.c_long(keys.shape[0]), ctypes.c_int(keys.shape[1]))
        assert np.array_equal(out, np.sort(keys, axis=1)[:, keys.shape[1] // 2]), keys.shape

    for keys in (rng.integers(0, 1 << 32, (n, 31), dtype=np.uint64).astype(np.uint32), rng.integers(0, 2, (n, 31)).astype(np.uint32),
                 rng.integers(0, 5, (n, 31)).astype(np.uint32), floats.view(np.uint32)):
        check(lib.median32_n, keys)
    for keys in (rng.integers(0, 1 << 32, (n // 2, 63), dtype=np.uint64).astype(np.uint32), rng.integers(0, 2, (n, 63)).astype(np.uint32),
                 rng.integers(0, 5, (n // 2, 63)).astype(np.uint32)):
        check(lib.median64_n, keys)
    for length in (3, 9, 17, 29):                       # padded with as many smallest as largest keys; the key values 0 and 2^32 - 1 too
        keys = rng.integers(0, 1 << 32, (1 << 16, length), dtype=np.uint64).astype(np.uint32)
        keys[:256, ::2] = 0
        keys[256:512, 1::2] = 0xFFFFFFFF
        check(lib.median32_n, keys)
    for length in (3, 33, 47, 61):
        check(lib.median64_n, rng.integers(0, 7, (1 << 16, length)).astype(np.uint32))
    assert np.array_equal(np.sort(floats, axis=1)[:, 15].view(np.uint32), np.sort(floats.view(np.uint32), axis=1)[:, 15])
    for size in (1, 2, 5, 40, 512, 2 ** 31 - 129):
        for j in list(range(-130, 130)) + [size - 1, size, size + 62, 2 * size - 1, 2 * size, 3 * size + 1, -size - 1, -2 * size]:
            r = j
            while r < 0 or r >= size:
                r = -r - 1 if r < 0 else 2 * size - 1 - r
            assert lib.reflect1(j, size) == r == R.reflect(j, size), (j, size)


@pytest.mark.parametrize("length", [1, 255, 256, 257, 256 * 9, 256 * 9 + 100])
def test_overlap_add_at_rate_one_is_the_identity(length):
    """in float32, as the device computes: within 2^-22 max|x| (two roundings of w, one product each, one sum)"""
    x = R.waveform(length, 10 + length).numpy()
    y, _ = R.ola(x, 7, 7, length, np.float32)
    err = float(np.abs(y.astype(np.float64) - x).max())
    print(f"OLA IDENTITY L={length}: err {err:.3e}, bound {2.0 ** -22 * float(np.abs(x).max()):.3e}")
    assert y.dtype == np.float32 and y.shape == (length,)
    assert err <= 2.0 ** -22 * float(np.abs(x).max())
    exact, _ = R.ola(x, 1, 1, length + 300)
    assert float(np.abs(exact[:length] - x).max()) <= 1e-14 and not exact[length:].any()
    w = R.window(np.float32)
    assert w[0] == 0 and w[256] == 1 and float(np.abs(w[:256].astype(np.float64) + w[256:] - 1).max()) <= 2.0 ** -24


def test_overlap_add_reference_reads_where_the_definition_says():
    """rate 2: frame m is taken from 512 m; rate 1/2: from 128 m -- spelled out sample by sample"""
    x = R.waveform(256 * 9, 5).numpy().astype(np.float64)
    w = R.window()
    for p, q in ((2, 1), (1, 2), (11, 10)):
        out_len = 256 * 4 + 17
        y, mass = R.ola(x, p, q, out_len)
        for n in (0, 1, 255, 256, 257, 700, out_len - 1):
            m, j = divmod(n, 256)
            a, b = (256 * m * p) // q, ((256 * (m - 1) * p) // q if m else -256)
            x1 = x[a + j] if 0 <= a + j < len(x) else 0.0
            x2 = x[b + j + 256] if 0 <= b + j + 256 < len(x) else 0.0
            assert y[n] == w[j] * x1 + w[j + 256] * x2 and mass[n] == abs(x1) + abs(x2)
    assert R.ola(x, 1, 1, 0)[0].shape == (0,)


def test_output_lengths():
    from musicgan_amd import hpss_ops, pv_ops
    for frames in (4, 5, 37, 130, 513, 103360):
        for rate in (Fraction(1), Fraction(9, 10), Fraction(11, 10), Fraction(1, 8), Fraction(8)):
            n = math.ceil(frames / rate)
            assert hpss_ops.stretched_samples(frames, rate) == 256 * (n - 1)
            # ... whose STFT has the frames of the phase vocoder's output: the two parts of a variant can be added
            assert 1 + hpss_ops.stretched_samples(frames, rate) // 256 == pv_ops.phase_vocoder_len(frames, rate.numerator, rate.denominator)


def test_tile_constant_is_the_kernels():
    from musicgan_amd import hpss_ops
    src = open(os.path.join(ROOT, "musicgan_amd", "csrc", "hpss.hip")).read()
    assert int(re.search(r"constexpr int TILE = (\d+);", src).group(1)) == hpss_ops.TILE
    assert int(re.search(r"constexpr int MAX_L = (\d+);", src).group(1)) == hpss_ops.MAX_KERNEL
    assert int(re.search(r"constexpr int OLA_HOP = (\d+);", src).group(1)) == hpss_ops.OLA_HOP


def test_argument_errors_need_no_device():
    from musicgan_amd import _lib, audio, hpss_ops
    from musicgan_amd.create_dataset import check_separation, create_dataset
    from musicgan_amd.separate import separate
    X = torch.zeros(512, 8, dtype=torch.complex64)
    bad = [dict(kernel_size=30), dict(kernel_size=(31, 30)), dict(kernel_size=65), dict(kernel_size=(65, 3)), dict(kernel_size=1),
           dict(kernel_size=31.0), dict(kernel_size=(31, 31, 31)), dict(kernel_size=True), dict(power=3), dict(power=0.5),
           dict(power=float("nan")), dict(power="2"), dict(margin=0.5), dict(margin=(1.0, 0.99)), dict(margin=float("inf")),
           dict(margin=float("nan")), dict(margin=(1, 2, 3)), dict(margin="1")]
    for kw in bad:
        with pytest.raises(ValueError):
            audio.hpss(X, **kw)
        with pytest.raises(ValueError):
            hpss_ops.hpss(X, **{**kw, **({"kernel_size": (kw["kernel_size"],) * 2} if isinstance(kw.get("kernel_size"), int) else {})})
        with pytest.raises(ValueError):
            audio.harmonic(torch.zeros(4096), **kw)
        with pytest.raises(ValueError):
            audio.percussive(torch.zeros(4096), **kw)
    for want in ((), ("harmonic", "harmonic"), ("magnitude",)):
        with pytest.raises(ValueError):
            hpss_ops.hpss(X, want=want)
    for spectrum in (torch.zeros(511, 8, dtype=torch.complex64), torch.zeros(512, 0, dtype=torch.complex64), torch.zeros(512, 8),
                     torch.zeros(2, 512, 8, dtype=torch.complex64)):
        with pytest.raises(ValueError):
            audio.hpss(spectrum)
    with pytest.raises(ValueError):
        audio.harmonic(torch.zeros(2, 4096))
    with pytest.raises(ValueError):
        audio.time_stretch(torch.zeros(2, 4096), 1, preserve_transients=True)
    with pytest.raises(ValueError):
        audio.time_stretch(torch.zeros(4096), 9, preserve_transients=True)
    with pytest.raises(ValueError):
        audio.pitch_shift(torch.zeros(4096), 37, preserve_transients=True)
    assert hpss_ops.check_arguments(31, 2, 1) == (31, 31, 2.0, 1.0, 1.0, ("harmonic", "percussive"))
    assert hpss_ops.check_arguments((3, 63), math.inf, (1, 2.5), "H") == (3, 63, math.inf, 1.0, 2.5, ("H",))
    x = torch.zeros(4096)
    for args in ((0, 1, 10), (1, 0, 10), (9, 1, 10), (1, 9, 10), (1, 1, -1), (2 ** 31, 2 ** 31, 10), (1, 1, 2 ** 40), (4, 1, 2 ** 60),
                 (1.0, 1, 10), (1, 1, 10.0), (True, 1, 10)):
        with pytest.raises(ValueError):
            hpss_ops.ola_stretch(x, *args)
    with pytest.raises(ValueError):
        hpss_ops.ola_stretch(torch.zeros(0), 1, 1, 10)
    with pytest.raises(ValueError):
        hpss_ops.ola_stretch(torch.zeros(2, 4096), 1, 1, 10)
    # what is left once the arguments are fine: no device, and no CPU path
    with pytest.raises(_lib.MusicGanHipError):
        hpss_ops.hpss(X)
    with pytest.raises(_lib.MusicGanHipError):
        hpss_ops.ola_stretch(x, 1, 1, 10)
    for kw in (dict(preserve_transients=True), dict(component="tonal"), dict(component="harmonic", preserve_transients=True),
               dict(component=1), dict(preserve_transients=1, stretch=(2,))):
        with pytest.raises(ValueError):   # before the glob, the output directory or the device
            create_dataset("/nonexistent/*.wav", "/nonexistent/out", **kw)
    with pytest.raises(ValueError):
        check_separation(None, True)
    check_separation("percussive", True, rates=(Fraction(9, 10),))
    check_separation(None, True, ratios=((1, Fraction(53, 50)),))
    for kw in (dict(audio_format="mp3"), dict(kernel_size=30), dict(margin=0.5)):
        with pytest.raises(ValueError):
            separate("/nonexistent/a.wav", "/nonexistent/out", **kw)


def test_the_library_refuses_bad_arguments_before_any_launch():
    from musicgan_amd import _build, _lib
    _build.build()
    lib = _lib.load()
    p = ctypes.c_void_p(4096)      # never dereferenced: every call below is refused on its arguments
    inf = float("inf")
    assert lib.mg_hpss(None, p, p, None, None, None, None, 8, 31, 31, 2.0, 1.0, 1.0, None) != 0
    assert lib.mg_hpss(p, None, None, None, None, None, None, 8, 31, 31, 2.0, 1.0, 1.0, None) != 0
    for frames, lh, lp, power, mh, mp in ((0, 31, 31, 2.0, 1.0, 1.0), (2 ** 31, 31, 31, 2.0, 1.0, 1.0), (8, 30, 31, 2.0, 1.0, 1.0),
                                          (8, 31, 65, 2.0, 1.0, 1.0), (8, 1, 31, 2.0, 1.0, 1.0), (8, 31, 31, 3.0, 1.0, 1.0),
                                          (8, 31, 31, -inf, 1.0, 1.0), (8, 31, 31, 2.0, 0.5, 1.0), (8, 31, 31, 2.0, 1.0, inf),
                                          (8, 31, 31, 2.0, float("nan"), 1.0)):
        assert lib.mg_hpss(p, p, p, None, None, None, None, frames, lh, lp, power, mh, mp, None) != 0, (frames, lh, lp, power, mh, mp)
    assert b"mg_hpss" in lib.mg_last_error()
    for length, out_len, pp, qq in ((0, 10, 1, 1), (10, -1, 1, 1), (10, 10, 0, 1), (10, 10, 9, 1), (10, 10, 1, 9), (10, 2 ** 40, 1, 1),
                                    (10, 2 ** 39, 2 ** 30, 2 ** 30)):
        assert lib.mg_ola_stretch(p, length, p, out_len, pp, qq, None) != 0, (length, out_len, pp, qq)
    assert lib.mg_ola_stretch(p, 10, None, 0, 1, 1, None) == 0         # nothing to write: no launch


def test_sample_counts_are_unchanged_by_preserve_transients():
    """variant_counts does not know the flag: a variant has ceil(T q / p) frames whichever way its percussive part is re-timed"""
    import inspect
    from musicgan_amd import hpss_ops, ops
    from musicgan_amd.create_dataset import check_variants, variant_counts
    assert "preserve_transients" not in inspect.signature(variant_counts).parameters
    rates, ratios = check_variants((Fraction(9, 10), 2), (1, -12))
    for length in (44100 * 4, 256 * 512, 256 * 512 - 1, 256 * 1024 + 255):
        t0 = 1 + length // 256
        frames = [1 + hpss_ops.stretched_samples(t0, r) // 256 for r in rates]
        for _, f in ratios:
            t1 = 1 + ops.resample_len(length, f.numerator, f.denominator) // 256
            frames.append(1 + hpss_ops.stretched_samples(t1, 1 / f) // 256)
        want = [0 if t < 512 else (t - 1) // 512 for t in [t0] + frames]
        assert variant_counts(length, 512, rates, ratios) == want, (length, want)


def test_command_line():
    from musicgan_amd.__main__ import _FILE_MODES, _MODES, build_parser
    kwargs = _MODES["create_dataset"][4]
    base = ["create_dataset", "in/*.wav", "-o", "out"]
    a = build_parser().parse_args(base)
    assert kwargs(a) == {} and a.component is None and a.preserve_transients is False
    a = build_parser().parse_args(base + ["--stretch", "9/10", "--preserve-transients"])
    assert kwargs(a) == {"stretch": (Fraction(9, 10),), "preserve_transients": True}
    a = build_parser().parse_args(base + ["--component", "harmonic", "--resample"])
    assert kwargs(a) == {"resample": True, "component": "harmonic"}
    assert kwargs(build_parser().parse_args(base + ["--component", "percussive"])) == {"component": "percussive"}
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--component", "tonal"])
    assert "separate" in _FILE_MODES
    module, function, _, call_args, call_kwargs = _FILE_MODES["separate"]
    assert (module, function) == ("separate", "separate")
    a = build_parser().parse_args(["separate", "song.flac", "-o", "parts"])
    assert call_args(a) == ("song.flac", "parts") and call_kwargs(a) == {}
    a = build_parser().parse_args(["separate", "song.flac", "-o", "parts", "--format", "ogg", "--kernel", "17", "--margin", "2", "--resample"])
    assert call_kwargs(a) == {"audio_format": "ogg", "kernel_size": 17, "margin": 2.0, "resample": True}
    for bad in (["--format", "mp3"], ["--kernel", "x"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["separate", "song.flac", "-o", "parts"] + bad)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["separate", "song.flac"])


def test_public_surface():
    import inspect
    from musicgan_amd import audio
    for name in ("hpss", "harmonic", "percussive"):
        assert name in audio.__all__ and callable(getattr(audio, name))
    sig = inspect.signature(audio.hpss).parameters
    assert [(k, v.default) for k, v in list(sig.items())[1:]] == [("kernel_size", 31), ("power", 2.0), ("margin", 1.0), ("mask", False)]
    assert inspect.signature(audio.time_stretch).parameters["preserve_transients"].default is False
    assert inspect.signature(audio.pitch_shift).parameters["preserve_transients"].default is False


def test_abi_and_registers():
    from musicgan_amd import _build, _lib
    header = open(os.path.join(ROOT, "include", "musicgan_hip.h")).read()
    _build.build()
    lib = _lib.load()
    for name in ("mg_hpss", "mg_ola_stretch"):
        assert re.search(rf"\b{name}\s*\(", header) and name in _lib.SIGNATURES and hasattr(lib, name)
    usage = {k: v for k, v in _build.resource_usage().items() if re.search(r"hpss_tile|ola_stretch", k)}
    assert len(usage) == 6, sorted(usage)               # five instantiations of hpss_tile (network sizes, default lengths) and the gather
    for name, u in usage.items():
        assert u.get("VGPRs", 0) > 0, (name, u)
    fast = [u for k, u in usage.items() if "hpss_tileILi32ELi32ELb1E" in k]     # the instantiation for kernel lengths 31 / 31
    assert len(fast) == 1
    assert fast[0].get("ScratchSize [bytes/lane]", 0) == 0, fast[0]   # the windows of the selection network live in registers
    assert all(u.get("ScratchSize [bytes/lane]", 0) == 0 for u in usage.values()), usage
