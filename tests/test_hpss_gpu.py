"""GPU: harmonic / percussive separation and overlap-add re-timing (csrc/hpss.hip, musicgan_amd.hpss_ops, audio.hpss / harmonic /
percussive, time_stretch(..., preserve_transients=True), the component / preserve_transients options of create_dataset and the
`separate` sub-command) against the float64 / NumPy restatement in tests/hpss_ref.py.

The medians are selections and must have the reference's bits.  The bounds for masks, outputs, the sum of the two components and
the overlap-add are derived from the operation counts in tests/hpss_ref.py (MASK 10 u, OUTPUT 11 u |X|, SUM 6 u |X|, OLA 2^-22
(|x1| + |x2|); u = 2^-24) and fitted to nothing; every test prints its figures before it asserts.  References are computed once per
input (hpss_ref.case is cached) and never written to."""
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from musicgan_amd import hpss_ops  # the module under test: without it nothing here can pass

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpss_ref as R  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNELS = [(31, 31), (3, 63), (63, 3), (17, 9)]
assert all(hpss_ops.MIN_KERNEL <= length <= hpss_ops.MAX_KERNEL for kernel in KERNELS for length in kernel)
FRAMES = [1, 5, 16, 40, "tile-1", "tile", "tile+1", "2tile+3"]
MARGINS = [(1.0, 1.0), (2.0, 1.0), (1.0, 3.0)]
RATES = [(1, 1), (9, 10), (11, 10), (1, 8), (8, 1)]
LENGTHS = [1, 255, 256, 257, 256 * 9]
ALL = ("harmonic", "percussive", "H", "P", "mask_h", "mask_p")


def _frames(t):
    if isinstance(t, str):
        from musicgan_amd import hpss_ops
        tile = hpss_ops.TILE
        return {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+3": 2 * tile + 3}[t]
    return t


def _bits(a):
    a = a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return a.contiguous().view(torch.int32)


# ---------------------------------------------------------------- (a) medians, bit for bit
def _medians_body(kind, frames, kernel):
    from musicgan_amd import hpss_ops
    X, ref = R.case(kind, frames, kernel)
    H, P = hpss_ops.hpss(X.to(DEV), kernel, want=("H", "P"))
    assert H.dtype == torch.float32 and H.is_cuda and tuple(H.shape) == (512, frames) == tuple(P.shape)
    bad_h, bad_p = int((_bits(H) != _bits(ref["H"])).sum()), int((_bits(P) != _bits(ref["P"])).sum())
    print(f"MEDIANS {kind} T={frames} {kernel}: {bad_h} of H and {bad_p} of P differ from scipy's")
    assert bad_h == 0 and bad_p == 0
    return [H, P]


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: f"{k[0]}x{k[1]}")
@pytest.mark.parametrize("frames", FRAMES, ids=str)
def test_medians_have_the_bits_of_the_reference(frames, kernel):
    _medians_body("random", _frames(frames), kernel)


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: f"{k[0]}x{k[1]}")
def test_medians_of_tones_and_clicks(kernel):
    _medians_body("tonal_clicks", _frames("2tile+3"), kernel)


def test_silence_gives_masks_of_one_half_and_outputs_of_zero():
    from musicgan_amd import audio, hpss_ops
    X = R.silent_spectrum(40, 0).to(DEV)
    outs = hpss_ops.hpss(X, want=ALL)
    for name, t in zip(ALL, outs):
        want = 0.5 if name.startswith("mask") else 0.0
        assert bool((torch.view_as_real(t) if t.is_complex() else t).eq(want).all()), name
    mh, mp = audio.hpss(X, mask=True)
    assert bool(mh.eq(0.5).all()) and bool(mp.eq(0.5).all())
    mh, mp = audio.hpss(X, margin=(2.0, 1.0), mask=True)         # librosa: an empty bin is split only when both margins are 1
    assert bool(mh.eq(0.0).all()) and bool(mp.eq(0.0).all())


# ---------------------------------------------------------------- (b) masks and outputs against float64
def _masks_body(kind, frames, kernel, power, margin):
    from musicgan_amd import hpss_ops
    X, ref = R.case(kind, frames, kernel, power, margin)
    got = dict(zip(ALL, hpss_ops.hpss(X.to(DEV), kernel, power, margin, want=ALL)))
    assert torch.equal(_bits(got["H"]), _bits(ref["H"])) and torch.equal(_bits(got["P"]), _bits(ref["P"]))
    absx = torch.from_numpy(ref["absX"])
    worst = {}
    for name in ("mask_h", "mask_p"):
        assert got[name].dtype == torch.float32 and tuple(got[name].shape) == (512, frames)
        worst[name] = float((got[name].cpu().double() - torch.from_numpy(ref[name])).abs().max())
    for name in ("harmonic", "percussive"):
        assert got[name].dtype == torch.complex64 and tuple(got[name].shape) == (512, frames)
        err = (got[name].cpu().to(torch.complex128) - torch.from_numpy(ref[name])).abs()
        worst[name] = float((err / (absx * R.OUTPUT_FACTOR + 2.0 ** -126)).max())
    print(f"MASKS {kind} T={frames} {kernel} power {power} margin {margin}: mask errors {worst['mask_h']:.3e} {worst['mask_p']:.3e} "
          f"(bound {R.MASK_BOUND:.3e} = 10 x 2^-24), output errors / (11 x 2^-24 |X|) {worst['harmonic']:.3f} {worst['percussive']:.3f}")
    if power == math.inf:
        for name in ALL:
            want = torch.from_numpy(ref[name])
            assert torch.equal(got[name].cpu(), want.to(got[name].dtype)), name      # exact
    assert worst["mask_h"] <= R.MASK_BOUND and worst["mask_p"] <= R.MASK_BOUND
    assert worst["harmonic"] <= 1.0 and worst["percussive"] <= 1.0
    return [got[name] for name in ALL]


@pytest.mark.parametrize("margin", MARGINS, ids=lambda m: f"m{m[0]:g}_{m[1]:g}")
@pytest.mark.parametrize("power", [1.0, 2.0, math.inf], ids=lambda p: f"p{p:g}")
@pytest.mark.parametrize("kind,kernel", [("random", (31, 31)), ("tonal_clicks", (31, 31)), ("random", (17, 9))],
                         ids=["random-31x31", "tonal_clicks-31x31", "random-17x9"])
def test_masks_and_outputs_against_float64(kind, kernel, power, margin):
    _masks_body(kind, _frames("2tile+3"), kernel, power, margin)


# ---------------------------------------------------------------- (c) the components sum to the input
@pytest.mark.parametrize("power", [1.0, 2.0], ids=lambda p: f"p{p:g}")
@pytest.mark.parametrize("kind", ["random", "tonal_clicks"])
def test_with_margins_of_one_the_components_sum_to_the_input(kind, power):
    from musicgan_amd import audio
    frames = _frames("2tile+3")
    X, ref = R.case(kind, frames, (31, 31), power)
    h, p = audio.hpss(X.to(DEV), power=power)
    err = (h.cpu().to(torch.complex128) + p.cpu().to(torch.complex128) - X.to(torch.complex128)).abs()
    rel = float((err / (torch.from_numpy(ref["absX"]) + 2.0 ** -100)).max())
    print(f"SUM {kind} power {power}: largest |h + p - X| / |X| = {rel:.3e} = {rel / R.U:.2f} x 2^-24 (bound 6 x 2^-24)")
    assert bool((err <= torch.from_numpy(ref["absX"]) * R.SUM_FACTOR + 2.0 ** -126).all())


# ---------------------------------------------------------------- (d) determinism
def test_two_runs_a_replayed_graph_and_an_embedded_spectrum_are_bit_identical():
    from musicgan_amd import hpss_ops
    frames, pad, kernel = 100, 70, (31, 17)      # 70 is no multiple of the tile: the same bins fall into other workgroups
    X = R.random_spectrum(frames, 77).to(DEV)
    a = hpss_ops.hpss(X, kernel, want=ALL)
    b = hpss_ops.hpss(X, kernel, want=ALL)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = hpss_ops.hpss(X, kernel, want=ALL)
    for t in c:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert torch.equal(u, v)
    long = torch.cat([R.random_spectrum(pad, 78).to(DEV), X, R.random_spectrum(300 - frames - pad, 79).to(DEV)], dim=1).contiguous()
    d = hpss_ops.hpss(long, kernel, want=ALL)
    keep = (kernel[0] - 1) // 2 + 1             # further from either end than half the time window
    for name, u, v in zip(ALL, a, d):
        assert torch.equal(u[:, keep:frames - keep], v[:, pad + keep:pad + frames - keep]), name


def test_calls_do_not_synchronise():
    from musicgan_amd import audio, hpss_ops
    X = R.random_spectrum(131, 2131).to(DEV)
    x = R.waveform(256 * 9, 9).to(DEV)
    audio.hpss(X)                                # warm-up: library load
    hpss_ops.ola_stretch(x, 9, 10, 2560)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        h, p = audio.hpss(X, kernel_size=(17, 9), margin=2.0)
        y = hpss_ops.ola_stretch(x, 9, 10, 2560)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(torch.view_as_real(h)).all()) and bool(torch.isfinite(torch.view_as_real(p)).all())
    assert bool(torch.isfinite(y).all())


# ---------------------------------------------------------------- (e) overlap-add re-timing
def _ola_body(length, p, q):
    from musicgan_amd import hpss_ops
    x = R.waveform(length, 10 + length)
    out_len = -((-length * q) // p) + 256        # the stretched length and one hop of what lies past the end
    ref, mass = R.ola(x.numpy(), p, q, out_len)
    y = hpss_ops.ola_stretch(x.to(DEV), p, q, out_len)
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (out_len,)
    err = (y.cpu().double() - torch.from_numpy(ref)).abs()
    bound = torch.from_numpy(mass) * R.OLA_FACTOR
    worst = float((err / (bound + 2.0 ** -100)).max())
    print(f"OLA L={length} {p}/{q} -> {out_len}: largest err {float(err.max()):.3e}, largest err / (2^-22 (|x1| + |x2|)) {worst:.3f}")
    assert bool((err <= bound).all())
    return [y]


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r[0]}_{r[1]}")
def test_ola_stretch_against_the_definition(rate, length):
    _ola_body(length, *rate)


def test_ola_stretch_of_nothing_and_at_rate_one():
    from musicgan_amd import hpss_ops
    x = R.waveform(256 * 9, 10 + 256 * 9).to(DEV)
    assert tuple(hpss_ops.ola_stretch(x, 1, 1, 0).shape) == (0,)
    y = hpss_ops.ola_stretch(x, 3, 3, x.numel() + 100)
    err = float((y[:x.numel()].double() - x.double()).abs().max())
    print(f"OLA IDENTITY: err {err:.3e}, bound {2.0 ** -22 * 3.0:.3e}")
    assert err <= 2.0 ** -22 * float(x.abs().max()) and not bool(y[x.numel():].any())


# ---------------------------------------------------------------- (f) the transient-preserving stretch
def test_time_stretch_preserving_transients_is_its_composition():
    from musicgan_amd import audio, hpss_ops
    x = R.waveform(256 * 40 + 17, 5).to(DEV) * 0.3
    for rate in (Fraction(9, 10), 1.25):
        r = Fraction(rate).limit_denominator(1000)
        plain = audio.time_stretch(x, rate)
        # with the flag off: what the call returned before it had the flag
        assert torch.equal(plain, audio.istft(audio.phase_vocoder(audio.stft_from_waveform(x), rate)))
        assert torch.equal(plain, audio.time_stretch(x, rate, preserve_transients=False))
        got = audio.time_stretch(x, rate, preserve_transients=True)
        assert got.shape == plain.shape and got.dtype == torch.float32 and got.is_cuda
        X = audio.stft_from_waveform(x)
        xh, xp = audio.hpss(X)
        n = math.ceil(X.shape[1] / r)
        assert tuple(got.shape) == (256 * (n - 1),)
        want = audio.istft(audio.phase_vocoder(xh, rate)) + hpss_ops.ola_stretch(audio.istft(xp), r.numerator, r.denominator, 256 * (n - 1))
        assert torch.equal(got, want)
        assert not torch.equal(got, plain)
    assert torch.equal(audio.time_stretch(x.cpu(), Fraction(9, 10), preserve_transients=True),
                       audio.time_stretch(x, Fraction(9, 10), preserve_transients=True))
    for steps in (1, -3.5):
        f = audio.pitch_ratio(steps)
        plain = audio.pitch_shift(x, steps)
        assert torch.equal(plain, audio.pitch_shift(x, steps, preserve_transients=False))
        y = audio.resample(audio.time_stretch(x, 1 / f, preserve_transients=True), f.numerator, f.denominator)
        want = torch.zeros_like(x)
        m = min(x.numel(), y.numel())
        want[:m] = y[:m]
        got = audio.pitch_shift(x, steps, preserve_transients=True)
        assert got.shape == x.shape and torch.equal(got, want), steps
    with pytest.raises(ValueError):
        audio.time_stretch(x[:256 * 2 + 5], 1, preserve_transients=True)  # 3 frames (the STFT takes nothing shorter): istft's error
    with pytest.raises(ValueError):
        audio.time_stretch(x[:256 * 6], 4, preserve_transients=True)     # 7 frames -> n = 2: istft's error


def test_harmonic_and_percussive_are_their_compositions():
    from musicgan_amd import audio
    x = R.waveform(256 * 40 + 17, 6).to(DEV) * 0.3
    X = audio.stft_from_waveform(x)
    h, p = audio.hpss(X)
    assert torch.equal(audio.harmonic(x), audio.istft(h)) and torch.equal(audio.percussive(x), audio.istft(p))
    assert tuple(audio.harmonic(x).shape) == (256 * 40,)
    h2, p2 = audio.hpss(X.cpu(), kernel_size=(17, 9), margin=(1.0, 2.0))          # a CPU tensor is moved to the device
    assert torch.equal(audio.harmonic(x, kernel_size=(17, 9), margin=(1.0, 2.0)), audio.istft(h2)) and h2.is_cuda
    assert torch.equal(audio.percussive(x.cpu(), kernel_size=(17, 9), margin=(1.0, 2.0)), audio.istft(p2))
    mh, mp = audio.hpss(X, mask=True)
    assert mh.dtype == torch.float32 and torch.equal(h, X * mh) and torch.equal(p, X * mp)


# ---------------------------------------------------------------- (g) create_dataset
def _pts(d):
    return sorted((f for f in os.listdir(d) if f.endswith(".pt")), key=lambda f: int(f[len("magn_phase_"):-3]))


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_create_dataset_with_component_and_preserved_transients(tmp_path, monkeypatch):
    import json
    import musicgan_amd
    from musicgan_amd import audio, hpss_ops, ops, pv_ops
    from musicgan_amd.audio import wavio
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    (tmp_path / "wav").mkdir()
    path = str(tmp_path / "wav" / "a.wav")
    wavio.save(path, (R.waveform(256 * 600, 12) * 0.3)[None, :], 44100)          # 601 frames: one sample, and one per variant
    pattern = str(tmp_path / "wav" / "*.wav")
    dirs = {name: str(tmp_path / name) for name in ("plain", "defaults", "harmonic", "variant", "preserved")}
    musicgan_amd.create_dataset(pattern, dirs["plain"])
    musicgan_amd.create_dataset(pattern, dirs["defaults"], component=None, preserve_transients=False)
    # without the two options: every byte written is the same
    names = sorted(os.listdir(dirs["plain"]))
    assert names == sorted(os.listdir(dirs["defaults"])) and _pts(dirs["plain"]) == ["magn_phase_0.pt"]
    for name in names:
        a, b = _read(os.path.join(dirs["plain"], name)), _read(os.path.join(dirs["defaults"], name))
        if name.endswith(".json"):
            assert json.loads(a) == json.loads(b), name
        else:
            assert a == b, name
    pcm = wavio.load_pcm_device(path, torch.device(DEV))
    X = audio.functions.stft_from_pcm(pcm, sample_rate=44100)
    # component: the coded sample is the codec applied to that component
    musicgan_amd.create_dataset(pattern, dirs["harmonic"], component="harmonic")
    want = audio.stft_to_stacked_phase_magn(audio.hpss(X)[0]).double().cpu()
    assert _pts(dirs["harmonic"]) == ["magn_phase_0.pt"] and want.shape[0] == 1
    got = torch.load(os.path.join(dirs["harmonic"], "magn_phase_0.pt"))
    assert torch.equal(got, want[0]) and not torch.equal(got, torch.load(os.path.join(dirs["plain"], "magn_phase_0.pt")))
    # preserve_transients: the sample counts of the plain variant run, the original's samples untouched, the variant its composition
    stretch = (Fraction(9, 10),)
    musicgan_amd.create_dataset(pattern, dirs["variant"], stretch=stretch)
    musicgan_amd.create_dataset(pattern, dirs["preserved"], stretch=stretch, preserve_transients=True)
    assert _pts(dirs["variant"]) == _pts(dirs["preserved"]) == ["magn_phase_0.pt", "magn_phase_1.pt"]
    assert _read(os.path.join(dirs["preserved"], "magn_phase_0.pt")) == _read(os.path.join(dirs["plain"], "magn_phase_0.pt"))
    xh, xp = audio.hpss(X)
    n = pv_ops.phase_vocoder_len(X.shape[1], 9, 10)
    spec = pv_ops.phase_vocoder(xh, 9, 10) + ops.stft_1024(hpss_ops.ola_stretch(audio.istft(xp), 9, 10, 256 * (n - 1)))
    assert spec.shape[1] == n
    want = audio.stft_to_stacked_phase_magn(spec).double().cpu()
    got = torch.load(os.path.join(dirs["preserved"], "magn_phase_1.pt"))
    assert want.shape[0] == 1 and torch.equal(got, want[0])
    assert not torch.equal(got, torch.load(os.path.join(dirs["variant"], "magn_phase_1.pt")))


# ---------------------------------------------------------------- (h) separate
def test_separate_writes_two_readable_files(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.__main__ import main
    from musicgan_amd.audio import wavio
    path = str(tmp_path / "in.wav")
    wavio.save(path, (R.waveform(256 * 40 + 100, 13) * 0.3)[None, :].repeat(2, 1), 44100)   # stereo: the mono mean is separated
    out = tmp_path / "parts"
    main(["separate", path, "-o", str(out)])
    assert sorted(os.listdir(out)) == ["harmonic.wav", "percussive.wav"]
    h, p = audio.hpss(audio.wav_to_stft(path))
    for name, part in (("harmonic", h), ("percussive", p)):
        wav, sr = wavio.load(str(out / f"{name}.wav"))
        assert sr == 44100 and tuple(wav.shape) == (1, 256 * 40)
        assert torch.equal(wav[0], audio.istft(part).cpu())
    main(["separate", path, "-o", str(out), "--format", "flac", "--kernel", "17", "--margin", "2"])
    for name in ("harmonic", "percussive"):
        wav, sr = wavio.load(str(out / f"{name}.flac"))
        assert sr == 44100 and tuple(wav.shape) == (1, 256 * 40) and bool(torch.isfinite(wav).all())


# ---------------------------------------------------------------- (i) poisoned memory
def test_bodies_on_poisoned_memory():
    """the bodies of (a), (b) and (e) under poison.rule pointed at hpss_ops: no guard band damaged by any launch, no argument
    changed, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import hpss_ops

    def run(p):
        t = _frames("2tile+3")
        p.out = (_medians_body("random", 1, (31, 31)) + _medians_body("random", _frames("tile+1"), (3, 63)) +
                 _medians_body("tonal_clicks", t, (63, 3)) + _masks_body("random", t, (31, 31), 2.0, (2.0, 1.0)) +
                 _masks_body("random", t, (17, 9), math.inf, (1.0, 3.0)) +
                 _ola_body(1, 1, 8) + _ola_body(257, 11, 10) + _ola_body(256 * 9, 8, 1))
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=hpss_ops, inplace={})
    for a, b in zip(r0.out, r1.out):
        assert torch.equal(a, b)
    names = [name for name, _, _ in r1.calls]
    assert names.count("hpss") == 5 and names.count("ola_stretch") == 3, names
    print(f"POISON hpss: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")
