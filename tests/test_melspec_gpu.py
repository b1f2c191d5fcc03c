"""GPU: the mel power spectrogram of waveforms and its pooled log rows (csrc/melspec.hip) through musicgan_amd.mel_ops,
audio.mel_spectrogram, metrics.WaveLogMel and the drivers `evaluate_mel_waveform` and `evaluate_audio`.  The kernels are held
against the float64 restatements of tests/melspec_ref.py; tolerances come from a float32 CPU evaluation of the same chain with the
margin 4 of test_griffinlim_gpu.py (another, equally precise summation order), never from the kernel's own figures; every figure is
printed before it is asserted (DESIGN.md 4.21 quotes them)."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import melspec_ref as R  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6
# the tensor arguments the two new wrappers of musicgan_amd/mel_ops.py write (their docstrings)
INPLACE = {
    "mel_power": ("out",),            # "out (B, M, T) float32 ..., every element written"
    "logmel_pool": ("out",),          # "out (B * W, M * pools) float32, every element written"
}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ mel_power: the cases
# name: (rows, samples, samples between two rows beyond L)
SHAPES = {
    "1x1024": (1, 1024, 0),                # T = 5: only frame 2 is interior, two before and two after it reflect
    "1x3841": (1, 256 * 15 + 1, 0),        # T = 16: exactly one tile
    "1x4096": (1, 256 * 16, 0),            # T = 17: a second tile of one frame
    "3x4173_stride": (3, 4096 + 77, 5),    # odd length, rows L + 5 apart: rows 1 starts at an odd sample
    "2x130816": (2, 130816, 0),            # the driver's shape: 512 frames, one window
}


def _waves(name):
    """row 0: seeded uniform noise in [-1, 1]; with three rows, row 1: a full-scale sine at 2 kHz; the last of several rows: zeros.
    Returns the (B, L) tensor as a view of a (B, L + extra) buffer."""
    b, length, extra = SHAPES[name]
    buf = torch.zeros(b, length + extra)
    buf[0, :length] = torch.rand(length, generator=torch.Generator().manual_seed(1000 + length)) * 2 - 1
    if b == 3:
        buf[1, :length] = torch.sin(2 * np.pi * 2000.0 / 44100.0 * torch.arange(length, dtype=torch.float64)).float()
    return buf[:, :length]


def _hand_bank():
    """6 bands in the manner of test_logmel_gpu._hand_case: two of one bin at bins 0 and 511, one of all 512 bins, two over the same
    bins, an empty one.  Weights outside [lo, hi) are NaN: they are never read."""
    gen = torch.Generator().manual_seed(191)
    lo = torch.tensor([0, 511, 0, 37, 37, 200], dtype=torch.int32)
    hi = torch.tensor([1, 512, 512, 101, 101, 200], dtype=torch.int32)
    weight = torch.full((6, 512), float("nan"))
    for m in range(6):
        weight[m, lo[m]:hi[m]] = torch.rand(int(hi[m] - lo[m]), generator=gen)
    return weight, lo, hi


def _bank(name):
    from musicgan_amd import metrics
    if name == "mel64":                    # no empty band; LogMel's bank at level 7
        return metrics.mel_filterbank(512, 64)
    if name == "mel8_300_8000":
        return metrics.mel_filterbank(512, 8, 300.0, 8000.0)
    return _hand_bank()


BANKS = ("mel64", "mel8_300_8000", "hand6")
CASES = [(s, b) for s in SHAPES for b in BANKS]
_REF = {}


def _reference(shape, bank):
    """(waves, (weight, lo, hi), float64 restatement, band scale, error of the float32 CPU evaluation over the scale): computed once
    per case and shared, read-only"""
    if (shape, bank) not in _REF:
        waves = _waves(shape)
        weight, lo, hi = _bank(bank)
        w, l, h = weight.numpy(), lo.tolist(), hi.tolist()
        x = waves.numpy()
        ref = R.mel_power(x, w, l, h)
        scale = R.band_scale(x, w, l, h)
        f32 = R.mel_power_f32(x, w, l, h).astype(np.float64)
        live = scale > 0
        own = float((np.abs(f32 - ref)[:, live] / scale[None, live, None]).max())
        for arr in (ref, scale):
            arr.setflags(write=False)
        _REF[(shape, bank)] = (waves, (weight, lo, hi), ref, scale, own)
    return _REF[(shape, bank)]


def _run(waves, bank, **kw):
    from musicgan_amd import mel_ops
    weight, lo, hi = bank
    dev = torch.zeros(waves.shape[0], waves.stride(0) if waves.shape[0] > 1 else waves.shape[1], device=DEV)
    view = dev[:, :waves.shape[1]]
    view.copy_(waves)
    return mel_ops.mel_power(view, weight.to(DEV), lo, hi, **kw)


def _mel_power_body(shape, bank):
    waves, bk, ref, scale, own = _reference(shape, bank)
    out = _run(waves, bk)
    b, length = waves.shape
    assert out.dtype == torch.float32 and out.is_cuda and tuple(out.shape) == (b, bk[0].shape[0], 1 + length // 256)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    live = scale > 0
    err = float((np.abs(got - ref)[:, live] / scale[None, live, None]).max())
    print(f"mel_power {shape} {bank}: worst err / band scale {err:.3e}, float32 CPU {own:.3e}, ratio {err / own:.3f} (allowed 4); "
          f"band scales {scale[live].min():.3e} .. {scale.max():.3e}")
    assert err <= 4 * own
    assert (_bits(out[:, ~torch.from_numpy(live)]) == 0).all()            # an empty band: exactly +0.0
    if b > 1:                                                            # the row of zeros: exactly +0.0 everywhere
        assert (_bits(out[b - 1]) == 0).all()
        assert float(out[0].max()) > 0.0
    return out


@pytest.mark.parametrize("shape,bank", CASES, ids=[f"{s}-{b}" for s, b in CASES])
def test_mel_power_is_the_float64_definition_within_four_times_a_float32_evaluation(shape, bank):
    _mel_power_body(shape, bank)


@pytest.mark.parametrize("shape,bank", CASES, ids=[f"{s}-{b}" for s, b in CASES])
def test_mel_power_equals_the_unfused_route_bit_for_bit(shape, bank):
    """the definition evaluated in numpy float32 -- explicit products and sums, nothing fused -- over ops.stft_1024 of each row"""
    from musicgan_amd import ops
    waves, bk, _, _, _ = _reference(shape, bank)
    out = _run(waves, bk).cpu().numpy()
    w, lo, hi = bk[0].numpy(), bk[1].tolist(), bk[2].tolist()
    for i in range(waves.shape[0]):
        spec = ops.stft_1024(waves[i].contiguous().to(DEV)).cpu().numpy()
        assert spec.dtype == np.complex64
        want = R.band_sums(R.power_of_bins(spec), w, lo, hi)
        assert want.dtype == np.float32
        assert np.array_equal(out[i].view(np.int32), want.view(np.int32)), (shape, bank, i)


def test_rows_of_a_batch_equal_single_row_calls_and_runs_are_bit_identical():
    for shape in ("3x4173_stride", "2x130816"):
        waves, bk, _, _, _ = _reference(shape, "mel64")
        whole, again = _run(waves, bk), _run(waves, bk)
        assert torch.equal(_bits(whole), _bits(again))
        for i in range(waves.shape[0]):
            alone = _run(waves[i:i + 1], bk)
            assert torch.equal(_bits(alone[0]), _bits(whole[i])), (shape, i)


def test_mel_power_into_a_given_tensor_and_mel_spectrogram():
    from musicgan_amd import audio
    waves, bk, _, _, _ = _reference("3x4173_stride", "mel64")
    want = _run(waves, bk)
    out = torch.empty_like(want)
    assert _run(waves, bk, out=out) is out and torch.equal(_bits(out), _bits(want))
    spec = audio.mel_spectrogram(waves)                                   # host input, default bank = mel64
    assert spec.is_cuda and torch.equal(_bits(spec), _bits(want))
    one = audio.mel_spectrogram(waves[0].double())                        # (L,) float64 -> (64, T)
    assert tuple(one.shape) == (64, 17) and torch.equal(_bits(one), _bits(want[0]))
    stereo = audio.mel_spectrogram(waves[None, :2].contiguous(), n_mels=8, f_min=300.0, f_max=8000.0)
    assert tuple(stereo.shape) == (1, 2, 8, 17)                           # channels are rows, not averaged
    assert torch.equal(_bits(stereo[0]), _bits(_run(waves[:2], _bank("mel8_300_8000"))))


# ------------------------------------------------------------------ logmel_pool
POOLS = [("2x130816", 512, 512, 8), ("2x130816", 512, 512, 32), ("2x130816", 64, 32, 1), ("2x130816", 64, 32, 64),
         ("1x4096", 16, 16, 4)]                                          # the last: T = 17, one window, the tail dropped


def _pool_body(shape, win, hop, pools):
    from musicgan_amd import mel_ops
    waves, bk, _, _, _ = _reference(shape, "mel64")
    power = _run(waves, bk)
    out = mel_ops.logmel_pool(power, win, hop, pools, FLOOR)
    b, m, t = power.shape
    nwin = (t - win) // hop + 1
    assert out.dtype == torch.float32 and tuple(out.shape) == (b * nwin, m * pools)
    ref = R.logmel_pool(power.cpu().numpy(), win, hop, pools, FLOOR)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-12
    worst = float((np.abs(out.cpu().double().numpy() - ref) / bound).max())
    print(f"logmel_pool {shape} win {win} hop {hop} pools {pools}: {nwin} windows, worst err / bound {worst:.4f}; values "
          f"{ref.min():.3f} .. {ref.max():.3f}")
    assert worst <= 1.0
    # a window's row equals the row of the same frames cut out and pooled alone
    for n in sorted({0, nwin // 2, nwin - 1}):
        cut = power[:, :, n * hop:n * hop + win].contiguous()
        alone = mel_ops.logmel_pool(cut, win, win, pools, FLOOR)
        rows = torch.arange(b, device=DEV) * nwin + n
        assert torch.equal(_bits(alone), _bits(out[rows])), n
    return out


@pytest.mark.parametrize("shape,win,hop,pools", POOLS, ids=[f"{s}-{w}-{h}-{p}" for s, w, h, p in POOLS])
def test_logmel_pool_is_the_float64_mean_rounded_once(shape, win, hop, pools):
    out = _pool_body(shape, win, hop, pools)
    if shape == "1x4096":
        assert out.shape[0] == 1


def test_wavelogmel_is_the_two_wrappers():
    from musicgan_amd import mel_ops, metrics
    waves, bk, _, _, _ = _reference("2x130816", "mel64")
    wl = metrics.WaveLogMel(pools=8)
    assert wl.dims == 512 and wl.windows(130816) == 1 and wl.windows(130815) == 0
    rows = wl(waves.to(DEV).contiguous())
    want = mel_ops.logmel_pool(_run(waves, bk), 512, 512, 8, 1e-6)
    assert tuple(rows.shape) == (2, 512) and torch.equal(_bits(rows), _bits(want))
    with pytest.raises(ValueError):
        wl(waves[:, :130815].contiguous().to(DEV))                        # fewer than one window


# ------------------------------------------------------------------ poisoned memory
def test_mel_power_and_pool_on_poisoned_memory():
    """the bodies under poison.rule pointed at mel_ops: no guard band damaged by either launch, no argument changed that the table
    does not name, equal digests under both fills (nothing read that nobody wrote), nothing non-finite in the 0xFF run"""
    from musicgan_amd import mel_ops

    def run(p):
        p.bodies = [_mel_power_body("3x4173_stride", "mel64"), _mel_power_body("1x4096", "hand6"),
                    _mel_power_body("1x1024", "mel8_300_8000"), _pool_body("1x4096", 16, 16, 4), _pool_body("2x130816", 64, 32, 64)]
        waves, bk, _, _, _ = _reference("3x4173_stride", "mel64")
        power = torch.empty(3, 64, 17, device=DEV)                        # given outputs: written in place, every element
        rows = torch.empty(3, 64 * 4, device=DEV)
        _run(waves, bk, out=power)
        mel_ops.logmel_pool(power, 16, 16, 4, FLOOR, out=rows)
        p.bodies += [power, rows]
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=mel_ops, inplace=INPLACE)
    for a, b in zip(r0.bodies, r1.bodies):
        assert torch.equal(_bits(a), _bits(b))
    names = {name for name, _, _ in r1.calls}
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    assert {"mel_power", "logmel_pool"} <= names, names
    print(f"POISON melspec: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


# ------------------------------------------------------------------ the point of the feature
def _signal(length):
    """five sinusoids and one click, seeded"""
    gen = torch.Generator().manual_seed(77)
    t = torch.arange(length, dtype=torch.float64)
    x = torch.zeros(length, dtype=torch.float64)
    for f in (220.0, 440.0, 1000.0, 3300.0, 7000.0):
        x += 0.15 * torch.sin(2 * np.pi * f / 44100.0 * t + float(torch.rand(1, generator=gen)) * 6.28)
    x[length // 2] += 0.8
    return x.float()


def test_phase_changes_the_waveform_rows_and_not_the_image_rows():
    """One (2, 512, 512) image made by the codec from a seeded signal, and its copy with channel 1 (the phase deltas) replaced by
    seeded uniform values.  The signal has 131 072 samples: the codec's first difference drops a frame, so an image of 512 frames
    needs 513 (130 816 samples, 512 frames, would give no image); what the image decodes to has 130 816 samples."""
    from musicgan_amd import audio, metrics
    from oracle import audio as O
    spec = audio.stft_from_waveform(_signal(131072).to(DEV))
    image = audio.stft_to_stacked_phase_magn(spec)
    assert tuple(image.shape) == (1, 2, 512, 512)
    other = image.clone()
    other[0, 1] = (torch.rand(512, 512, generator=torch.Generator().manual_seed(78)) * 2 - 1).to(DEV)
    lm = metrics.LogMel(512, 512)
    assert torch.equal(_bits(lm(image)), _bits(lm(other)))               # the image rows cannot see it
    wl = metrics.WaveLogMel()
    w, lo, hi = wl.weight.numpy(), wl.lo.tolist(), wl.hi.tolist()
    refs, gpu = [], []
    for x in (image, other):
        host = x[0].cpu().numpy()
        ref = R.wave_logmel(R.magn_phase_to_wave(host)[None], w, lo, hi, 512, 512, 32, FLOOR)
        f32 = R.wave_logmel(O.magn_phase_to_wav(host[None])[None], w, lo, hi, 512, 512, 32, FLOOR, np.float32)
        wave = audio.magn_phase_to_waveform(x)
        assert tuple(wave.shape) == (130816,)
        got = wl(wave[None].contiguous())
        assert tuple(got.shape) == (1, 64 * 32)
        own = float(np.abs(f32 - ref).max())
        err = float(np.abs(got.cpu().double().numpy() - ref).max())
        print(f"WaveLogMel of the decoded image: worst |gpu - float64| {err:.3e}, float32 CPU {own:.3e}, ratio {err / own:.3f} "
              f"(allowed 4)")
        refs.append(ref)
        gpu.append((err, own))
    # a condition on the input, asserted on the reference alone: the two images must differ by far more than the parity tolerance
    parity = 4 * _reference("2x130816", "mel64")[4]
    moved = float(np.abs(refs[0] - refs[1]).mean())
    print(f"scrambling the phase moves the float64 waveform rows by {moved:.4f} nat on average (largest "
          f"{float(np.abs(refs[0] - refs[1]).max()):.4f}); 100 x the parity tolerance of mel_power: {100 * parity:.3e}")
    assert moved >= 100 * parity
    for err, own in gpu:
        assert err <= 4 * own


# ------------------------------------------------------------------ evaluate_mel_waveform
WAVE_METRICS = ("fd", "kid", "nn")
WAVE_KW = dict(level=7, nb_images=8, seed=1)


def _quiet(fn, *args, **kw):
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        result = fn(*args, **kw)
    return result, text.getvalue()


@pytest.fixture(scope="module")
def corpus7(tmp_path_factory):
    """8 dataset entries of 512 x 512, a generator at level 7, and the waveform run at batch size 3 with its text: made once"""
    import musicgan_amd
    root = tmp_path_factory.mktemp("melspec")
    data_dir, ck = tiny_corpus(root, files=4, seed=17, level=7)
    fn, plain = musicgan_amd.__getattr__("evaluate_mel_waveform"), musicgan_amd.__getattr__("evaluate_mel")
    full, text = _quiet(fn, ck, 8, data_dir, WAVE_METRICS, batch_size=3, **WAVE_KW)
    return dict(root=root, data=data_dir, ck=ck, fn=fn, plain=plain, full=full, text=text)


def test_evaluate_mel_scores_the_waveforms(corpus7):
    fn, ck, data, full, text = (corpus7[k] for k in ("fn", "ck", "data", "full", "text"))
    print(text)
    plain, plain_text = _quiet(corpus7["plain"], ck, 8, data, WAVE_METRICS, batch_size=3, **WAVE_KW)
    assert list(full) == list(plain) and len(full) == 3 + 4 + 5           # the keys of the plain run, in its order
    assert all(isinstance(v, float) and np.isfinite(v) for v in full.values()), full
    assert all(full[k] != plain[k] for k in ("fd", "fd_real", "nn_fake", "nn_real", "kid_full")), (full, plain)
    assert "in waveform log-mel space (64 bands x 8 pools)" in text and "in waveform log-mel space (64 bands x 32 pools)" in text
    assert "waveform" not in plain_text and "in log-mel space (64 bands x 8 pools)" in plain_text
    assert text.count("waveform log-mel space") == plain_text.count("log-mel space")
    again, text2 = _quiet(fn, ck, 8, data, WAVE_METRICS, batch_size=3, **WAVE_KW)
    assert again == full and text2 == text                                # from run to run
    # the real side does not depend on the batch size, nor does kid (its generated images come in batches of 16 whatever it is)
    other, _ = _quiet(fn, ck, 8, data, WAVE_METRICS, batch_size=8, **WAVE_KW)
    fixed = [k for k in full if k.endswith("_real") or k.startswith(("nn_real", "kid"))]
    assert len(fixed) == 1 + 2 + 5
    assert {k: other[k] for k in fixed} == {k: full[k] for k in fixed}


def test_evaluate_mel_with_griffin_lim_moves_the_generated_side_only(corpus7):
    fn, ck, data, full = (corpus7[k] for k in ("fn", "ck", "data", "full"))
    gl, _ = _quiet(fn, ck, 8, data, ("fd",), batch_size=3, griffin_lim=2, **WAVE_KW)
    assert gl["fd_real"] == full["fd_real"] and gl["fd"] != full["fd"] and np.isfinite(gl["fd"])


# ------------------------------------------------------------------ evaluate_audio
WINDOW = 130816


def _write_sets(root):
    """two directories of three seeded mono wav files of two windows each (every window at a level of its own), a file shorter than
    one window in the first, and 24-bit FLAC copies of the first directory's files"""
    from musicgan_amd.audio import wavio
    gen = torch.Generator().manual_seed(31)
    dirs = {name: root / name for name in ("real", "other", "copies")}
    for d in dirs.values():
        d.mkdir()
    for name in ("real", "other"):
        for i in range(3):
            wave = torch.rand(2 * WINDOW + 300, generator=gen) - 0.5
            if name == "other":
                wave = (wave + torch.roll(wave, 1)) / 2                  # another spectrum: a two-tap low-pass
            wave[:WINDOW] *= 0.05 + float(torch.rand(1, generator=gen))
            wave[WINDOW:] *= 0.05 + float(torch.rand(1, generator=gen))
            wavio.save(str(dirs[name] / f"f{i}.wav"), wave[None], 44100)
            if name == "real":
                wavio.save(str(dirs["copies"] / f"f{i}.flac"), wave[None], 44100)
    wavio.save(str(dirs["real"] / "short.wav"), torch.rand(1, WINDOW - 256, generator=gen) - 0.5, 44100)
    return {k: str(v) for k, v in dirs.items()}


@pytest.fixture(scope="module")
def audio_sets(tmp_path_factory):
    return _write_sets(tmp_path_factory.mktemp("audiosets"))


def test_evaluate_audio_compares_two_sets_of_files(audio_sets, tmp_path):
    import musicgan_amd
    from musicgan_amd import metrics
    from musicgan_amd.audio import wavio
    fn = musicgan_amd.__getattr__("evaluate_audio")
    real, other = audio_sets["real"] + "/*.wav", audio_sets["other"] + "/*.wav"
    js = str(tmp_path / "audio.json")
    result, text = _quiet(fn, real, other, ("fd", "kid", "nn"), output=js)
    print(text)
    with open(js) as f:
        assert json.load(f) == result
    assert list(result) == ["fd", "fd_half", "fd_real", "nn_fake", "nn_real", "nn_fake_min", "nn_real_min", "kid", "kid_std",
                            "kid_full", "kid_real", "kid_real_std"]
    assert all(np.isfinite(v) for v in result.values()), result
    assert np.isfinite(result["fd_real"]) and np.isfinite(result["kid_real"])          # the two real-half figures
    assert "too short" in text and "short.wav" in text and "real: 6 windows of 3 of 4 files" in text
    assert "other: 6 windows of 3 of 3 files" not in text and "fake: 6 windows of 3 of 3 files" in text
    assert "in waveform log-mel space (64 bands x 8 pools)" in text
    assert _quiet(fn, real, other, ("fd", "kid", "nn"))[0] == result
    # The squared MMD is symmetric in its two sets, and poly_mmd2 of the two sets' rows is, to float64 rounding.  evaluate_audio's
    # kid_full is NOT: metrics.KID standardises both sets by the moments of the FIRST one, so swapping the globs
    # changes the rows the kernel sees.  Both figures are printed; the symmetry is asserted where it holds.
    swapped, _ = _quiet(fn, other, real, ("kid",))
    print(f"kid_full {result['kid_full']:.6f}, globs swapped {swapped['kid_full']:.6f}")
    assert np.isfinite(swapped["kid_full"])
    wl = metrics.WaveLogMel(pools=8)
    rows = []
    for d in ("real", "other"):
        waves = torch.stack([wavio.load(f"{audio_sets[d]}/f{i}.wav")[0][0, :2 * WINDOW] for i in range(3)]).to(DEV)
        rows.append(wl(waves.reshape(6, WINDOW).contiguous()))
    ab, ba = metrics.poly_mmd2(rows[0], rows[1]), metrics.poly_mmd2(rows[1], rows[0])
    print(f"poly_mmd2 of the two sets' rows {ab:.9e}, swapped {ba:.9e}")
    assert abs(ab - ba) <= 1e-12 * max(abs(ab), 1.0)
    with pytest.raises(FileNotFoundError):
        fn(audio_sets["real"] + "/*.mp3", other)
    with pytest.raises(ValueError):
        fn(real, audio_sets["real"] + "/short.wav")                       # no window at all: fewer than fd's four


def test_evaluate_audio_of_files_and_their_flac_copies_is_zero_up_to_quantisation(audio_sets):
    """the .wav files against their 24-bit FLAC copies (wavio.save): a window's nearest neighbour is its own copy.  What "0" is:
    the copy's samples are off by at most 2^-24, far below what float32 rows hold, and nn's distance |q|^2 + |r|^2 - 2 q.r takes the
    dot product in float32 chunks of 256, an error of at most 2 gamma_264 |q| |r| in d, so the per-component RMS
    of a window against its copy is at most sqrt(2 gamma_264) x the rows' RMS value (+ 1e-5 for the quantisation)."""
    import musicgan_amd
    from musicgan_amd import metrics
    from musicgan_amd.audio import wavio
    fn = musicgan_amd.__getattr__("evaluate_audio")
    result, text = _quiet(fn, audio_sets["real"] + "/f*.wav", audio_sets["copies"] + "/*.flac", ("fd", "nn"))
    waves = torch.stack([wavio.load(f"{audio_sets['real']}/f{i}.wav")[0][0, :2 * WINDOW] for i in range(3)]).to(DEV)
    rows = metrics.WaveLogMel()(waves.reshape(6, WINDOW).contiguous())
    rms = float(rows.double().pow(2).mean(1).sqrt().max())
    gamma = 264 * 2.0 ** -24 / (1 - 264 * 2.0 ** -24)
    bound = (2 * gamma) ** 0.5 * rms + 1e-5
    print(f"wav against its flac copies: nn_fake_min {result['nn_fake_min']:.3e} (bound {bound:.3e}, rows' RMS {rms:.3f}), nn_real_min "
          f"{result['nn_real_min']:.3e}; fd {result['fd']:.3e}, fd_real {result['fd_real']:.3e}")
    assert result["nn_fake_min"] <= bound and result["nn_fake"] <= bound and result["nn_real_min"] > bound
    assert result["fd"] <= 1e-3 * result["fd_real"]
