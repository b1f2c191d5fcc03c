"""GPU: the look-ahead true-peak limiter (csrc/limiter.hip) against the float64 numpy restatement of tests/limiter_ref.py -- the
envelope, the gain curve around every boundary of the tiles (the hold's right halo, the mean's left halo, the release carried along
the file), the guarantees that hold by construction, `normalize_loudness(limiter=True)`, capture in a graph, and the way from a
checkpoint to a file through `generate(..., limiter=True)`.  T = lim_ops.TILE.

Bounds.
m: bit for bit the maximum over `ops.resample_rows(x, 1, 4)` of the same tensor on the device (the same sums in the same order) and
  of |x|; within 1e-6 max|x| of the float64 evaluation of the bank, what tests/test_resample_gpu.py grants the resampler.
g: 1e-8 absolute against the restatement run on the device's m.  Both sides are float64.  The release is a chain of at most about
  81 000 products by rho that matter (rho^k < 2^-53 beyond), each within 2^-53: 1e-11.  The window sums are differences of a prefix
  sum over at most T + A terms of at most 1, restarted in every tile: at most (T + A)^2 2^-53 = 1.9e-9 in the worst case, divided by
  A + 1.  A dropped carry, a window shifted by one sample or a missing halo moves g by more than 1e-4 on these inputs (each case
  asserts that its input makes the limiter work where it is meant to).
y: relative 2^-22 against float32(double(x) G g) of the restatement: one float32 rounding either way.
By construction, asserted on every case: |y| <= c (1 + 2^-23); g == 1 exactly and y == float32(double(x) G) bit for bit where
G m <= c everywhere."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limiter_ref as LR  # noqa: E402
import loudness_ref as R  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C0 = 10 ** (-1.0 / 20)              # -1 dBTP
RHO = math.exp(-1.0 / 2205.0)       # 50 ms at 44.1 kHz
LOOKAHEADS = [0, 1, 220, 2047]


def _tile():
    from musicgan_amd import lim_ops
    return lim_ops.TILE


@functools.lru_cache(maxsize=None)
def _spiky(channels, length, seed):
    """noise at 0.05 with a spike of up to 3 about every 300 samples (at least one)"""
    rng = np.random.default_rng(seed)
    x = 0.05 * rng.standard_normal((channels, length))
    n = max(1, length // 300)
    x[rng.integers(0, channels, n), rng.integers(0, length, n)] = rng.uniform(1.0, 3.0, n) * rng.choice([-1.0, 1.0], n)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def _envelope_from_the_resampler(xd):
    """step 1 on the device from the resampler's own output: max over the channels of max(|x[n]|, |u[4n - 3 .. 4n + 3]|)"""
    from musicgan_amd import ops
    au = ops.resample_rows(xd, 1, 4).abs()
    assert au.shape == (xd.shape[0], 4 * xd.shape[1])
    win = torch.nn.functional.pad(au, (3, 3)).unfold(1, 7, 4)      # window n = au[4n - 3 .. 4n + 3]
    assert win.shape[1] == xd.shape[1]
    return torch.maximum(xd.abs(), win.max(dim=2).values).max(dim=0).values


def _check(x, G, A, rho=RHO, c=C0, xd=None, what="", active=None):
    """envelope, gain curve, output and the construction bound of one case; returns (y, g, reference curve).  active: a slice of
    samples in which the reference must reduce the gain by more than 1e-3 (the case is then not a passthrough in disguise)."""
    from musicgan_amd import lim_ops
    if xd is None:
        xd = torch.from_numpy(np.array(x)).to(DEV)
    m = lim_ops.envelope(xd)
    assert m.dtype == torch.float32 and m.shape == (x.shape[1],)
    assert torch.equal(m, _envelope_from_the_resampler(xd)), what
    top = float(np.abs(x).max())
    assert np.max(np.abs(m.cpu().numpy().astype(np.float64) - LR.envelope(x))) <= 1e-6 * top, what
    pre = torch.full((1,), G, dtype=torch.float64, device=DEV)
    y, g = lim_ops.limit(xd, pre, c, A, rho, return_gain=True)
    assert y.dtype == torch.float32 and y.shape == xd.shape and y.is_contiguous() and g.dtype == torch.float64 and g.shape == m.shape
    assert torch.equal(lim_ops.limit(xd, pre, c, A, rho), y), what          # without the curve: the same output
    ref = LR.gain_curve(m.cpu().numpy(), G, c, A, rho)
    err = float(np.max(np.abs(g.cpu().numpy() - ref["g"])))
    want = ((x.astype(np.float64) * G) * ref["g"][None, :]).astype(np.float32)
    got = y.cpu().numpy()
    rel = np.abs(got.astype(np.float64) - want) - 2.0 ** -22 * np.abs(want)
    print(f"LIMIT {what}: C {x.shape[0]} L {x.shape[1]} A {A}: g error {err:.2e}, least g {ref['g'].min():.4f}, "
          f"|y| max / c {np.abs(got).max() / c:.9f}")
    assert err <= 1e-8, (what, err)
    assert rel.max() <= 1e-44, (what, float(rel.max()))
    assert np.abs(got).max() <= c * (1 + 2.0 ** -23), what
    if active is not None:
        assert (1.0 - ref["g"][active]).max() > 1e-3, what
    return y, g, ref


def _lengths(A):
    T = _tile()
    return sorted({1, max(A, 1), A + 1, T - 1, T, T + 1, 3 * T + 17, 40 * T + 5})


@pytest.mark.parametrize("A", LOOKAHEADS)
def test_lengths_around_the_tile_and_the_window(A):
    """L < A, L = A, windows longer than the file and windows that reach into the next tile"""
    for length in _lengths(A):
        x = _spiky(2, length, 1000 + length % 997)
        _check(x, 1.5, A, what=f"length {length}", active=slice(None))


@pytest.mark.parametrize("A", [220, 2047])
def test_spikes_at_tile_borders(A):
    """one spike on quiet noise: the gain must fall before it (the hold looks A samples to the right, over the tile's border), hold
    across it and recover after it (the mean looks A samples to the left); two spikes A + 1 and A apart: one window of the hold
    holds both or only one"""
    T = _tile()
    length = 2 * T + 300
    rng = np.random.default_rng(5)
    base = (0.01 * rng.standard_normal((1, length))).astype(np.float32)
    singles = {"sample 0": [0], "sample L-1": [length - 1], "sample T-1": [T - 1], "sample T": [T]}
    pairs = {"A+1 apart": [T - 5, T - 5 + A + 1], "A apart": [T - 5, T - 5 + A]}
    for name, where in {**singles, **pairs}.items():
        x = base.copy()
        x[0, where] = 4.0
        lo, hi = max(0, where[0] - A), min(length, where[-1] + A + 1)
        y, g, ref = _check(x, 1.0, A, what=f"spike at {name}", active=slice(lo, hi))
        gq = ref["g"]
        assert gq[where[0]] <= C0 / 4.0 and np.all(np.diff(gq[lo:where[0] + 1]) <= 0)         # falls towards the spike
        if lo > 1:   # and not earlier: the sample before the spike counts the interpolated points next to it, so A + 1 before it
            assert gq[lo - 2] == 1.0 and gq[lo - 1] < 1.0
    # a spike at sample 0 meets a gain that fell during the A silent samples before the file
    x = base.copy()
    x[0, 0] = 4.0
    _, g, _ = _check(x, 1.0, A, what="start of file")
    assert float(g[0]) <= C0 / 4.0


@pytest.mark.parametrize("release_ms", [50.0, 1.0])
def test_release_is_carried_over_many_tiles(release_ms):
    """one spike of 8 c, then 100 000 quiet samples: at 50 ms the release is still above 1e-4 four tiles later, at 1 ms it is over
    within the spike's own tile"""
    T = _tile()
    rho = math.exp(-1.0 / (release_ms * 44.1))
    rng = np.random.default_rng(8)
    x = (0.001 * rng.standard_normal((1, 1000 + 100000))).astype(np.float32)
    x[0, 1000] = 8.0 * C0
    _, g, ref = _check(x, 1.0, 220, rho=rho, what=f"release {release_ms} ms", active=slice(780, 1001))
    gq = g.cpu().numpy()
    if release_ms == 50.0:
        assert 1.0 - gq[1000 + 4 * T] > 1e-4 and np.all(np.diff(gq[1300:1300 + 6 * T]) >= -1e-9)
    else:
        assert gq[1000 + T] == 1.0


def test_release_is_carried_over_more_tiles_than_the_carry_has_threads():
    """600 000 samples are 293 tiles: two to a thread of the carry along the file; at a release of 2 s the spike at the start still
    holds the gain down by more than 1e-3 at the end"""
    from musicgan_amd import lim_ops
    rho = math.exp(-1.0 / (2000.0 * 44.1))
    length = 600000
    assert -(-length // lim_ops.TILE) > 256
    x = np.zeros((1, length), np.float32)
    x[0, 500] = 8.0 * C0
    x[0, 300000] = 2.0 * C0
    _, g, ref = _check(x, 1.0, 220, rho=rho, what="293 tiles", active=slice(length - 10, length))
    assert 1.0 - float(g[-1]) > 1e-3


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_channels_share_one_gain_and_row_strides_do_not_matter(channels):
    T = _tile()
    length = T + 333
    rng = np.random.default_rng(channels)
    x = (0.02 * rng.standard_normal((channels, length))).astype(np.float32)
    x[channels - 1, T - 2] = -3.0                                  # the only peak, in the last channel
    wide = torch.zeros(channels, length + 100, device=DEV)
    wide[:, 50:-50] = torch.from_numpy(x).to(DEV)
    view = wide[:, 50:-50]
    assert view.stride(0) == length + 100
    y, g, ref = _check(x, 1.0, 220, what=f"{channels} channels", active=slice(T - 222, T))
    y2, g2, _ = _check(x, 1.0, 220, xd=view, what=f"{channels} channels, row stride {length + 100}")
    assert torch.equal(y, y2) and torch.equal(g, g2)
    # the first channel is scaled by the gain that the last channel asked for
    first = (x[0].astype(np.float64) * g.cpu().numpy()).astype(np.float32)
    assert np.array_equal(y[0].cpu().numpy(), first) and (channels == 1 or not np.array_equal(first, x[0]))


def test_below_the_ceiling_nothing_moves_and_silence_stays_silent():
    from musicgan_amd import audio, lim_ops
    T = _tile()
    x = _spiky(2, 3 * T + 17, 77)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    top = float(lim_ops.envelope(xd).max())
    for G in (0.999 * C0 / top, 0.25):
        y, g, _ = _check(x, G, 220, what=f"passthrough G {G:.3f}")
        assert torch.equal(g, torch.ones_like(g))
        assert torch.equal(y, (xd.double() * G).float())
    y, g = audio.limit(xd, 44100, gain_db=20 * math.log10(0.25), return_gain=True)
    assert torch.equal(g, torch.ones_like(g)) and torch.equal(y, (xd.double() * 10.0 ** (20 * math.log10(0.25) / 20.0)).float())
    z = torch.zeros(2, T + 9, device=DEV)
    y, g = audio.limit(z, 44100, gain_db=30.0, return_gain=True)
    assert not y.any() and torch.equal(g, torch.ones_like(g))
    # shapes: (L,) in, (L,) out; a CPU tensor is moved to the device; nothing at all in, nothing out
    mono = audio.limit(torch.from_numpy(np.array(x[0])), 44100, gain_db=6.0)
    assert mono.is_cuda and mono.shape == (x.shape[1],) and mono.dtype == torch.float32
    assert torch.equal(mono, audio.limit(xd[:1], 44100, gain_db=6.0)[0])
    assert audio.limit(torch.zeros(2, 0), 44100).shape == (2, 0)


def test_audio_limit_is_the_restatement_at_its_defaults():
    """gain_db, ceiling_dbtp, attack_ms and release_ms reach the kernels as 10^(dB / 20), round(ms fs / 1000), exp(-1 / (ms fs / 1000))"""
    from musicgan_amd import audio, lim_ops
    x = _spiky(2, 5000, 3)
    xd = torch.from_numpy(np.array(x)).to(DEV)
    m = lim_ops.envelope(xd).cpu().numpy()
    for fs, kw in ((44100, {}), (48000, dict(ceiling_dbtp=-3.0, gain_db=4.0, attack_ms=1.5, release_ms=20.0))):
        c, A, rho = LR.parameters(fs, kw.get("ceiling_dbtp", -1.0), kw.get("attack_ms", 5.0), kw.get("release_ms", 50.0))
        y, g = audio.limit(xd, fs, return_gain=True, **kw)
        ref = LR.gain_curve(m, 10.0 ** (kw.get("gain_db", 0.0) / 20.0), c, A, rho)
        assert np.max(np.abs(g.cpu().numpy() - ref["g"])) <= 1e-8 and ref["g"].min() < 0.5
        assert float(y.abs().max()) <= c * (1 + 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def _normalised_reference(target):
    x = LR.prototype_signal(0)
    x.setflags(write=False)
    return x, LR.normalize(x, 44100, target)


def test_normalisation_with_the_limiter_reaches_what_the_restatement_reaches():
    """the prototype's signal, 2 s at 44.1 kHz, at a target for which the one-gain rule is peak-bound by several dB"""
    from musicgan_amd import audio
    target = -20.0
    x, ref = _normalised_reference(target)
    assert ref["static_lufs"] < target - 3.0 and ref["reduction_db"] > 3.0          # the ceiling binds, the limiter works
    xd = torch.from_numpy(np.array(x)).to(DEV)
    out, gain, (lufs, peak_db, reduction) = audio.normalize_loudness(xd, 44100, target_lufs=target, limiter=True, return_gain=True,
                                                                     return_details=True)
    assert out.shape == xd.shape and out.dtype == torch.float32 and gain.dtype == torch.float32 and gain.dim() == 0
    assert all(v.is_cuda and v.dtype == torch.float64 and v.dim() == 0 for v in (lufs, peak_db, reduction))
    plain = audio.normalize_loudness(xd, 44100, target_lufs=target)
    lufs_plain = float(audio.loudness(plain, 44100))
    c = 10 ** (-1.0 / 20)
    print(f"NORMALISE with the limiter: {float(lufs):.6f} LUFS (reference {ref['lufs']:.6f}, target {target}), {float(peak_db):.6f} dBTP "
          f"(reference {ref['peak_dbtp']:.6f}), reduction {float(reduction):.3f} dB (reference {ref['reduction_db']:.3f}); one gain: "
          f"{lufs_plain:.6f} LUFS (reference {ref['static_lufs']:.6f}); pre-gain x trim {float(gain):.6f}")
    assert abs(float(lufs) - ref["lufs"]) <= 1e-4 and abs(float(peak_db) - ref["peak_dbtp"]) <= 1e-4
    assert abs(float(reduction) - ref["reduction_db"]) <= 1e-4
    assert abs((float(lufs) - lufs_plain) - (ref["lufs"] - ref["static_lufs"])) <= 1e-4 and float(lufs) > lufs_plain + 3.0
    assert float(lufs) == float(audio.loudness(out, 44100)) and abs(float(peak_db) - 20 * math.log10(float(audio.true_peak(out)))) <= 1e-12
    # the sample bound and, after the trim, the ceiling as the project's own true peak measures it
    assert float(out.abs().max()) <= c * (1 + 2.0 ** -23)
    assert float(audio.true_peak(out)) <= c * (1 + 4 * 2.0 ** -23)
    # passes: one pass is the first iterate, and more passes come closer to the target on this signal
    one = LR.normalize(x, 44100, target, passes=1)
    got1 = float(audio.loudness(audio.normalize_loudness(xd, 44100, target_lufs=target, limiter=True, passes=1), 44100))
    assert abs(got1 - one["lufs"]) <= 1e-4 and abs(target - float(lufs)) < abs(target - got1)
    # (L,) in, (L,) out, the same samples
    assert torch.equal(audio.normalize_loudness(xd[0], 44100, target_lufs=target, limiter=True), out[0])


def test_trim_holds_the_ceiling_on_every_case_it_is_given():
    from musicgan_amd import audio, lim_ops, loud_ops
    for length, A in ((_tile() + 1, 220), (3 * _tile() + 17, 37)):
        xd = torch.from_numpy(np.array(_spiky(2, length, 31))).to(DEV)
        y = lim_ops.limit(xd, torch.full((1,), 2.0, dtype=torch.float64, device=DEV), C0, A, RHO)
        peak = loud_ops.true_peak(y)
        out = lim_ops.trim(y, peak, C0)
        t = min(1.0, C0 / float(peak))
        assert torch.equal(out, (y.double() * t).float())
        print(f"TRIM: true peak {float(peak) / C0:.9f} c before, {float(audio.true_peak(out)) / C0:.9f} c after")
        assert float(audio.true_peak(out)) <= C0 * (1 + 4 * 2.0 ** -23)
        # a ceiling that the waveform passes: the factor is below 1 and the true peak lands on the ceiling
        for low in (0.5 * C0, 0.3):
            out = lim_ops.trim(y, peak, low)
            assert torch.equal(out, (y.double() * (low / float(peak))).float()) and low / float(peak) < 1.0
            after = float(audio.true_peak(out))
            print(f"TRIM to {low:.4f}: true peak {after / low:.9f} of it")
            assert low * (1 - 4 * 2.0 ** -23) <= after <= low * (1 + 4 * 2.0 ** -23)


def test_without_the_limiter_nothing_moves():
    from musicgan_amd import audio
    x = torch.from_numpy(np.array(LR.prototype_signal(1))).to(DEV)
    for kw in ({}, {"target_lufs": -20.0, "peak_dbtp": -2.0}):
        a = audio.normalize_loudness(x, 44100, return_gain=True, **kw)
        b = audio.normalize_loudness(x, 44100, return_gain=True, limiter=False, attack_ms=1.0, release_ms=7.0, passes=3, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        out, gain, (lufs, peak_db, reduction) = audio.normalize_loudness(x, 44100, return_gain=True, return_details=True, **kw)
        assert torch.equal(out, a[0]) and float(reduction) == 0.0 and float(lufs) == float(audio.loudness(out, 44100))
    mp = (torch.rand(1, 2, 512, 128, generator=torch.Generator().manual_seed(12)) * 2 - 1).to(DEV)
    assert torch.equal(audio.magn_phase_to_waveform(mp, loudness=-14), audio.magn_phase_to_waveform(mp, loudness=-14, limiter=False))


def test_runs_are_bit_identical_and_a_captured_graph_follows_the_pregain():
    from musicgan_amd import audio, lim_ops
    T = _tile()
    x = torch.from_numpy(np.array(_spiky(2, 5 * T + 123, 42))).to(DEV)
    a, b = audio.limit(x, 44100, gain_db=3.0, return_gain=True), audio.limit(x, 44100, gain_db=3.0, return_gain=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[1].min()) < 0.5
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = audio.limit(x, 44100, gain_db=3.0, return_gain=True)
    c[0].zero_()
    c[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
    # the pre-gain is device memory: rewritten between two replays, the same graph limits to the new level
    pre = torch.full((1,), 1.0, dtype=torch.float64, device=DEV)
    eager = [lim_ops.limit(x, torch.full((1,), G, dtype=torch.float64, device=DEV), C0, 220, RHO) for G in (1.0, 2.5)]
    assert not torch.equal(eager[0], eager[1])
    torch.cuda.synchronize()
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        y = lim_ops.limit(x, pre, C0, 220, RHO)
    for G, want in zip((1.0, 2.5), eager):
        pre.fill_(G)
        graph2.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, want)


def test_generate_with_the_limiter_writes_a_file_at_the_restatements_loudness(tmp_path):
    """from a checkpoint to a file and back: the file that `generate --loudness --limiter` writes measures what the restatement
    reaches from the file written without normalisation, and stays under the ceiling; without the limiter the bytes are the old ones"""
    from musicgan_amd import audio
    from musicgan_amd.__main__ import main
    from musicgan_amd.audio import wavio
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    ck = str(tmp_path / "gen7.pt")
    torch.save(Generator(8, end_layer=7).state_dict(), ck)
    target = -14.0
    for name, extra in (("plain", []), ("loud", ["--loudness", str(target)]), ("limited", ["--loudness", str(target), "--limiter"]),
                        ("fast", ["--loudness", str(target), "--limiter", "--limiter-attack", "1", "--limiter-release", "10"])):
        main(["generate", ck, "8", "-n", "1", "-m", "1", "-o", str(tmp_path / name), "--seed", "3", *extra])
    # (the command line has imported the module `generate` over the package's name for the function)
    sys.modules["musicgan_amd.generate"].generate(str(tmp_path / "loud2"), 8, ck, 1, 1, seed=3, loudness=target, limiter=False)
    assert (tmp_path / "loud" / "sound_0.wav").read_bytes() == (tmp_path / "loud2" / "sound_0.wav").read_bytes()
    wav, sr = wavio.load(str(tmp_path / "plain" / "sound_0.wav"))
    lim, _ = wavio.load(str(tmp_path / "limited" / "sound_0.wav"))
    fast, _ = wavio.load(str(tmp_path / "fast" / "sound_0.wav"))
    assert sr == 44100 and lim.shape == wav.shape and not torch.equal(lim, fast)
    c = 10 ** (-1.0 / 20)
    for got, kw in ((lim, {}), (fast, dict(attack_ms=1.0, release_ms=10.0))):
        ref = LR.normalize(wav.numpy(), sr, target, **kw)
        lufs, peak = float(audio.loudness(got, sr)), float(audio.true_peak(got))
        print(f"GENERATE {kw}: {lufs:.6f} LUFS (reference {ref['lufs']:.6f}), {R.db(peak):.6f} dBTP, reduction {ref['reduction_db']:.2f} dB")
        assert abs(lufs - ref["lufs"]) <= 1e-4 and peak <= c * (1 + 4 * 2.0 ** -23)


def test_body_on_poisoned_memory():
    """under poison.rule pointed at lim_ops: no guard band damaged by any launch, no argument changed, the workspace poisoned again
    before every call, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import audio, lim_ops
    x = torch.from_numpy(np.array(_spiky(2, 3 * _tile() + 17, 7)))
    z = torch.from_numpy(np.array(LR.prototype_signal(2)[:, :30000]))

    def run(p):
        p.a = audio.limit(x.to(DEV), 44100, gain_db=6.0, return_gain=True)
        p.b = audio.limit(x.to(DEV)[0, :100], 44100, attack_ms=2047 / 44.1)
        p.c = audio.normalize_loudness(z.to(DEV), 44100, target_lufs=-20.0, limiter=True, return_gain=True, return_details=True)
        p.d = lim_ops.envelope(x.to(DEV))
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=lim_ops, inplace={})
    flat = lambda r: r.a + (r.b,) + r.c[:2] + r.c[2] + (r.d,)
    for a, b in zip(flat(r0), flat(r1)):
        assert torch.equal(a, b)
    names = [name for name, _, _ in r1.calls]
    assert {"limit", "trim", "envelope", "pregain"} <= set(names), names
    print(f"POISON limiter: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")
