"""GPU: the inverse STFT, the magnitude projection and the Griffin-Lim loop (csrc/griffinlim.hip, musicgan_amd.gl_ops,
audio.istft / audio.griffin_lim / generate) against the float64 restatement in tests/griffinlim_ref.py.

Every tolerance is 4 x the distance of the SAME restatement run in float32 on the CPU from its float64 run on the same input (the
parity table's convention), with a floor of 1e-6 (one transform) or 1e-5 (the loop) of the largest reference value; none is fitted
to what the kernels give.  Each test prints its figures before it asserts.  References are computed once per input and shared."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_ref as G  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 4), (2, 37), (1, 130), (3, 512)]          # (N, W): TT = 4, 74, 130, 1536
IDS = [f"{n}x{w}" for n, w in SHAPES]
KINDS = ["random", "tone", "zero"]                       # uniform images; two sinusoids plus noise; the same from the magnitude alone
INPLACE = {"griffin_lim": ("Z",)}                        # "All of Z is rewritten in place"


@functools.lru_cache(maxsize=None)
def _images(kind, n, w):
    return G.random_images(n, w, 100 + n * w) if kind == "random" else G.tone_images(n, w, 200 + n * w)


def _init(kind):
    return "zero" if kind == "zero" else "phase"


@functools.lru_cache(maxsize=None)
def _spectrum(kind, n, w, dtype):
    return G.spectrum(_images(kind, n, w), _init(kind), dtype)


@functools.lru_cache(maxsize=None)
def _loop(kind, n, w, n_iter, momentum, dtype):
    M, Z0 = _spectrum(kind, n, w, dtype)
    return G.loop(M, Z0, n_iter, momentum, trace=True)


@functools.lru_cache(maxsize=None)
def _random_spectrum(tt):
    g = torch.Generator().manual_seed(300 + tt)
    return torch.complex(torch.randn(512, tt, generator=g), torch.randn(512, tt, generator=g))


def _bark():
    from musicgan_amd.audio.functions import _bark_vector
    return _bark_vector(512, torch.device(DEV))


def _device_spectrum(kind, n, w):
    from musicgan_amd import gl_ops
    return gl_ops.codec_inv_spectrum(_images(kind, n, w).to(DEV), _bark(), zero_phase=kind == "zero")


# ---------------------------------------------------------------- 1. the inverse STFT alone
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_istft_against_float64(shape):
    from musicgan_amd import audio
    tt = shape[0] * shape[1]
    Z = _random_spectrum(tt)
    ref = G.istft(Z.to(torch.complex128))
    own = float((G.istft(Z).double() - ref).abs().max())
    tol = max(4 * own, 1e-6 * float(ref.abs().max()))
    got = audio.istft(Z.to(DEV))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (256 * (tt - 1),)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"ISTFT TT={tt}: err {err:.3e}, float32 CPU {own:.3e}, tol {tol:.3e}, max|wav| {float(ref.abs().max()):.3f}")
    assert err <= tol
    # the round trip is the reference's R
    R = G.stft(ref)
    own_r = float((G.stft(G.istft(Z)).to(torch.complex128) - R).abs().max())
    tol_r = max(4 * own_r, 1e-6 * float(R.abs().max()))
    back = audio.stft_from_waveform(got)
    err_r = float((back.cpu().to(torch.complex128) - R).abs().max())
    print(f"ROUND TRIP TT={tt}: err {err_r:.3e}, float32 CPU {own_r:.3e}, tol {tol_r:.3e}")
    assert tuple(back.shape) == (512, tt) and err_r <= tol_r


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_istft_agrees_with_the_codec_path(shape):
    """on Z0, within the bound of the test above: the codec's own inverse (inv_frames + inv_overlap_add) and the new kernel"""
    from musicgan_amd import audio, ops
    n, w = shape
    mp = _images("random", n, w)
    M, Z0 = _device_spectrum("random", n, w)
    M64, Z64 = _spectrum("random", n, w, torch.float64)
    assert float((M.cpu().double() - M64).abs().max()) <= 1e-5 * float(M64.max())
    Zc = Z0.cpu()
    ref = G.istft(Zc.to(torch.complex128))
    own = float((G.istft(Zc).double() - ref).abs().max())
    tol = max(4 * own, 1e-6 * float(ref.abs().max()))
    new, old = audio.istft(Z0), ops.codec_inv(mp.to(DEV), _bark())
    e_new, e_old = float((new.cpu().double() - ref).abs().max()), float((new - old).abs().max())
    print(f"CODEC PATH TT={n * w}: new vs float64 {e_new:.3e}, new vs codec {e_old:.3e}, tol {tol:.3e}")
    assert e_new <= tol and e_old <= tol


# ---------------------------------------------------------------- 2. one projection step, and a second one
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 37), (1, 130)], ids=["2x37", "1x130"])
@pytest.mark.parametrize("steps", [1, 2])
def test_projection_step(kind, shape, steps):
    from musicgan_amd import gl_ops
    n, w = shape
    M64 = _spectrum(kind, n, w, torch.float64)[0]
    _, _, Z64, trace = _loop(kind, n, w, steps, 0.99, torch.float64)
    Z32 = _loop(kind, n, w, steps, 0.99, torch.float32)[2]
    c64 = trace[-1][1]
    keep = (c64.abs() >= 1e-3 * M64.mean()) & (M64 > 0)
    left_out = 1.0 - float(keep.double().mean())
    own = float(((Z32.to(torch.complex128) - Z64).abs() / M64)[keep].max())
    M, Z = _device_spectrum(kind, n, w)
    gl_ops.griffin_lim(M, Z, steps, 0.99)
    err = float(((Z.cpu().to(torch.complex128) - Z64).abs() / M64)[keep].max())
    print(f"PROJECTION {kind} TT={n * w} step {steps}: err {err:.3e}, float32 CPU {own:.3e}, tol {4 * own:.3e}, left out {100 * left_out:.4f} %")
    assert left_out <= 1e-3
    assert err <= 4 * own


# ---------------------------------------------------------------- 3. the loop
LOOP_CASES = [("random", (2, 37), 0.0), ("random", (2, 37), 0.99), ("random", (1, 130), 0.99), ("tone", (2, 37), 0.0),
              ("tone", (2, 37), 0.99), ("zero", (2, 37), 0.0), ("zero", (1, 130), 0.99), ("random", (1, 4), 0.99),
              ("zero", (1, 4), 0.0), ("random", (3, 512), 0.99), ("zero", (3, 512), 0.0)]


def _ulp(x):
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


@pytest.mark.parametrize("kind,shape,momentum", LOOP_CASES, ids=[f"{k}-{n}x{w}-m{m}" for k, (n, w), m in LOOP_CASES])
def test_loop(kind, shape, momentum):
    from musicgan_amd import audio, gl_ops
    n, w = shape
    wav64, conv64, _, _ = _loop(kind, n, w, 8, momentum, torch.float64)
    wav32, conv32, _, _ = _loop(kind, n, w, 8, momentum, torch.float32)
    own_w, own_c = float((wav32.double() - wav64).abs().max()), float((conv32 - conv64).abs().max())
    tol_w = max(4 * own_w, 1e-5 * float(wav64.abs().max()))
    tol_c = max(4 * own_c, 1e-5 * float(conv64.abs().max()))
    wav, conv = audio.griffin_lim(_images(kind, n, w).to(DEV), n_iter=8, momentum=momentum, init=_init(kind), return_convergence=True)
    assert wav.dtype == torch.float32 and tuple(wav.shape) == (256 * (n * w - 1),)
    assert conv.dtype == torch.float64 and conv.is_cuda and tuple(conv.shape) == (8,)
    err_w, err_c = float((wav.cpu().double() - wav64).abs().max()), float((conv.cpu() - conv64).abs().max())
    print(f"LOOP {kind} TT={n * w} momentum {momentum}: wav err {err_w:.3e} (float32 CPU {own_w:.3e}, tol {tol_w:.3e}, max {float(wav64.abs().max()):.3f}); "
          f"convergence err {err_c:.3e} (float32 CPU {own_c:.3e}, tol {tol_c:.3e}); device {[round(v, 4) for v in conv.tolist()]}")
    assert err_w <= tol_w
    assert err_c <= tol_c
    if momentum == 0.0:
        assert bool((conv[1:] <= conv[:-1]).all()), conv
    # every output Z keeps the magnitude
    M, Z = _device_spectrum(kind, n, w)
    gl_ops.griffin_lim(M, Z, 8, momentum)
    off = ((Z.cpu().to(torch.complex128).abs() - M.cpu().double()).abs() / _ulp(M.cpu())).max()
    print(f"  | |Z| - M | <= {float(off):.2f} ulp")
    assert float(off) <= 4.0


def test_zero_iterations_is_one_inversion():
    from musicgan_amd import audio
    mp = _images("random", 2, 37).to(DEV)
    wav, conv = audio.griffin_lim(mp, n_iter=0, return_convergence=True)
    _, Z0 = _device_spectrum("random", 2, 37)
    assert conv.numel() == 0 and torch.equal(wav, audio.istft(Z0))


# ---------------------------------------------------------------- 4. behaviour that must not move
def test_without_refinement_nothing_moves():
    from musicgan_amd import audio, ops
    for n, w in SHAPES[:3]:
        mp = _images("random", n, w).to(DEV)
        ref = ops.codec_inv(mp, _bark())
        assert torch.equal(audio.magn_phase_to_waveform(mp), ref)
        assert torch.equal(audio.magn_phase_to_waveform(mp, griffin_lim=0), ref)
    mp = _images("random", 2, 37).to(DEV)
    assert torch.equal(audio.magn_phase_to_waveform(mp, griffin_lim=3, momentum=0.5), audio.griffin_lim(mp, n_iter=3, momentum=0.5))


def test_generate_with_and_without_refinement(tmp_path):
    import musicgan_amd
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    ck = str(tmp_path / "gen7.pt")
    torch.save(Generator(8, end_layer=7).state_dict(), ck)
    for name, kw in (("plain", {}), ("zero", {"griffin_lim": 0}), ("four", {"griffin_lim": 4})):
        torch.manual_seed(21)
        musicgan_amd.generate(str(tmp_path / name), 8, ck, 1, 1, **kw)
    plain, zero, four = ((tmp_path / d / "sound_0.wav").read_bytes() for d in ("plain", "zero", "four"))
    assert plain == zero
    assert len(four) == len(plain) and four != plain


# ---------------------------------------------------------------- 5. determinism and memory
def test_two_runs_and_a_replayed_graph_are_bit_identical():
    from musicgan_amd import audio
    mp = _images("tone", 2, 37).to(DEV)
    a = audio.griffin_lim(mp, n_iter=4, momentum=0.99, return_convergence=True)
    b = audio.griffin_lim(mp, n_iter=4, momentum=0.99, return_convergence=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = audio.griffin_lim(mp, n_iter=4, momentum=0.99, return_convergence=True)
    c[0].zero_()
    c[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_loop_does_not_synchronise():
    from musicgan_amd import audio
    mp = _images("random", 1, 130).to(DEV)
    audio.griffin_lim(mp, n_iter=1)   # warm-up: library load, function attributes, workspace
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        wav, conv = audio.griffin_lim(mp, n_iter=3, return_convergence=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(wav).all()) and bool(torch.isfinite(conv).all())


@pytest.mark.parametrize("kind,shape", [("random", (2, 37)), ("zero", (1, 4))], ids=["random-2x37", "zero-1x4"])
def test_body_on_poisoned_memory(kind, shape):
    """the loop, the inverse alone and the split codec entry under poison.rule pointed at gl_ops: no guard band damaged by any
    launch, no argument changed that the table does not name, the workspace poisoned again before every call, equal digests under
    both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import audio, gl_ops
    n, w = shape

    def run(p):
        mp = _images(kind, n, w).to(DEV)
        p.loop = audio.griffin_lim(mp, n_iter=3, momentum=0.99, init=_init(kind), return_convergence=True)
        p.none = audio.griffin_lim(mp, n_iter=0, init=_init(kind))
        p.inv = audio.istft(_random_spectrum(n * w).to(DEV))
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=gl_ops, inplace=INPLACE)
    for a, b in zip(r0.loop + (r0.none, r0.inv), r1.loop + (r1.none, r1.inv)):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert {"codec_inv_spectrum", "griffin_lim", "istft_1024"} <= names, names
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    print(f"POISON griffin-lim {kind} {shape}: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")
