"""CPU: the float64 restatement of the Griffin-Lim definition (tests/griffinlim_ref.py) against oracle.audio, the command line and
the argument errors that are raised before any device call."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import griffinlim_ref as G  # noqa: E402


def test_zero_iterations_is_the_oracle_inverse():
    from oracle import audio as oracle_audio
    mp = G.random_images(2, 37, 1)
    wav, conv, _ = G.griffin_lim(mp, 0, 0.99)
    ref = oracle_audio.magn_phase_to_wav(mp.numpy())
    assert wav.shape == ref.shape == (256 * 73,) and conv.numel() == 0
    # the oracle works in float32 up to the spectrum and rounds its result to float32
    assert float(np.abs(wav.numpy() - ref).max()) <= 1e-5 * float(np.abs(ref).max())


def test_round_trip_of_the_restatement_is_the_oracle_stft():
    from oracle import audio as oracle_audio
    g = torch.Generator().manual_seed(2)
    wav = torch.rand(256 * 9, generator=g, dtype=torch.float64) - 0.5
    ref = oracle_audio.stft(wav.float().numpy())
    got = G.stft(wav)
    assert tuple(got.shape) == ref.shape == (512, 10)
    assert float(np.abs(got.numpy() - ref).max()) <= 1e-6 * float(np.abs(ref).max())


@pytest.mark.parametrize("kind", ["random", "tone", "zero"])
def test_without_momentum_the_distance_does_not_grow(kind):
    mp = G.random_images(2, 37, 3) if kind == "random" else G.tone_images(2, 37, 4)
    _, conv, _ = G.griffin_lim(mp, 8, 0.0, "zero" if kind == "zero" else "phase")
    assert conv.shape == (8,) and bool((conv[1:] <= conv[:-1]).all()), conv


def test_parser_takes_griffin_lim():
    from musicgan_amd.__main__ import _MODES, build_parser
    p = build_parser()
    a = p.parse_args(["generate", "gen.pt", "32", "-o", "o", "--griffin-lim", "8"])
    assert a.griffin_lim == 8 and _MODES["generate"][4](a) == {"griffin_lim": 8}
    b = p.parse_args(["generate", "gen.pt", "32", "-o", "o"])
    assert b.griffin_lim == 0 and _MODES["generate"][4](b) == {}
    c = p.parse_args(["generate", "gen.pt", "32", "-o", "o", "--format", "flac", "--griffin-lim", "2"])
    assert _MODES["generate"][4](c) == {"audio_format": "flac", "griffin_lim": 2}


def test_argument_errors_come_before_the_device(tmp_path):
    import musicgan_amd
    from musicgan_amd import audio
    mp = torch.zeros(1, 2, 512, 8)
    with pytest.raises(ValueError, match="init"):
        audio.griffin_lim(mp, init="random")
    with pytest.raises(ValueError, match="n_iter"):
        audio.griffin_lim(mp, n_iter=-1)
    for m in (-0.1, 1.0):
        with pytest.raises(ValueError, match="momentum"):
            audio.griffin_lim(mp, momentum=m)
        with pytest.raises(ValueError, match="momentum"):
            audio.magn_phase_to_waveform(mp, griffin_lim=2, momentum=m)
    with pytest.raises(ValueError, match="frames"):
        audio.griffin_lim(torch.zeros(1, 2, 512, 3))
    with pytest.raises(ValueError, match="spectrum"):
        audio.istft(torch.zeros(512, 3, dtype=torch.complex64))
    with pytest.raises(ValueError, match="spectrum"):
        audio.istft(torch.zeros(513, 8, dtype=torch.complex64))
    with pytest.raises(ValueError, match="griffin_lim"):
        musicgan_amd.generate(str(tmp_path / "g"), 8, "missing.pt", 1, 1, griffin_lim=-1)
    assert not os.path.exists(tmp_path / "g")


def test_workspace_query_counts_two_spectra_and_the_partial_sums():
    from musicgan_amd import gl_ops
    tt = 74
    pairs = 512 * tt // 2
    blocks = min((pairs + 255) // 256, 2048)
    assert gl_ops.griffin_lim_ws_bytes(tt, 8) == 2 * 512 * tt * 8 + (8 * blocks * 2 + 2) * 8
    assert gl_ops.griffin_lim_ws_bytes(tt, 0) == 2 * 512 * tt * 8 + 16


def test_kernels_keep_their_registers():
    from musicgan_amd import _build
    _build.build()
    hits = {k: v for k, v in _build.resource_usage().items() if "istft1024" in k or "gl_project" in k or "gl_convergence" in k}
    assert len(hits) == 4, sorted(hits)
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)
        if "istft1024" in name:   # two workgroups of 8 waves per CU
            assert u["VGPRs"] <= 128 and u["Occupancy [waves/SIMD]"] >= 4, u
