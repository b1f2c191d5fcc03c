"""CPU: the float64 yardstick of tests/ppl_ref.py against project.slerp, numpy's percentiles and the closed form of a chord on a
sphere; every host-side refusal of ppl_ops, metrics.PPL and `path_length` -- each raised before a file or a device is touched --;
and the command line of `path_length`."""
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ppl_ref as R  # noqa: E402


def _pairs(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g), torch.randn(n, d, generator=g), torch.rand(n, dtype=torch.float64, generator=g)


# ------------------------------------------------------------------ the reference
def test_reference_slerp_is_project_slerp_within_half_a_float32_ulp():
    from musicgan_amd import project
    worst = 0.0
    for d, seed in ((3, 1), (32, 2), (128, 3), (2049, 4)):
        z0, z1, t = _pairs(6, d, seed)
        z1[1] = z0[1]                                                     # an equal pair
        z1[2] = z0[2] + 1e-7 * z1[2]                                      # nearly parallel: the straight line
        z0[3] = 0.0                                                       # a zero vector: the straight line
        ts = t.tolist()
        ts[4], ts[5] = 0.0, 1.0
        for i in range(6):
            ref, _, anti = R.slerp(z0[i].numpy(), z1[i].numpy(), ts[i])
            got = project.slerp(z0[i].view(-1, 1, 1), z1[i].view(-1, 1, 1), ts[i]).view(-1).double().numpy()
            assert not anti
            worst = max(worst, float((np.abs(got - ref) / R.half_ulp32(ref)).max()))
        assert np.array_equal(project.slerp(z0[4], z1[4], 0.0).numpy(), z0[4].numpy())
        assert np.array_equal(R.slerp(z0[4].numpy(), z1[4].numpy(), 0.0)[0].astype(np.float32), z0[4].numpy())
    print(f"reference slerp against project.slerp: worst error {worst:.4f} half ulps of float32")
    assert worst <= 1.0
    a = torch.randn(8, generator=torch.Generator().manual_seed(5))
    assert R.slerp(a.numpy(), (-a).numpy(), 0.3)[2]                        # antipodal: project.slerp raises there
    with pytest.raises(ValueError):
        project.slerp(a, -a, 0.3)


def test_half_ulp_is_half_the_float32_spacing():
    for x in (1.0, 1.5, 0.75, 3.0e-5, 123456.0, 2.0 ** -130, 0.0):
        want = 0.5 * float(np.spacing(np.float32(x))) if x >= 2.0 ** -126 else 2.0 ** -150
        assert float(R.half_ulp32(np.array(x))) == want, x


@pytest.mark.parametrize("n", [2, 3, 100, 101])
def test_trimming_is_numpy_percentile_lower_and_higher(n):
    from musicgan_amd import metrics
    values = np.random.default_rng(n).standard_normal(n) ** 2
    lo, hi = metrics.ppl_trim(values.tolist())
    assert lo == float(np.percentile(values, 1, method="lower")) and hi == float(np.percentile(values, 99, method="higher"))
    assert (lo, hi) == R.trim(values)
    ordered = np.sort(values)
    assert lo == ordered[math.floor(0.01 * (n - 1))] and hi == ordered[math.ceil(0.99 * (n - 1))]
    flag = np.zeros(n)
    flag[0] = 1                                                           # one pair left out of everything
    chord = values + 1.0
    got, want = metrics.ppl_aggregate(values.tolist(), flag.tolist(), chord.tolist()), R.aggregate(values, flag, chord)
    assert got == want and list(got) == ["ppl", "ppl_mean", "ppl_chord", "ppl_ratio", "ppl_pairs"] and got["ppl_pairs"] == n - 1
    end = metrics.ppl_aggregate(values.tolist(), flag.tolist())
    assert end == R.aggregate(values, flag) and list(end) == ["ppl", "ppl_mean", "ppl_pairs"]
    with pytest.raises(ValueError):
        metrics.ppl_aggregate(values.tolist(), [1.0] * n)


def test_identity_rows_on_a_sphere_give_the_chord_of_the_step():
    """rows = the latent itself, ends of one norm r at the angle w: za and zb lie on the sphere an angle w eps apart, so
    d = (2 r sin(w eps / 2))^2 / (D eps^2).  Every component of za - zb carries at most 4 u r of rounding against a length of
    r w eps, so d is within 2 * 4 u sqrt(D) / (w eps) of it, relatively: under 1e-8 for every case here (w >= 0.5, eps >= 1e-5)."""
    for d, eps, seed in ((128, 1e-4, 1), (32, 1e-3, 2), (512, 1e-5, 3)):
        z0, z1, t = _pairs(5, d, seed)
        z0, z1 = z0.double().numpy(), z1.double().numpy()
        r = 1.7
        z0 *= r / np.linalg.norm(z0, axis=1, keepdims=True)
        z1 *= r / np.linalg.norm(z1, axis=1, keepdims=True)
        za, zb, _, _, flag = R.slerp_pairs(z0, z1, t.numpy(), eps)
        got = R.per_pair(za, zb, eps)
        omega = np.arccos((z0 * z1).sum(1) / r ** 2)
        want = (2.0 * r * np.sin(omega * eps / 2.0)) ** 2 / (d * eps * eps)
        assert not flag.any() and omega.min() >= 0.5
        bound = 8 * R.U64 * math.sqrt(d) / (0.5 * eps)
        worst = float(np.abs(got / want - 1.0).max())
        print(f"chord of the step, d = {d}, eps = {eps:g}: worst relative error {worst:.2e}, bound {bound:.2e}")
        assert worst <= bound < 1e-8, (d, eps)


# ------------------------------------------------------------------ refusals, each before a device or a file is touched
def test_ops_refuse_bad_shapes_and_values_on_the_host():
    from musicgan_amd import _lib, ppl_ops
    z, t = torch.zeros(3, 8), torch.zeros(3, dtype=torch.float64)
    for args in ((z[0], z, t, 1e-4), (z, torch.zeros(3, 7), t, 1e-4), (z, z, t[:2], 1e-4), (z, z, t, float("nan")), (z, z, t, "1e-4"),
                 (torch.zeros(0, 8), torch.zeros(0, 8), t[:0], 1e-4)):
        with pytest.raises(ValueError):
            ppl_ops.slerp_pairs(*args)
    for args in ((z, z[:2]), (z.view(-1), z.view(-1)), (z, z, float("inf")), (z, z, 1.0, torch.zeros(2, dtype=torch.float64))):
        with pytest.raises(ValueError):
            ppl_ops.rows_sqdist(*args)
    with pytest.raises(_lib.MusicGanHipError):                            # well-formed, on the host: no fallback
        ppl_ops.slerp_pairs(z, z, t, 1e-4)
    with pytest.raises(_lib.MusicGanHipError):
        ppl_ops.rows_sqdist(z, z)


def test_ppl_refuses_bad_arguments():
    from musicgan_amd import metrics
    rows = lambda z: z.reshape(z.shape[0], -1)   # noqa: E731
    for kw in (dict(epsilon=0.0), dict(epsilon=0.2), dict(epsilon=True), dict(sampling="middle"), dict(seed=1.5),
               dict(rand_channels=0)):
        with pytest.raises(ValueError):
            metrics.PPL(rows, **{"rand_channels": 8, **kw})
    with pytest.raises(ValueError):
        metrics.PPL(None, rand_channels=8)
    ppl = metrics.PPL(rows, rand_channels=8)
    assert (ppl.epsilon, ppl.sampling, ppl.seed) == (1e-4, "full", 0)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            ppl.feed(bad)
    with pytest.raises(ValueError):
        ppl.result()                                                      # nothing fed


def test_path_length_signature_and_refusals_before_the_checkpoint_is_opened():
    import musicgan_amd
    fn = musicgan_amd.__getattr__("path_length")                          # the lazy export itself
    assert fn is musicgan_amd.path_length and callable(fn)
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["gen_dict_state", "rand_channels", "level", "nb_pairs", "epsilon", "sampling", "seed", "output",
                                    "waveform", "griffin_lim"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert defaults == dict(level=7, nb_pairs=8192, epsilon=1e-4, sampling="full", seed=0, output=None, waveform=False, griffin_lim=0)
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in defaults)
    for kw in (dict(level=3), dict(level=8), dict(waveform=True, level=6), dict(griffin_lim=4), dict(griffin_lim=-1, waveform=True),
               dict(nb_pairs=1), dict(nb_pairs=2.5), dict(epsilon=0.0), dict(epsilon=0.11), dict(epsilon=-1e-4),
               dict(sampling="both"), dict(seed="0")):
        with pytest.raises(ValueError):
            fn("/nonexistent/gen.pt", 8, **kw)
    with pytest.raises(ValueError):
        fn("/nonexistent/gen.pt", 0)


# ------------------------------------------------------------------ the command line
def test_the_parser_takes_path_length_and_hands_over_the_keywords(monkeypatch):
    import importlib
    from musicgan_amd.__main__ import (_FEATURE_MODES, _FILE_MODES, _FILE_SET_MODES, _LATENT_MODES, _MODES, _PATH_MODES, _all_modes,
                                       build_parser, main)
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"]
    assert list(_FILE_MODES) == ["loudness", "separate"] and list(_LATENT_MODES) == ["project"]
    assert list(_FILE_SET_MODES) == ["evaluate_audio"] and list(_FEATURE_MODES) == ["evaluate_mel"]
    assert list(_PATH_MODES) == ["path_length"]
    assert list(_all_modes())[-2:] == ["path_length", "evaluate_mel"]
    p = build_parser()
    _, _, _, pos, kw = _PATH_MODES["path_length"]
    a = p.parse_args(["path_length", "gen.pt", "32"])
    assert pos(a) == ("gen.pt", 32)
    assert kw(a) == dict(level=7, nb_pairs=8192, epsilon=1e-4, sampling="full", seed=0, output=None)
    a = p.parse_args(["path_length", "gen.pt", "32", "--level", "5", "-n", "100", "--epsilon", "1e-3", "--sampling", "end", "--seed",
                      "3", "--waveform", "--griffin-lim", "8", "-o", "ppl.json"])
    assert kw(a) == dict(level=5, nb_pairs=100, epsilon=1e-3, sampling="end", seed=3, output="ppl.json", waveform=True, griffin_lim=8)
    for bad in (["--sampling", "middle"], ["--epsilon", "0"], ["--epsilon", "0.5"], ["--epsilon", "x"], ["-n", "many"], ["--level", "x"]):
        with pytest.raises(SystemExit):
            p.parse_args(["path_length", "gen.pt", "32"] + bad)
    with pytest.raises(SystemExit):
        p.parse_args(["path_length", "gen.pt"])
    with pytest.raises(SystemExit):
        main(["path_length", "gen.pt", "32", "--griffin-lim", "8"])       # needs --waveform
    seen = []
    module = importlib.import_module("musicgan_amd.path_length")
    monkeypatch.setattr(module, "path_length", lambda *args, **kwargs: seen.append((args, kwargs)))
    main(["path_length", "gen.pt", "32", "-n", "64", "--level", "4"])
    assert seen == [(("gen.pt", 32), dict(level=4, nb_pairs=64, epsilon=1e-4, sampling="full", seed=0, output=None))]


def test_the_abi_declares_and_binds_the_two_entry_points():
    from musicgan_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "musicgan_hip.h")).read()
    for name in ("mg_slerp_pairs", "mg_rows_sqdist"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
