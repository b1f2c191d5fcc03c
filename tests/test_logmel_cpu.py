"""CPU: the host half of the log-mel feature space -- metrics.mel_filterbank against the formula written out in
tests/logmel_ref.py, metrics.frechet_distance against closed forms and against scipy's matrix square root, the `evaluate_mel`
sub-command's parser and the refusals of the function, the argument checks of musicgan_amd/mel_ops.py, and the scratch use of the
new kernels."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as L  # noqa: E402

BANKS = [(512, 64), (256, 32), (128, 16), (64, 8)]


# ------------------------------------------------------------------ mel_filterbank
@pytest.mark.parametrize("shape", BANKS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filterbank_is_the_formula(shape):
    from musicgan_amd import metrics
    rows, bands = shape
    w, lo, hi = metrics.mel_filterbank(rows, bands)
    ref, ref_lo, ref_hi, empty = L.filterbank(rows, bands)
    assert w.dtype == torch.float32 and tuple(w.shape) == (bands, rows) and lo.dtype == torch.int32 and hi.dtype == torch.int32
    assert not w.is_cuda and not lo.is_cuda and not hi.is_cuda and empty == 0
    got = w.double().numpy()
    # two float64 evaluations of one formula, each rounded once to float32: one float32 ulp of a weight <= 1
    assert np.abs(got - ref).max() <= 2.0 ** -23
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert lo.tolist() == ref_lo and hi.tolist() == ref_hi
    for m in range(bands):                                               # every band non-empty, [lo, hi) tight
        assert 0 <= lo[m] < hi[m] <= rows
        assert got[m, lo[m]] > 0 and got[m, hi[m] - 1] > 0
        assert not got[m, :lo[m]].any() and not got[m, hi[m]:].any()
    assert int((got > 0).sum(0).max()) <= 2                              # a row is in at most two bands
    longest = int((hi - lo).max())
    print(f"mel_filterbank {rows} x {bands}: longest band {longest} rows, largest difference {np.abs(got - ref).max():.2e}")
    if shape == (512, 64):
        assert longest == 53


@pytest.mark.parametrize("shape,empty", [((512, 128), 1), ((64, 64), 13)], ids=["512x128", "64x64"])
def test_filterbank_refuses_empty_bands(shape, empty):
    from musicgan_amd import metrics
    assert L.filterbank(*shape)[3] == empty
    with pytest.raises(ValueError):
        metrics.mel_filterbank(*shape)


def test_filterbank_and_logmel_refuse_bad_arguments():
    from musicgan_amd import metrics
    for rows, bands in ((100, 8), (4, 1), (1024, 64), (64, 0)):
        with pytest.raises(ValueError):
            metrics.mel_filterbank(rows, bands)
    with pytest.raises(ValueError):
        metrics.mel_filterbank(64, 8, f_min=5000.0, f_max=4000.0)
    for args, kw in (((32, 64), {}), ((64, 64), dict(pools=7)), ((64, 64), dict(floor=0.0)), ((64, 64), dict(bands=64))):
        with pytest.raises(ValueError):
            metrics.LogMel(*args, **kw)
    lm = metrics.LogMel(512, 512)
    assert (lm.bands, lm.pools, lm.dims, lm.floor) == (64, 32, 2048, 1e-6)
    small = metrics.LogMel(64, 64)
    assert (small.bands, small.pools) == (8, 8)
    assert "unmeasured" in metrics.LogMel.__doc__
    # scale = 1 / (2 b): at 512 rows b is the codec's vector itself, below that its mean over the bins of a row
    from musicgan_amd.audio.functions import _bark_vector
    bark = _bark_vector(512, "cpu").double()
    assert torch.equal(lm.scale, (1.0 / (2.0 * bark)).float())
    assert torch.equal(small.scale, (1.0 / (2.0 * bark.view(64, 8).mean(1))).float())
    with pytest.raises(ValueError):
        lm(torch.zeros(1, 2, 64, 64))


# ------------------------------------------------------------------ frechet_distance
def _sample(n, d, seed, shift=0.0, spread=1.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)) @ (rng.standard_normal((d, d)) * spread / np.sqrt(d)) + shift
    return torch.from_numpy(x.mean(0)), torch.from_numpy(np.cov(x.T).reshape(d, d))


def _scale(c1, c2):
    return float(torch.trace(c1) + torch.trace(c2))


def test_frechet_of_identical_moments_is_zero():
    from musicgan_amd import metrics
    for n, d in ((200, 32), (20, 32), (5, 1)):                           # full rank, singular, one dimension
        m, c = _sample(n, d, 80 + n)
        got = metrics.frechet_distance(m, c, m.clone(), c.clone())
        print(f"frechet identical {n} x {d}: {got:.3e} at scale {_scale(c, c):.3e}")
        assert abs(got) <= 1e-10 * _scale(c, c)


def test_frechet_of_diagonal_covariances_is_the_closed_form():
    from musicgan_amd import metrics
    rng = np.random.default_rng(81)
    a, b = rng.uniform(0.0, 3.0, 40), rng.uniform(0.0, 3.0, 40)
    a[:3] = 0.0                                                          # singular directions
    m1, m2 = rng.standard_normal(40), rng.standard_normal(40)
    got = metrics.frechet_distance(torch.from_numpy(m1), torch.diag(torch.from_numpy(a)), torch.from_numpy(m2),
                                   torch.diag(torch.from_numpy(b)))
    want = L.frechet_diagonal(m1, a, m2, b)
    assert abs(got - want) <= 1e-10 * (a.sum() + b.sum()), (got, want)


def test_frechet_of_full_rank_sample_covariances_is_the_textbook_form():
    """n >= 4 d: scipy's sqrtm(C1 C2) is accurate there (the two differ by 2e-16 of the scale)"""
    from musicgan_amd import metrics
    for n, d, seed in ((200, 32, 82), (64, 16, 83), (400, 7, 84)):
        m1, c1 = _sample(n, d, seed)
        m2, c2 = _sample(n, d, seed + 100, shift=0.3, spread=1.4)
        got, want = metrics.frechet_distance(m1, c1, m2, c2), L.frechet(m1.numpy(), c1.numpy(), m2.numpy(), c2.numpy())
        print(f"frechet {n} x {d}: {got:.12f} against {want:.12f}, difference / scale {abs(got - want) / _scale(c1, c2):.2e}")
        assert abs(got - want) <= 1e-10 * _scale(c1, c2)
        assert got > 0.0
        back = metrics.frechet_distance(m2, c2, m1, c1)                  # symmetric up to rounding
        assert abs(got - back) <= 1e-10 * _scale(c1, c2)


def test_frechet_of_singular_covariances_is_finite_and_not_negative():
    from musicgan_amd import metrics
    for n, d, seed in ((8, 32, 85), (2, 64, 86), (30, 31, 87)):
        m1, c1 = _sample(n, d, seed)
        m2, c2 = _sample(n, d, seed + 100, shift=0.1)
        got = metrics.frechet_distance(m1, c1, m2, c2)
        assert np.isfinite(got) and got >= -1e-9 * _scale(c1, c2), got


def test_frechet_refuses_what_is_no_pair_of_moments():
    from musicgan_amd import metrics
    m, c = _sample(20, 4, 88)
    for args in ((m.float(), c, m, c), (m, c[:3], m, c), (m, c, m[:3], c[:3, :3]), (m.reshape(1, 4), c, m, c)):
        with pytest.raises(ValueError):
            metrics.frechet_distance(*args)
    with pytest.raises(ValueError):
        metrics.Frechet().moments()                                      # nothing fed


# ------------------------------------------------------------------ the sub-command
def _function_and_module():
    """the package's lazy export (asked for directly: a sub-module imported earlier in the process is bound over the name)"""
    import musicgan_amd
    fn = musicgan_amd.__getattr__("evaluate_mel")
    return fn, sys.modules["musicgan_amd.evaluate_mel"]


def test_evaluate_mel_parses_and_dispatches(monkeypatch):
    _, module = _function_and_module()
    from musicgan_amd.__main__ import _FEATURE_MODES, _LATENT_MODES, _MODES, _all_modes, build_parser, main
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"] and list(_LATENT_MODES) == ["project"]
    assert list(_FEATURE_MODES) == ["evaluate_mel"] and list(_all_modes())[-1] == "evaluate_mel"
    p = build_parser()
    a = p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data", "--metrics", "fd,prdc"])
    _, _, _, pos, kw = _FEATURE_MODES["evaluate_mel"]
    assert pos(a) == ("gen.pt", 32, "data")
    assert kw(a) == dict(level=7, nb_images=8192, batch_size=16, seed=0, output=None, metrics=("fd", "prdc"))
    plain = p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data"])
    assert "metrics" not in kw(plain)                                    # the function's own default
    for bad in ("fid", "", "fd,fd", "swd", "fd,,nn"):
        with pytest.raises(SystemExit):
            p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data", "--metrics", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["evaluate", "gen.pt", "32", "-i", "data", "--metrics", "fd"])   # not a metric of evaluate
    seen = []
    monkeypatch.setattr(module, "evaluate_mel", lambda *args, **kwargs: seen.append((args, kwargs)))
    main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--level", "5", "-n", "100", "--metrics", "ndb,fd", "-o", "out.json"])
    assert seen == [(("gen.pt", 32, "data"), dict(level=5, nb_images=100, batch_size=16, seed=0, output="out.json",
                                                  metrics=("ndb", "fd")))]


def test_evaluate_mel_refuses_before_it_opens_a_file():
    import inspect
    import musicgan_amd
    fn, module = _function_and_module()
    assert callable(fn) and fn is module.evaluate_mel and musicgan_amd.evaluate_mel is fn
    assert module.METRICS == ("fd", "nn", "prdc", "ndb")
    sig = inspect.signature(fn)
    assert list(sig.parameters) == ["gen_dict_state", "rand_channels", "input_dataset", "metrics", "level", "nb_images", "batch_size",
                                    "seed", "output"]
    assert sig.parameters["metrics"].default == ("fd",) and sig.parameters["level"].kind is inspect.Parameter.KEYWORD_ONLY
    missing = "/nonexistent/gen.pt"
    for kw in (dict(level=3), dict(level=8), dict(nb_images=3), dict(metrics=("fid",)), dict(metrics=()), dict(metrics=("fd", "fd")),
               dict(metrics=("swd",)), dict(metrics=("prdc",), nb_images=7), dict(batch_size=0)):
        with pytest.raises(ValueError):
            fn(missing, 8, "/nonexistent/data", **kw)


# ------------------------------------------------------------------ the wrappers
def _logmel_args(h=64, w=64, bands=8):
    from musicgan_amd import metrics
    weight, lo, hi = metrics.mel_filterbank(h, bands)
    return dict(x=torch.zeros(2, 2, h, w), c=0, scale=torch.ones(h), weight=weight, lo=lo, hi=hi, floor=1e-6, pools=8)


def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from musicgan_amd import _lib, mel_ops, ops
    assert not [name for name in vars(ops) if "mel" in name or "moments" in name]
    good = _logmel_args()
    with pytest.raises(_lib.MusicGanHipError):
        mel_ops.logmel_rows(**good)                                      # well-formed, but on the host
    with pytest.raises(_lib.MusicGanHipError):
        mel_ops.moments(torch.zeros(5, 3))
    bad = [dict(pools=7), dict(pools=0), dict(hi=good["hi"] + 57), dict(lo=good["lo"] - 1), dict(lo=good["hi"] + 1), dict(c=2),
           dict(c=-1), dict(scale=torch.ones(63)), dict(weight=torch.ones(8, 63)), dict(floor=0.0), dict(floor=float("inf")),
           dict(x=torch.zeros(2, 64, 64)), dict(lo=good["lo"].long()), dict(hi=good["hi"][:7]), dict(out=torch.zeros(2, 63)),
           dict(x=torch.zeros(1, 1, 64, 4096), pools=2)]
    for change in bad:
        with pytest.raises(ValueError):
            mel_ops.logmel_rows(**dict(good, **change))
    assert int((good["hi"] + 57).max()) > 64                             # the hi > H case above is one
    for shape in ((1, 4), (0, 4), (5, 0), (5, 4097), (5,), (5, 2, 2)):
        with pytest.raises(ValueError):
            mel_ops.moments(torch.zeros(shape))
    with pytest.raises(ValueError):
        mel_ops.moments(torch.zeros(5, 3), mean=torch.zeros(4, dtype=torch.float64))
    assert mel_ops.moments_ws_bytes(1000, 513) == 1 * (513 + 513 * 513) * 8
    assert mel_ops.moments_ws_bytes(1025, 7) == 2 * (7 + 49) * 8
    assert mel_ops.moments_ws_bytes(1, 7) == 0 and mel_ops.moments_ws_bytes(5, 4097) == 0
    for fn in (mel_ops.logmel_rows, mel_ops.moments, mel_ops.moments_ws_bytes):
        assert fn.__doc__ and ("written" in fn.__doc__ or "host query" in fn.__doc__)


def test_new_kernels_use_no_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    hits = {k: v for k, v in usage.items() if "logmel_rows_k" in k or "mo_mean_" in k or "mo_cov_" in k}
    assert len(hits) == 6, sorted(hits)                                  # two tile widths of the feature kernel, four of the moments
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)
