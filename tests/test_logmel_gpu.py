"""GPU: the log-mel feature kernel (csrc/logmel.hip) and the float64 moments (csrc/moments.hip) through musicgan_amd.mel_ops,
metrics.LogMel / metrics.Frechet and the `evaluate_mel` driver.  Both kernels are held against the float64 restatements of
tests/logmel_ref.py within bounds derived from the precisions alone; every figure is printed before it is asserted."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logmel_ref as L  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 1e-6
# the tensor arguments the wrappers of musicgan_amd/mel_ops.py write (their docstrings)
INPLACE = {
    "logmel_rows": ("out",),          # "out (N, M * pools) float32, every element written"
    "moments": ("mean", "cov"),       # "all of mean (d,) and all of cov (d, d) float64 are written"
}


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ logmel_rows: the cases
def _mel_case(n, h, w, bands, pools, seed, channels=2, c=0):
    """uniform values in [-1.2, 1.2] (a generator's outputs are not clamped), the last image all -1; the codec's scale"""
    from musicgan_amd import metrics
    weight, lo, hi = metrics.mel_filterbank(h, bands)
    x = torch.rand(n, channels, h, w, generator=torch.Generator().manual_seed(seed)) * 2.4 - 1.2
    x[n - 1] = -1.0
    return dict(x=x, c=c, scale=metrics.LogMel(h, max(w, 8), bands=bands, pools=1).scale, weight=weight, lo=lo, hi=hi, pools=pools)


def _hand_case():
    """40 rows, 96 columns in 2 pools of 48 (no multiple of a wave: a wave's lanes lie in two bands), channel 1 of 3, 6 bands (no
    multiple of a workgroup's 4): two of length 1 at the ends, one of all rows, two over the same rows, an empty one.  Weights
    outside [lo, hi) are NaN: they are never read."""
    gen = torch.Generator().manual_seed(91)
    lo = torch.tensor([0, 39, 0, 5, 5, 20], dtype=torch.int32)
    hi = torch.tensor([1, 40, 40, 17, 17, 20], dtype=torch.int32)
    weight = torch.full((6, 40), float("nan"))
    for m in range(6):
        weight[m, lo[m]:hi[m]] = torch.rand(int(hi[m] - lo[m]), generator=gen)
    x = torch.rand(2, 3, 40, 96, generator=gen) * 2.4 - 1.2
    x[1] = -1.0
    return dict(x=x, c=1, scale=torch.rand(40, generator=gen) * 50 + 0.5, weight=weight, lo=lo, hi=hi, pools=2)


CASES = {
    "64x64_8x8": lambda: _mel_case(3, 64, 64, 8, 8, 92),                     # pools of 8 columns
    "512x512_64x32": lambda: _mel_case(2, 512, 512, 64, 32, 93),             # the longest band: 53 rows
    "128x256_16x4": lambda: _mel_case(2, 128, 256, 16, 4, 94),               # pools of 64 columns: one wave
    "128x256_16x256": lambda: _mel_case(2, 128, 256, 16, 256, 94),           # pools of one column
    "128x256_16x1": lambda: _mel_case(2, 128, 256, 16, 1, 94),               # one pool of 256 columns: across waves
    "hand_bank_c1_of_3": _hand_case,
}
_REF = {}


def _reference(name):
    """(case, float64 restatement, bound), computed once and shared"""
    if name not in _REF:
        case = CASES[name]()
        a = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in case.items()}
        lo, hi = case["lo"].tolist(), case["hi"].tolist()
        ref = L.logmel(a["x"], a["c"], a["scale"], a["weight"], lo, hi, FLOOR, a["pools"])
        f32 = L.logmel_f32(a["x"], a["c"], a["scale"], a["weight"], lo, hi, FLOOR, a["pools"])
        bound = L.logmel_bound(ref, lo, hi)
        for arr in (ref, bound):
            arr.setflags(write=False)
        _REF[name] = (case, ref, bound, float((np.abs(f32 - ref) / bound).max()))
    return _REF[name]


def _run(case, **kw):
    from musicgan_amd import mel_ops
    return mel_ops.logmel_rows(case["x"].to(DEV), case["c"], case["scale"].to(DEV), case["weight"].to(DEV), case["lo"], case["hi"],
                               FLOOR, case["pools"], **kw)


def _logmel_body(name):
    case, ref, bound, numpy_margin = _reference(name)
    out = _run(case)
    n, bands = case["x"].shape[0], case["weight"].shape[0]
    assert out.dtype == torch.float32 and tuple(out.shape) == (n, bands * case["pools"]) and out.is_cuda
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    worst = float((np.abs(got - ref) / bound).max())
    print(f"logmel_rows {name}: worst err / bound {worst:.4f} (a float32 numpy evaluation: {numpy_margin:.4f}); bound "
          f"{float(bound.min()):.3e} .. {float(bound.max()):.3e}; values {got.min():.3f} .. {got.max():.3f}")
    assert worst <= 1.0
    # the image of all -1 decodes to silence: every band is log(floor), within one float32 ulp
    silent, want = out[n - 1].cpu(), np.float32(np.log(FLOOR))
    ulp = float(np.spacing(np.abs(want)))
    assert float((silent.double() - float(want)).abs().max()) <= ulp, silent
    assert float(got[:n - 1].max()) > float(want) + 1.0                 # ... and the others are not silent
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_logmel_rows_are_the_float64_definition_within_the_derived_bound(name):
    _logmel_body(name)


def test_a_row_depends_on_its_image_alone_and_runs_are_bit_identical():
    case = _mel_case(5, 64, 64, 8, 8, 95)
    case["x"][4] = case["x"][2] * 0.5                                    # no silent image here: five different ones
    whole, again = _run(case), _run(case)
    assert torch.equal(_bits(whole), _bits(again))
    for i in (0, 2, 4):                                                  # first, inside, last: alone
        alone = _run(dict(case, x=case["x"][i:i + 1].contiguous()))
        assert torch.equal(_bits(alone[0]), _bits(whole[i])), i
    order = [3, 0, 4, 2, 1]
    shuffled = _run(dict(case, x=case["x"][order].contiguous()))
    assert torch.equal(_bits(shuffled), _bits(whole[order]))
    wide = _mel_case(3, 128, 256, 16, 1, 96)                             # the wide tile's kernel
    whole = _run(wide)
    assert torch.equal(_bits(_run(dict(wide, x=wide["x"][1:2].contiguous()))[0]), _bits(whole[1]))


def test_logmel_rows_in_a_captured_graph_equal_the_eager_call():
    from musicgan_amd import mel_ops
    case = _mel_case(3, 64, 64, 8, 8, 97)
    dev = {k: (v.to(DEV) if k in ("x", "scale", "weight") else v) for k, v in case.items()}
    eager = mel_ops.logmel_rows(floor=FLOOR, **dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mel_ops.logmel_rows(floor=FLOOR, **dev)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(eager))


def test_logmel_class_is_the_wrapper_on_channel_0():
    from musicgan_amd import mel_ops, metrics
    lm = metrics.LogMel(64, 128, pools=4)
    x = (torch.rand(3, 2, 64, 128, generator=torch.Generator().manual_seed(98)) * 2.4 - 1.2).to(DEV)
    rows = lm(x)
    assert tuple(rows.shape) == (3, 8 * 4) and lm.dims == 32
    want = mel_ops.logmel_rows(x, 0, lm.scale.to(DEV), lm.weight.to(DEV), lm.lo, lm.hi, 1e-6, 4)
    assert torch.equal(_bits(rows), _bits(want))
    other = x.clone()
    other[:, 1] = 0.0                                                    # the phase-delta channel is not looked at
    assert torch.equal(_bits(lm(other)), _bits(rows))
    with pytest.raises(ValueError):
        lm(x[:, :, :, :64].contiguous())


# ------------------------------------------------------------------ moments
MOMENT_SHAPES = [(2, 1), (33, 7), (300, 64), (1000, 513), (2100, 33)]      # the last: three chunks of rows, the last one ragged


def _moment_rows(n, d):
    """values with a mean well away from 0, as log-mel rows have"""
    gen = torch.Generator().manual_seed(100 + n + d)
    return torch.randn(n, d, generator=gen) * (torch.rand(d, generator=gen) + 0.1) - 3.0


def _moments_body(shape):
    from musicgan_amd import mel_ops
    x = _moment_rows(*shape)
    mean, cov = mel_ops.moments(x.to(DEV))
    n, d = shape
    assert mean.dtype == torch.float64 and cov.dtype == torch.float64 and tuple(mean.shape) == (d,) and tuple(cov.shape) == (d, d)
    ref_mean, ref_cov, bound_mean, bound_cov = L.moments(x.numpy())
    err_mean = float((np.abs(mean.cpu().numpy() - ref_mean) / bound_mean).max())
    err_cov = float((np.abs(cov.cpu().numpy() - ref_cov) / bound_cov).max())
    print(f"moments {n} x {d}: worst err / bound {err_mean:.4f} (mean), {err_cov:.4f} (cov)")
    assert err_mean <= 1.0 and err_cov <= 1.0
    assert torch.equal(cov.view(torch.int64), cov.T.contiguous().view(torch.int64))     # cov[j,k] and cov[k,j]: the same bits
    mean2, cov2 = mel_ops.moments(x.to(DEV))
    assert torch.equal(mean.view(torch.int64), mean2.view(torch.int64)) and torch.equal(cov.view(torch.int64), cov2.view(torch.int64))
    return [mean, cov]


@pytest.mark.parametrize("shape", MOMENT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_are_the_float64_two_pass_definition_within_the_bound(shape):
    _moments_body(shape)


def test_moments_into_given_tensors_and_refusals():
    from musicgan_amd import _lib, mel_ops
    x = _moment_rows(33, 7).to(DEV)
    mean, cov = torch.empty(7, dtype=torch.float64, device=DEV), torch.empty(7, 7, dtype=torch.float64, device=DEV)
    got = mel_ops.moments(x, mean, cov)
    assert got[0] is mean and got[1] is cov
    want = mel_ops.moments(x)
    assert torch.equal(mean, want[0]) and torch.equal(cov, want[1])
    with pytest.raises(ValueError):
        mel_ops.moments(x[:1])
    with pytest.raises(_lib.MusicGanHipError):
        mel_ops.moments(x.double())
    with pytest.raises(_lib.MusicGanHipError):
        mel_ops.moments(x, mean.float(), cov)


# ------------------------------------------------------------------ Frechet
def _frechet(real, fake, splits=None):
    from musicgan_amd import metrics
    fd = metrics.Frechet()
    for lo in range(0, real.shape[0], splits or real.shape[0]):
        fd.feed_real(real[lo:lo + (splits or real.shape[0])].contiguous())
    for lo in range(0, fake.shape[0], splits or fake.shape[0]):
        fd.feed_fake(fake[lo:lo + (splits or fake.shape[0])].contiguous())
    return fd


def _frechet_body():
    from musicgan_amd import metrics
    real, fake = _moment_rows(300, 64).to(DEV), (_moment_rows(280, 64) * 1.2 + 0.3).to(DEV)
    whole = _frechet(real, fake)
    moments = whole.moments()
    for splits in (1, 7, 299):
        other = _frechet(real, fake, splits).moments()
        for a, b in zip(moments, other):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64)), splits
    value = whole.result()
    assert value == metrics.frechet_distance(*(t.cpu() for t in moments)) and value > 0.0
    scale = float(torch.trace(moments[1]) + torch.trace(moments[3]))
    ref = L.frechet(*(t.cpu().numpy() for t in moments))
    print(f"Frechet 300 / 280 x 64: {value:.9f} against scipy {ref:.9f} at scale {scale:.3f}")
    assert abs(value - ref) <= 1e-10 * scale
    same = _frechet(real, real.clone(), 50)
    zero, scale = same.result(), 2 * float(torch.trace(same.moments()[1]))
    print(f"Frechet of a set against itself: {zero:.3e} at scale {scale:.3f}")
    assert abs(zero) <= 1e-10 * scale
    return list(moments)


def test_frechet_any_feed_split_gives_the_same_bits_and_a_set_against_itself_zero():
    _frechet_body()


def test_frechet_refuses_too_few_rows_and_another_shape():
    from musicgan_amd import metrics
    fd = metrics.Frechet()
    fd.feed_real(_moment_rows(5, 4).to(DEV))
    fd.feed_fake(_moment_rows(1, 4).to(DEV))
    with pytest.raises(ValueError):
        fd.result()
    with pytest.raises(ValueError):
        fd.feed_fake(_moment_rows(3, 5).to(DEV))
    fd.feed_fake(_moment_rows(3, 4).to(DEV))
    assert np.isfinite(fd.result())                                      # 5 and 4 rows of 4 numbers


# ------------------------------------------------------------------ poisoned memory
def test_parity_bodies_on_poisoned_memory():
    """the parity bodies under poison.rule pointed at mel_ops: no guard band damaged by any launch, no argument changed that the
    table does not name, equal digests under both fills (nothing read that nobody wrote: the partial sums of the tiles below the
    diagonal are never read), nothing non-finite"""
    from musicgan_amd import mel_ops

    def run(p):
        assert mel_ops.moments_ws_bytes(2100, 33) == 3 * (33 + 33 * 33) * 8
        p.bodies = [_logmel_body(name) for name in ("64x64_8x8", "128x256_16x1", "128x256_16x256", "hand_bank_c1_of_3")]
        p.bodies += _moments_body((33, 7)) + _moments_body((2100, 33)) + _moments_body((300, 64)) + _frechet_body()
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=mel_ops, inplace=INPLACE)
    for a, b in zip(r0.bodies, r1.bodies):
        assert torch.equal(a, b)
    names = {name for name, _, _ in r1.calls}
    assert all(outs for name, _, outs in r1.calls if name in INPLACE)
    assert {"logmel_rows", "moments", "moments_ws_bytes"} <= names, names   # all three wrappers
    print(f"POISON logmel: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


# ------------------------------------------------------------------ evaluate_mel
ALL = ("fd", "nn", "prdc", "ndb")
KW = dict(level=4, nb_images=16, batch_size=3, seed=1)
FD_KEYS = ["fd", "fd_half", "fd_real"]
NN_KEYS = ["nn_fake", "nn_real", "nn_fake_min", "nn_real_min"]
PRDC_KEYS = ["precision", "recall", "density", "coverage"]
PRDC_KEYS = PRDC_KEYS + [k + "_real" for k in PRDC_KEYS]
NDB_KEYS = ["ndb", "jsd", "ndb_real", "jsd_real"]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """16 dataset entries of 64 x 64 and a generator at level 4, the full run and its printed text: made once for the tests below"""
    import contextlib
    import io
    import musicgan_amd
    root = tmp_path_factory.mktemp("logmel")
    data_dir, ck = tiny_corpus(root, files=8, seed=7, level=4)
    fn = musicgan_amd.__getattr__("evaluate_mel")                        # the lazy export itself
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        full = fn(ck, 8, data_dir, ALL, **KW)
    return dict(root=root, data=data_dir, ck=ck, fn=fn, full=full, text=text.getvalue())


def test_evaluate_mel_reports_every_metric_in_log_mel_space(corpus):
    full, text = corpus["full"], corpus["text"]
    print(text)
    assert list(full) == FD_KEYS + NN_KEYS + PRDC_KEYS + NDB_KEYS
    assert all(isinstance(v, float) and np.isfinite(v) for v in full.values()), full
    assert "Evaluate 16 real and 16 generated images of 64 x 64" in text
    # fd: 8 bands x 8 pools = 64 dimensions; half = 8 is below 2 x 64, so the bias line is there
    for name in FD_KEYS:
        assert f"FD [{name:>7}] = {full[name]:.6f} in log-mel space (8 bands x 8 pools)" in text
    assert "fd is dominated by its bias" in text and "fd_half near fd_real is what a perfect generator scores" in text
    # a Frechet distance is not negative; rounding may leave 1e-9 of the scale tr C1 + tr C2 for singular covariances.  The scale
    # of 64 log-mel dimensions of a noise corpus is above 1, so -1e-9 asks no less than -1e-9 x scale
    for name in FD_KEYS:
        assert full[name] >= -1e-9, (name, full[name])
    space = "in log-mel space (8 bands x 8 pools)"
    for line in text.splitlines():
        if line.startswith(("NN RMS", "PRDC [")) or line.startswith("NDB: 2 k-means bins"):
            assert space in line and "at 64 x 64" not in line, line
    assert text.count("NN RMS") == 2 and text.count("PRDC [") == 8 and "NDB: 2 k-means bins fitted on 8 real images " + space in text
    for name in ("ndb", "jsd", "precision", "recall", "coverage"):
        assert 0.0 <= full[name] <= 1.0 and 0.0 <= full[name + "_real"] <= 1.0
    assert full["nn_fake_min"] <= full["nn_fake"] and full["nn_real_min"] <= full["nn_real"] and full["nn_real_min"] > 0.0


def test_evaluate_mel_through_the_cli_single_metrics_and_batch_sizes(corpus, capsys):
    import musicgan_amd
    from musicgan_amd.__main__ import main
    fn, ck, data, full = corpus["fn"], corpus["ck"], corpus["data"], corpus["full"]
    js = str(corpus["root"] / "mel.json")
    main(["evaluate_mel", ck, "8", "-i", data, "--level", "4", "-n", "16", "--batch-size", "3", "--seed", "1",
          "--metrics", "fd,nn,prdc,ndb", "-o", js])
    with open(js) as f:
        loaded = json.load(f)
    assert loaded == full and list(loaded) == list(full)                 # a second run, through the CLI: the identical result
    assert capsys.readouterr().out == corpus["text"]
    for metric, keys in (("fd", FD_KEYS), ("nn", NN_KEYS), ("prdc", PRDC_KEYS), ("ndb", NDB_KEYS)):
        only = fn(ck, 8, data, (metric,), **KW)
        assert list(only) == keys and only == {k: full[k] for k in keys}, metric
    mixed = fn(ck, 8, data, ("ndb", "fd"), **KW)                         # the order run is METRICS', not the order asked for
    assert list(mixed) == FD_KEYS + NDB_KEYS
    # the real side does not depend on the batch size (the generated side may: the generator picks its kernels by it)
    real_keys = [k for k in full if k.endswith("_real") or k.startswith("nn_real")]
    assert len(real_keys) == 1 + 2 + 4 + 2 and "fd_real" in real_keys
    for bs in (1, 16):
        other = fn(ck, 8, data, ALL, **dict(KW, batch_size=bs))
        assert {k: other[k] for k in real_keys} == {k: full[k] for k in real_keys}, bs
    with pytest.raises(ValueError):
        fn(ck, 8, data, ("fd",), level=4, nb_images=3)
    capsys.readouterr()
    pixels = musicgan_amd.__getattr__("evaluate")(ck, 8, data, metrics=("nn",), **KW)   # evaluate itself still names its own space
    text = capsys.readouterr().out
    assert list(pixels) == NN_KEYS and text.count("at 64 x 64") == 2 and "log-mel" not in text
