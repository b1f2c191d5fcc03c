"""No GPU: the float64 restatement of the kernel distance (tests/kid_ref.py) is unbiased, its derived error bound holds against a
float32-chunked evaluation in torch CPU operators, `evaluate_mel` takes "kid" and `evaluate` does not, the wrappers of
musicgan_amd/kid_ops.py refuse what they must, and the new kernels use no scratch memory."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_ref as K  # noqa: E402


# ------------------------------------------------------------------ the reference
def _draws(shift: float):
    """mmd2 of 200 seeded pairs of sets of 24 rows x 16 dimensions of one Gaussian, the second set moved by `shift`"""
    return torch.tensor([K.mmd2(K.gaussian(24, 16, 2 * i), K.gaussian(24, 16, 2 * i + 1, shift)) for i in range(200)],
                        dtype=torch.float64)


def test_the_reference_estimate_is_unbiased_and_sees_a_shift():
    same, moved = _draws(0.0), _draws(0.5)
    for name, v in (("same", same), ("shifted by 0.5", moved)):
        se = float(v.std()) / math.sqrt(v.numel())
        print(f"mmd2, 200 draws of 24 x 16, {name}: mean {float(v.mean()):+.5f}, standard error {se:.5f}, mean / se "
              f"{float(v.mean()) / se:+.2f}, {int((v < 0).sum())} negative")
    se = float(same.std()) / math.sqrt(200)
    assert abs(float(same.mean())) <= 3.0 * se
    assert 50 <= int((same < 0).sum()) <= 150                            # an unbiased estimate of 0 is negative about as often as not
    assert float(moved.mean()) >= 20.0 * float(moved.std()) / math.sqrt(200)


# the deviation of mmd2 between two samples of ONE distribution at the shapes below, to one digit (float64, 20 seeded draws of
# standardised kid_ref.logmel_like rows; the test prints what it finds and holds it against these): the scale a distance is read at
SAME_STD = {(37, 64): 3e-2, (200, 512): 2e-3, (130, 520): 3e-3}


@pytest.mark.parametrize("shape", list(SAME_STD), ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_derived_bound_holds_against_float32_chunks(shape):
    n, d = shape
    x, y = K.logmel_like(n, d, 5), K.logmel_like(n, d, 6)
    mean, sd = K.moments(x)
    zx, zy = K.standardise(x, mean, sd), K.standardise(y, mean, sd)
    assert zx.dtype == torch.float32 and float(zx.double().mean(0).abs().max()) < 1e-6       # every column: mean 0, deviation 1
    assert float((zx.double().std(0) - 1.0).abs().max()) < 1e-6
    pair_err = (K.kernel_f32_chunks(zx, zy) - K.kernel(zx, zy)).abs()
    pair_ratio = float((pair_err / K.kernel_bound(zx, zy)).max())
    row_err = (K.rowsums(zx, zy, kernel_fn=K.kernel_f32_chunks) - K.rowsums(zx, zy)).abs()
    row_ratio = float((row_err / K.rowsums_bound(zx, zy)).max())
    err, bound = abs(K.mmd2(zx, zy, K.kernel_f32_chunks) - K.mmd2(zx, zy)), K.mmd2_bound(zx, zy)
    draws = []
    for i in range(20):
        a, b = K.logmel_like(n, d, 100 + 2 * i), K.logmel_like(n, d, 101 + 2 * i)
        draws.append(K.mmd2(K.standardise(a, mean, sd), K.standardise(b, mean, sd)))
    std = float(torch.tensor(draws, dtype=torch.float64).std())
    print(f"bound {n} x {d}: worst err / bound {pair_ratio:.2e} (pairs), {row_ratio:.2e} (row sums); mmd2 error {err:.2e}, bound "
          f"{bound:.2e}; same-distribution deviation {std:.2e} (stated: {SAME_STD[shape]:.0e}): bound / deviation {bound / std:.3f}, "
          f"error / deviation {err / std:.1e}")
    assert pair_ratio <= 1.0 and row_ratio <= 1.0 and err <= bound
    # the bound is a worst case over every rounding at once: it stays below 1e-3, which is of the size of the deviation between
    # two samples of one distribution, and the error that float32 chunks actually make is below a thousandth of that deviation
    assert bound < 1e-3
    assert 0.5 * SAME_STD[shape] <= std <= 2.0 * SAME_STD[shape]
    assert err <= 1e-3 * SAME_STD[shape]


def test_the_reference_standardises_as_defined():
    x = torch.tensor([[1.0, 5.0, 2.0], [3.0, 5.0, 2.5]])
    mean, sd = torch.tensor([2.0, 5.0, 0.0], dtype=torch.float64), torch.tensor([0.5, 0.0, float("nan")], dtype=torch.float64)
    assert K.standardise(x, mean, sd).tolist() == [[-2.0, 0.0, 0.0], [2.0, 0.0, 0.0]]
    k = K.kernel(torch.tensor([[1.0, 1.0]]), torch.tensor([[2.0, 4.0], [-1.0, -1.0]]))
    assert k.tolist() == [[64.0, 0.0]]                                   # (6 / 2 + 1)^3 and (-2 / 2 + 1)^3
    sums = K.rowsums(torch.eye(3), torch.eye(3), ia=[[0, 1], [2, 2]], ib=[[0, 1], [1, 0]], skip_diag=True)
    assert sums.tolist() == [[1.0, 1.0], [1.0, 1.0]]                     # off the diagonal every pair is orthogonal: k = 1


# ------------------------------------------------------------------ the sub-command
def _function_and_module():
    import musicgan_amd
    fn = musicgan_amd.__getattr__("evaluate_mel")
    return fn, sys.modules["musicgan_amd.evaluate_mel"]


def test_evaluate_mel_takes_kid_and_evaluate_does_not(monkeypatch):
    _, module = _function_and_module()
    from musicgan_amd import evaluate as pixels
    from musicgan_amd.__main__ import _FEATURE_MODES, _MEL_METRICS, _MEL_METRICS_ALL, build_parser, main
    assert module.METRICS == ("fd", "nn", "prdc", "ndb") == _MEL_METRICS
    assert module.METRICS_ALL == module.METRICS + ("kid",) == _MEL_METRICS_ALL and module.METRICS_ALL[-1] == "kid"
    assert tuple(module._RUNNERS) == module.METRICS_ALL
    assert "kid" not in sys.modules["musicgan_amd.evaluate"].METRICS_EVERY
    p = build_parser()
    a = p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data", "--metrics", "kid,fd"])
    assert _FEATURE_MODES["evaluate_mel"][4](a)["metrics"] == ("kid", "fd")
    for bad in ("kid,kid", "kid,", "KID"):
        with pytest.raises(SystemExit):
            p.parse_args(["evaluate_mel", "gen.pt", "32", "-i", "data", "--metrics", bad])
    with pytest.raises(SystemExit):
        p.parse_args(["evaluate", "gen.pt", "32", "-i", "data", "--metrics", "kid"])
    with pytest.raises(ValueError):
        pixels("/nonexistent/gen.pt", 8, "/nonexistent/data", metrics=("kid",))
    seen = []
    monkeypatch.setattr(module, "evaluate_mel", lambda *args, **kwargs: seen.append((args, kwargs)))
    main(["evaluate_mel", "gen.pt", "32", "-i", "data", "--level", "5", "--metrics", "kid"])
    assert seen == [(("gen.pt", 32, "data"), dict(level=5, nb_images=8192, batch_size=16, seed=0, output=None, metrics=("kid",)))]
    text = p._subparsers._group_actions[0].choices["evaluate_mel"].format_help()
    assert "fd,nn,prdc,ndb,kid" in text and "Kernel" in text


def test_evaluate_mel_refuses_kid_before_it_opens_a_file():
    import inspect
    fn, module = _function_and_module()
    assert inspect.signature(fn).parameters["metrics"].default == ("fd",)
    missing = "/nonexistent/gen.pt"
    for kw in (dict(metrics=("kid",), nb_images=3), dict(metrics=("kid", "kid")), dict(metrics=("kid",), level=3),
               dict(metrics=("fd", "kid"), nb_images=2), dict(metrics=("kid", "prdc"), nb_images=7), dict(metrics=("kid", "swd")),
               dict(metrics=("kid",), batch_size=0)):
        with pytest.raises(ValueError):
            fn(missing, 8, "/nonexistent/data", **kw)
    with pytest.raises(ValueError, match="kid needs at least 4 images"):
        fn(missing, 8, "/nonexistent/data", metrics=("kid",), nb_images=3)
    with pytest.raises(ValueError, match="'kid'"):                       # the refusal names every metric there is
        fn(missing, 8, "/nonexistent/data", metrics=("fid",))


# ------------------------------------------------------------------ the wrappers
def test_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from musicgan_amd import _lib, kid_ops, metrics, ops
    assert not [name for name in vars(ops) if "polyk" in name or "standardise" in name]
    x, mean, sd = torch.zeros(5, 7), torch.zeros(7, dtype=torch.float64), torch.ones(7, dtype=torch.float64)
    with pytest.raises(_lib.MusicGanHipError):
        kid_ops.standardise_rows(x, mean, sd)                            # well-formed, but on the host
    with pytest.raises(_lib.MusicGanHipError):
        kid_ops.polyk_rowsums(x, torch.zeros(3, 7))
    with pytest.raises(_lib.MusicGanHipError):
        kid_ops.polyk_rowsums(x, x, torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), skip_diag=True)
    for args in ((torch.zeros(5), mean, sd), (torch.zeros(0, 7), mean, sd), (torch.zeros(5, 2, 7), mean, sd), (x, mean[:6], sd),
                 (x, mean, sd.reshape(1, 7)), (x, mean, sd, torch.zeros(5, 6))):
        with pytest.raises(ValueError):
            kid_ops.standardise_rows(*args)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)           # noqa: E731
    bad = [dict(b=torch.zeros(3, 6)), dict(a=torch.zeros(5), b=torch.zeros(5)), dict(a=torch.zeros(0, 7)),
           dict(a=torch.zeros(5, 4097), b=torch.zeros(3, 4097)),          # d > 4096
           dict(skip_diag=True),                                          # 5 rows against 3
           dict(ia=i32(2, 4), ib=i32(2, 3), skip_diag=True),              # ma != mb through the lists
           dict(ia=torch.zeros(2, 4, dtype=torch.int64)), dict(ib=torch.zeros(2, 4)), dict(ia=i32(4)), dict(ia=i32(2, 0)),
           dict(ia=i32(2, 4), ib=i32(3, 4)),                              # two subset counts
           dict(out=torch.zeros(1, 4, dtype=torch.float64)), dict(ia=i32(2, 4), out=torch.zeros(5, dtype=torch.float64))]
    for change in bad:
        with pytest.raises(ValueError):
            kid_ops.polyk_rowsums(**dict(dict(a=x, b=torch.zeros(3, 7)), **change))
    assert kid_ops.polyk_ws_bytes(1, 5, 3) == 1 * 1 * 5 * 8
    assert kid_ops.polyk_ws_bytes(100, 1000, 1000) == 100 * 8 * 1000 * 8
    assert kid_ops.polyk_ws_bytes(3, 130, 257) == 3 * 3 * 130 * 8
    assert kid_ops.polyk_ws_bytes(0, 5, 3) == 0 and kid_ops.polyk_ws_bytes(1, 0, 3) == 0 and kid_ops.polyk_ws_bytes(65536, 5, 3) == 0
    for fn in (kid_ops.standardise_rows, kid_ops.polyk_rowsums, kid_ops.polyk_ws_bytes):
        assert fn.__doc__ and ("written" in fn.__doc__ or "host query" in fn.__doc__)
    # fewer than 2 rows, rows that are no rows, and the counts of KID: refused on the host
    for args in ((torch.zeros(1, 7), x), (x, torch.zeros(1, 7)), (x, torch.zeros(5, 6)), (x.reshape(5, 7, 1), x),
                 (torch.zeros(5, 4097), torch.zeros(5, 4097))):
        with pytest.raises(ValueError):
            metrics.poly_mmd2(*args)
    for kw in (dict(subsets=0), dict(subset_size=1), dict(subsets=True), dict(seed=0.5), dict(subsets=65536)):
        with pytest.raises(ValueError):
            metrics.KID(**kw)
        with pytest.raises(ValueError):
            metrics.kid_subsets(x, x, **kw)
    kid = metrics.KID()
    assert (kid.subsets, kid.subset_size, kid.seed) == (100, 1000, 0) and metrics.KID.KEYS == ("kid", "kid_std", "kid_full")
    for call in (kid.result, kid.per_sample, kid.standardised):
        with pytest.raises(ValueError):
            call()                                                       # nothing fed: m < 2


def test_new_kernels_use_no_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    hits = {k: v for k, v in usage.items() if "kid_standardise_k" in k or "kid_rowsums_k" in k or "kid_finish_k" in k}
    assert len(hits) == 4, sorted(hits)                                  # the tile kernel with vector and with scalar loads
    for name, u in hits.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)
