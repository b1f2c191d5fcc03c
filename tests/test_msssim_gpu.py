"""GPU: the MS-SSIM kernels (csrc/ssim.hip) and musicgan_amd.metrics / evaluate against the float64 restatement of the definition
in tests/msssim_ref.py.  Every bound is derived (msssim_ref.term_bounds, the rounding analysis of a float32 evaluation in any
order, or twice the float32 CPU evaluation's own error), none is fitted to what the kernels give."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_ref as M  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402
import poison  # noqa: E402
import swd_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(6, 2, 512, 512), (8, 2, 128, 128), (8, 2, 64, 192), (8, 2, 32, 32), (8, 2, 16, 16), (3, 1, 96, 352)]
# the tensor arguments the wrappers of musicgan_amd/ssim_ops.py write, each all of it (their docstrings)
INPLACE = {
    "ssim_scale": ("slots", "a_next", "b_next"),   # "into all of slots ... into all of a_next and b_next"
    "ssim_finish": ("values", "terms"),            # "values[row .. row + n] ... terms[row .. row + n]"
    "ssim_mean": ("out",),
    "ms_ssim_into": ("values", "terms"),
}


def _parity(shape, rho, seed=43):
    """ms_ssim_terms and ms_ssim on the GPU against float64, on pairs whose terms are all clear of the clamp (the seed was picked
    on the float64 side alone: every term of every shape is >= 0.19 with it)"""
    from musicgan_amd import metrics
    a, b = M.pairs(shape, rho, torch.Generator().manual_seed(seed + shape[2] + int(10 * rho)))
    t64, t32, e = M.terms(a, b), M.terms(a, b, torch.float32), M.term_bounds(a, b)
    assert bool((t64 > 0.05).all()), f"{shape} rho {rho}: a term of {float(t64.min()):.4f} is too close to the clamp for this comparison"
    got_t = metrics.ms_ssim_terms(a.to(DEV), b.to(DEV))
    got_v = metrics.ms_ssim(a.to(DEV), b.to(DEV))
    assert got_t.dtype == torch.float64 and got_t.is_cuda and tuple(got_t.shape) == (shape[0], M.scales(*shape[2:]))
    assert got_v.dtype == torch.float64 and got_v.is_cuda and tuple(got_v.shape) == (shape[0],)
    own_t = (t32 - t64).abs()
    bound_t = torch.maximum(e, 2 * own_t)
    err_t = (got_t.cpu() - t64).abs()
    v64, v32 = M.combine(t64), M.combine(t32)
    bound_v = torch.maximum(M.value_bounds(t64, e), 2 * (v32 - v64).abs())
    err_v = (got_v.cpu() - v64).abs()
    print(f"msssim {shape} rho {rho}: terms {float(t64.min()):.3f} .. {float(t64.max()):.3f}, values {float(v64.min()):.3f} .. "
          f"{float(v64.max()):.3f}; term err {float(err_t.max()):.3e} (fp32 CPU {float(own_t.max()):.3e}, derived bound "
          f"{float(e.min()):.3e} .. {float(e.max()):.3e}), worst err / bound {float((err_t / bound_t).max()):.4f}; value err "
          f"{float(err_v.max()):.3e}, worst err / bound {float((err_v / bound_v).max()):.4f}")
    assert bool((err_t <= bound_t).all()), (shape, rho, float((err_t / bound_t).max()))
    assert bool((err_v <= bound_v).all()), (shape, rho, float((err_v / bound_v).max()))
    return got_v


@pytest.mark.parametrize("rho", [0.5, 0.9])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_terms_and_values_match_the_float64_definition(shape, rho):
    _parity(shape, rho)


@pytest.mark.parametrize("side", [32, 16])
def test_a_negative_mean_is_clamped_to_exactly_zero(side):
    """unrelated images (rho = 0) at small sizes: some means are negative in float64; such a pair scores exactly 0.0, and
    ms_ssim_terms still reports the negative mean within its bound"""
    from musicgan_amd import metrics
    shape = (8, 2, side, side)
    a, b = M.pairs(shape, 0.0, torch.Generator().manual_seed(50 + side))
    t64, t32, e = M.terms(a, b), M.terms(a, b, torch.float32), M.term_bounds(a, b)
    negative = (t64 < 0).any(1)
    assert bool(negative.any()), f"no negative term at {side} x {side}: {t64}"
    got_t, got_v = metrics.ms_ssim_terms(a.to(DEV), b.to(DEV)).cpu(), metrics.ms_ssim(a.to(DEV), b.to(DEV)).cpu()
    bound_t = torch.maximum(e, 2 * (t32 - t64).abs())
    err_t = (got_t - t64).abs()
    print(f"clamp {side}: most negative term {float(t64.min()):.4f}, {int(negative.sum())} of {shape[0]} pairs clamped, "
          f"term err / bound {float((err_t / bound_t).max()):.4f}, values {got_v.tolist()}")
    assert bool((err_t <= bound_t).all())
    assert bool((got_v[negative] == 0.0).all()), got_v
    assert torch.equal(M.combine(t64)[negative], torch.zeros(int(negative.sum()), dtype=torch.float64))
    assert bool(((got_v >= 0) & (got_v <= 1)).all())


@pytest.mark.parametrize("shape", [(4, 2, 512, 512), (5, 2, 64, 192), (5, 3, 16, 16), (2, 1, 96, 352)])
def test_identity_is_exactly_one_and_the_arguments_commute_bit_for_bit(shape):
    from musicgan_amd import metrics
    a, b = M.pairs(shape, 0.5, torch.Generator().manual_seed(60))
    a, b = a.to(DEV), b.to(DEV)
    assert torch.equal(metrics.ms_ssim(a, a).cpu(), torch.ones(shape[0], dtype=torch.float64))
    assert torch.equal(metrics.ms_ssim_terms(b, b).cpu(), torch.ones(shape[0], M.scales(*shape[2:]), dtype=torch.float64))
    assert torch.equal(metrics.ms_ssim(a, b), metrics.ms_ssim(b, a))
    assert torch.equal(metrics.ms_ssim_terms(a, b), metrics.ms_ssim_terms(b, a))


def _fed(a, b, splits):
    from musicgan_amd import metrics
    m = metrics.MSSSIM(a.shape[2], a.shape[3], channels=a.shape[1], pairs=a.shape[0])
    lo = 0
    for n in splits:
        m.feed(a[lo:lo + n].contiguous(), b[lo:lo + n].contiguous())
        lo += n
    return m.values.clone(), m.result()


@pytest.mark.parametrize("shape", [(8, 2, 128, 128), (8, 2, 64, 192), (8, 2, 16, 16)])
def test_feeding_in_any_split_gives_the_same_bits(shape):
    from musicgan_amd import metrics
    a, b = M.pairs(shape, 0.5, torch.Generator().manual_seed(61))
    a, b = a.to(DEV), b.to(DEV)
    values, mean = _fed(a, b, [8])
    assert torch.equal(values, metrics.ms_ssim(a, b))
    assert isinstance(mean, float) and abs(mean - float(values.cpu().mean())) <= 1e-14   # eight values <= 1 added in another order
    for splits in ([3, 3, 2], [1] * 8, [8]):
        v, m = _fed(a, b, splits)
        assert torch.equal(v, values) and m == mean, splits
    # a pair's value does not depend on its neighbours in the batch or on its position
    assert torch.equal(metrics.ms_ssim(a.flip(0).contiguous(), b.flip(0).contiguous()).flip(0), values)


def test_feeding_does_not_synchronise():
    from musicgan_amd import metrics
    a, b = M.pairs((12, 2, 64, 64), 0.5, torch.Generator().manual_seed(62))
    a, b = a.to(DEV), b.to(DEV)
    m = metrics.MSSSIM(64, 64, pairs=12)
    m.feed(a[:4].contiguous(), b[:4].contiguous())   # warm-up: library load, the value buffer
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for lo in (4, 8):
            m.feed(a[lo:lo + 4], b[lo:lo + 4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert 0 < m.result() < 1 and torch.equal(m.values, metrics.ms_ssim(a, b))


def test_near_copies_score_higher_than_independent_images():
    from musicgan_amd import metrics
    gen = torch.Generator().manual_seed(63)
    base = swd_ref.smooth_noise(1, 2, 64, 64, 2, gen)
    copies = (base + 0.05 * torch.randn(16, 2, 64, 64, generator=gen)).clamp(-1, 1)
    free = swd_ref.smooth_noise(16, 2, 64, 64, 2, gen)
    out = []
    for x in (copies, free):
        m = metrics.MSSSIM(64, 64, pairs=8)
        m.feed(x[:8].to(DEV), x[8:].to(DEV))
        out.append((m.result(), float(M.ms_ssim(x[:8], x[8:]).mean())))
    (near, near64), (far, far64) = out
    print(f"near copies {near:.4f} (f64 {near64:.4f}), independent images {far:.4f} (f64 {far64:.4f})")
    assert near64 > far64 and near > far


@pytest.mark.parametrize("shape", [(8, 2, 128, 128), (8, 2, 16, 16), (8, 2, 64, 192)], ids=["multi-scale", "single-scale", "non-square"])
def test_parity_body_on_poisoned_memory(shape):
    """the parity body and a fed MSSSIM under poison.rule pointed at ssim_ops: no guard band damaged by any launch, no argument
    changed that the table does not name, equal digests under both fills (nothing read that nobody wrote), nothing non-finite"""
    from musicgan_amd import metrics, ssim_ops

    def case(p):
        _parity(shape, 0.5)
        a, b = M.pairs(shape, 0.9, torch.Generator().manual_seed(64))
        m = metrics.MSSSIM(shape[2], shape[3], channels=shape[1], pairs=shape[0])
        m.feed(a.to(DEV), b.to(DEV))
        p.mean = m.result()
        torch.cuda.synchronize()

    r0, r1 = poison.rule(case, module=ssim_ops, inplace=INPLACE)
    assert r0.mean == r1.mean and 0 < r1.mean < 1
    names = {name for name, _, _ in r1.calls}
    assert {"ms_ssim_into", "ssim_mean"} <= names, names
    assert {"ssim_scale", "ssim_finish"} <= r1.census.ops()
    assert any(outs for name, _, outs in r1.calls if name == "ms_ssim_into")
    print(f"POISON msssim {shape}: {len(r1.calls)} calls ({r1.launches} with nested), ops {sorted(r1.census.ops())}")


def test_evaluate_with_msssim_on_a_tiny_corpus(tmp_path, capsys):
    import musicgan_amd
    from musicgan_amd.__main__ import main
    data_dir, ck = tiny_corpus(tmp_path, files=2, seed=5, level=2)      # 2 files x 2 samples
    capsys.readouterr()
    default = musicgan_amd.evaluate(ck, 8, str(data_dir), level=2, nb_images=8, batch_size=3, seed=1)
    text = capsys.readouterr().out
    assert list(default) == ["16", "avg"] and "MS-SSIM" not in text            # no new flag: what it printed and returned before
    both = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("swd", "msssim"), level=2, nb_images=8, batch_size=3, seed=1)
    text = capsys.readouterr().out
    assert list(both) == ["16", "avg", "msssim_real", "msssim_fake"]
    assert both["16"] == default["16"] and both["avg"] == default["avg"]
    assert all(isinstance(both[k], float) and 0.0 <= both[k] <= 1.0 for k in ("msssim_real", "msssim_fake")), both
    assert "MS-SSIM [real]" in text and "MS-SSIM [fake]" in text and "[ 16]" in text
    js = str(tmp_path / "eval.json")
    main(["evaluate", ck, "8", "-i", str(data_dir), "--level", "2", "-n", "8", "--batch-size", "3", "--seed", "1",
          "--metrics", "swd,msssim", "-o", js])
    with open(js) as f:
        assert json.load(f) == both                                            # the identical result through the CLI
    assert list(json.load(open(js))) == list(both)
    for bs in (1, 2, 16):                                                       # ... and at any batch size
        assert musicgan_amd.evaluate(ck, 8, str(data_dir), ("swd", "msssim"), level=2, nb_images=8, batch_size=bs, seed=1) == both, bs
    only = musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("msssim",), level=2, nb_images=8, batch_size=3, seed=1)
    assert only == {k: both[k] for k in ("msssim_real", "msssim_fake")} and list(only) == ["msssim_real", "msssim_fake"]
    with pytest.raises(ValueError):
        musicgan_amd.evaluate(ck, 8, str(data_dir), metrics=("msssim",), level=2, nb_images=1)   # nothing to pair
