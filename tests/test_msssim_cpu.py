"""CPU: the float64 restatement of MS-SSIM (tests/msssim_ref.py, the yardstick of test_msssim_gpu.py) against closed forms, the host
queries and argument checks of musicgan_amd.metrics / ssim_ops, the `--metrics` option of the `evaluate` sub-command, and the
scratch use of the filter kernel."""
import inspect
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_ref as M  # noqa: E402
import swd_ref  # noqa: E402

SCALES = [((512, 512), 5), ((128, 128), 4), ((64, 64), 3), ((32, 32), 2), ((16, 16), 1), ((96, 352), 4), ((512, 5120), 5),
          ((64, 192), 3), ((11, 11), 1), ((22, 44), 2), ((24, 20), 1)]


def test_window_sums_to_one_and_is_symmetric():
    g64, g32 = M.window(torch.float64), M.window(torch.float32)
    assert g32.dtype == torch.float32 and torch.equal(g32.double(), g64)      # the float64 copy holds the float32 numbers
    assert abs(float(g64.sum()) - 1) <= 11 * 2.0 ** -25                        # eleven roundings of at most half an ulp of < 1
    assert torch.equal(g64, g64.flip(0)) and int(g64.argmax()) == 5
    exact = torch.exp(-(torch.arange(-5, 6, dtype=torch.float64) ** 2) / 4.5)
    assert float((g64 - exact / exact.sum()).abs().max()) <= 2.0 ** -25


def test_the_library_hands_the_kernels_the_same_window():
    from musicgan_amd import ssim_ops
    assert torch.equal(ssim_ops.ssim_window(), M.window(torch.float32))


@pytest.mark.parametrize("side,expect", SCALES)
def test_number_of_scales(side, expect):
    from musicgan_amd import metrics, ssim_ops
    assert metrics.ms_ssim_scales(*side) == expect and M.scales(*side) == expect and ssim_ops.ssim_scales(*side) == expect


def test_a_side_below_the_window_is_an_error():
    from musicgan_amd import metrics, ssim_ops
    for side in ((10, 10), (10, 512), (512, 10)):
        with pytest.raises(ValueError):
            metrics.ms_ssim_scales(*side)
        with pytest.raises(ValueError):
            metrics.MSSSIM(*side)
        assert ssim_ops.ssim_scales(*side) == 0 and ssim_ops.ssim_tiles(*side) == 0 and ssim_ops.ssim_scratch_bytes(4, 2, *side) == 0


def test_weights_are_the_standard_five_renormalised():
    assert torch.allclose(M.weights(5), torch.tensor(M.WEIGHTS, dtype=torch.float64), rtol=0, atol=4e-5)   # they sum to 1.0001
    for s in range(1, 6):
        assert float(M.weights(s).sum()) == pytest.approx(1.0, abs=1e-15)
    assert float(M.weights(1)[0]) == 1.0


def test_size_queries_need_no_gpu():
    from musicgan_amd import ssim_ops
    assert ssim_ops.ssim_tiles(512, 512) == 16 * 8 and ssim_ops.ssim_tiles(16, 16) == 1 and ssim_ops.ssim_tiles(11, 11) == 1
    assert ssim_ops.ssim_tiles(512, 5120) == 16 * 80 and ssim_ops.ssim_tiles(42, 74) == 1 and ssim_ops.ssim_tiles(43, 75) == 4
    slots = sum(ssim_ops.ssim_tiles(512 >> s, 512 >> s) for s in range(5)) * 3 * 2 * 2 * 8
    pyramid = sum((512 >> s) ** 2 for s in range(1, 5)) * 3 * 2 * 2 * 4
    assert ssim_ops.ssim_scratch_bytes(3, 2, 512, 512) == slots + pyramid


def test_ms_ssim_of_an_image_with_itself_is_one_in_the_reference():
    gen = torch.Generator().manual_seed(1)
    for shape in ((2, 2, 64, 64), (2, 1, 16, 24)):
        x = swd_ref.smooth_noise(*shape, 1, gen)
        assert torch.equal(M.ms_ssim(x, x), torch.ones(shape[0], dtype=torch.float64))
        assert torch.equal(M.terms(x, x), torch.ones(shape[0], M.scales(*shape[2:]), dtype=torch.float64))


def test_reference_closed_forms():
    """constant images: every sigma vanishes, cs = 1 and ssim is the luminance factor; a and -a: sigma_ab = -sigma_aa, so cs < 0
    wherever the variance exceeds C2 / 2 and the clamp makes the pair score 0"""
    a, b = torch.full((1, 2, 16, 16), 0.5, dtype=torch.float64), torch.full((1, 2, 16, 16), -0.25, dtype=torch.float64)
    lum = (2 * 0.5 * -0.25 + M.C1) / (0.25 + 0.0625 + M.C1)
    assert float(M.terms(a, b)[0, 0]) == pytest.approx(lum, rel=1e-6)   # the float32 taps do not sum to exactly 1
    assert float(M.ms_ssim(a, b)[0]) == 0.0                              # negative: clamped
    x = swd_ref.smooth_noise(1, 2, 32, 32, 1, torch.Generator().manual_seed(2))
    t = M.terms(x, -x)
    assert float(t[0, 0]) < 0 and float(M.ms_ssim(x, -x)[0]) == 0.0
    # symmetric in its arguments
    y = swd_ref.smooth_noise(1, 2, 32, 32, 2, torch.Generator().manual_seed(3))
    assert torch.equal(M.ms_ssim(x, y), M.ms_ssim(y, x))


def test_near_copies_score_higher_than_independent_images_in_the_reference():
    gen = torch.Generator().manual_seed(4)
    base = swd_ref.smooth_noise(1, 2, 64, 64, 2, gen)
    copies = (base + 0.05 * torch.randn(8, 2, 64, 64, generator=gen)).clamp(-1, 1)
    free = swd_ref.smooth_noise(8, 2, 64, 64, 2, gen)
    near, far = M.ms_ssim(copies[:4], copies[4:]).mean(), M.ms_ssim(free[:4], free[4:]).mean()
    assert float(near) > 0.5 > float(far)


def test_the_bound_covers_the_float32_cpu_evaluation():
    """the derived bound is a bound: the float32 evaluation with torch's own summation order lies within it, and it is small
    enough to mean something (terms are of the order 0.1 .. 1)"""
    gen = torch.Generator().manual_seed(5)
    for shape in ((3, 2, 64, 64), (3, 2, 16, 16)):
        a, b = M.pairs(shape, 0.5, gen)
        t64, t32, e = M.terms(a, b), M.terms(a, b, torch.float32), M.term_bounds(a, b)
        assert bool(((t32 - t64).abs() <= e).all()) and float(e.max()) < 1e-3
        v = M.value_bounds(t64, e)
        assert bool(((M.combine(t32) - M.combine(t64)).abs() <= v).all())


def test_argument_errors_are_value_errors_before_any_gpu_work():
    from musicgan_amd import metrics
    z = torch.zeros
    for fn in (metrics.ms_ssim, metrics.ms_ssim_terms):
        with pytest.raises(ValueError):
            fn(z(2, 2, 16, 16), z(3, 2, 16, 16))          # unequal shapes
        with pytest.raises(ValueError):
            fn(z(2, 16, 16), z(2, 16, 16))                 # not (n, C, H, W)
        with pytest.raises(ValueError):
            fn(z(1, 2, 10, 64), z(1, 2, 10, 64))           # a side below the window
        with pytest.raises(ValueError):
            fn(z(0, 2, 16, 16), z(0, 2, 16, 16))
    m = metrics.MSSSIM(32, 32, pairs=4)
    assert m.scales == 2
    with pytest.raises(ValueError):
        m.result()                                         # nothing fed
    with pytest.raises(ValueError):
        m.values
    with pytest.raises(ValueError):
        m.feed(z(1, 2, 16, 16), z(1, 2, 16, 16))           # wrong image size
    with pytest.raises(ValueError):
        m.feed(z(5, 2, 32, 32), z(5, 2, 32, 32))           # more than `pairs`
    with pytest.raises(ValueError):
        m.feed(z(2, 2, 32, 32), z(1, 2, 32, 32))
    with pytest.raises(ValueError):
        metrics.MSSSIM(32, 32, pairs=0)
    with pytest.raises(ValueError):
        metrics.MSSSIM(32, 32, channels=0)


def test_cpu_tensors_wrong_types_and_strides_are_refused_loudly():
    from musicgan_amd import _lib, metrics, ops, ssim_ops
    z = torch.zeros
    with pytest.raises(_lib.MusicGanHipError):
        metrics.ms_ssim(z(1, 2, 16, 16), z(1, 2, 16, 16))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.ms_ssim_terms(z(1, 2, 16, 16), z(1, 2, 16, 16))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.MSSSIM(16, 16, pairs=1).feed(z(1, 2, 16, 16), z(1, 2, 16, 16))
    with pytest.raises(_lib.MusicGanHipError):
        ssim_ops.ssim_scale(z(1, 2, 16, 16), z(1, 2, 16, 16), z(1, 2, 1, 2, dtype=torch.float64))
    with pytest.raises(_lib.MusicGanHipError):
        ssim_ops.ssim_finish(z(4, dtype=torch.float64), 1, 2, 16, 16, z(1, dtype=torch.float64))
    with pytest.raises(_lib.MusicGanHipError):
        ssim_ops.ssim_mean(z(4, dtype=torch.float64), z(1, dtype=torch.float64))
    with pytest.raises(_lib.MusicGanHipError):
        ssim_ops.ms_ssim_into(z(1, 2, 16, 16), z(1, 2, 16, 16), z(1, dtype=torch.float64))
    # the type and layout checks themselves, on the checker the wrappers share
    class Cuda:   # stands for a device tensor: the checks read these three attributes only
        def __init__(self, t, contiguous=True):
            self.is_cuda, self.dtype, self._c = True, t.dtype, contiguous

        def is_contiguous(self):
            return self._c
    ops._chk_typed("x", Cuda(z(1)))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1, dtype=torch.float64)))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1), contiguous=False))
    with pytest.raises(_lib.MusicGanHipError):
        ops._chk_typed("x", Cuda(z(1)), dtype=torch.float64)


def test_ops_gains_no_public_name():
    """the wrappers live in ssim_ops: musicgan_amd.ops names nothing of MS-SSIM"""
    from musicgan_amd import ops
    assert not [n for n in vars(ops) if "ssim" in n.lower()]


def test_metrics_option_of_the_evaluate_parser():
    from musicgan_amd.__main__ import _MODES, build_parser
    p = build_parser()
    _, _, _, pos, kw = _MODES["evaluate"]
    today = ["evaluate", "g.pt", "8", "-i", "d", "--level", "2", "-n", "8", "--batch-size", "4", "--seed", "3", "-o", "swd.json"]
    a = p.parse_args(today)
    assert a.metrics is None
    assert kw(a) == dict(level=2, nb_images=8, batch_size=4, seed=3, output="swd.json")      # as without the option
    a = p.parse_args(today + ["--metrics", "swd,msssim"])
    assert pos(a) == ("g.pt", 8, "d")
    assert kw(a) == dict(level=2, nb_images=8, batch_size=4, seed=3, output="swd.json", metrics=("swd", "msssim"))
    assert kw(p.parse_args(today + ["--metrics", "msssim"]))["metrics"] == ("msssim",)
    for bad in ("fid", "swd,fid", "", "swd,swd"):
        with pytest.raises(SystemExit):
            p.parse_args(today + ["--metrics", bad])


def test_evaluate_keeps_its_pinned_signature():
    import musicgan_amd
    from musicgan_amd.__main__ import _MODES
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"]
    sig = inspect.signature(musicgan_amd.evaluate)
    assert list(sig.parameters)[:4] == ["gen_dict_state", "rand_channels", "input_dataset", "metrics"]
    m = sig.parameters["metrics"]
    assert m.kind is m.POSITIONAL_OR_KEYWORD and m.default == ("swd",)
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == \
        dict(level=7, nb_images=8192, batch_size=16, seed=0, output=None)


def test_evaluate_refuses_unknown_metrics_before_any_work():
    import musicgan_amd
    for bad in ((), ("fid",), ("swd", "swd")):
        with pytest.raises(ValueError):
            musicgan_amd.evaluate("missing.pt", 8, "missing", bad)


def test_ssim_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"ssim_scale_k", r"ssim_finish_k", r"ssim_mean_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: {u.get('ScratchSize [bytes/lane]')} B/lane of scratch memory"
            assert u.get("VGPRs", 0) > 0
