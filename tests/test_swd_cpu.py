"""CPU: the float64 restatement of the sliced Wasserstein distance (tests/swd_ref.py, the yardstick of test_swd_gpu.py) against
closed forms, the draw order and argument checks of musicgan_amd.metrics, the `evaluate` sub-command's parser, and the scratch
use of the projection and sort kernels."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_ref as R  # noqa: E402


def test_pyramid_of_a_constant_image_is_constant_and_zero():
    x = torch.full((2, 2, 64, 32), 0.7, dtype=torch.float64)
    p = R.pyramid(x, 3)
    assert [tuple(t.shape[2:]) for t in p] == [(64, 32), (32, 16), (16, 8)]
    for lap in p[:-1]:
        assert float(lap.abs().max()) <= 1e-15
    assert float((p[-1] - 0.7).abs().max()) <= 1e-15


def test_pyramid_reconstructs_its_input():
    x = torch.randn(3, 2, 64, 96, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    assert float((R.reconstruct(R.pyramid(x, 3)) - x).abs().max()) <= 1e-12


def test_up_touches_only_the_even_taps():
    """up() of an impulse is the 4 g stencil around its (even) position: the weights the kernel's parity rule evaluates"""
    x = torch.zeros(1, 1, 8, 8, dtype=torch.float64)
    x[0, 0, 3, 4] = 1.0
    u = R.up(x)
    k = torch.tensor(R.K5, dtype=torch.float64) / 8
    assert torch.allclose(u[0, 0, 4:9, 6:11], torch.outer(k, k), atol=0, rtol=1e-15)
    assert float(u.sum()) == pytest.approx(4.0, abs=1e-12)


def test_swd_of_a_set_with_itself_is_zero():
    gen = torch.Generator().manual_seed(1)
    x = R.smooth_noise(4, 2, 32, 32, 1, gen)
    from musicgan_amd import metrics
    draws = metrics.draw([(32, 32), (16, 16)], 2, 4, 16, 7, 2, 8, seed=3)
    same = [(a, a, d) for a, _, d in draws]
    out, _ = R.swd(x, x, same)
    assert out == {"32": 0.0, "16": 0.0, "avg": 0.0}


def test_distance_of_a_shift_along_a_direction_is_the_shift():
    gen = torch.Generator().manual_seed(2)
    a = torch.randn(500, 98, generator=gen, dtype=torch.float64)
    e1 = torch.zeros(1, 98, dtype=torch.float64)
    e1[0, 0] = 1.0
    for mu in (0.25, -3.0):
        b = a + mu * e1
        assert float(R.sliced_distance(a, b, e1)) * 1000 == pytest.approx(1000 * abs(mu), rel=1e-12)


def test_descriptors_are_channel_major_neighbourhoods():
    lvl = torch.arange(2 * 2 * 16 * 20, dtype=torch.float64).reshape(2, 2, 16, 20)
    cen = torch.tensor([[[3, 3], [12, 16]], [[8, 9], [3, 16]]], dtype=torch.int32)
    d = R.descriptors(lvl, cen)
    assert tuple(d.shape) == (4, 98)
    assert torch.equal(d[1].reshape(2, 7, 7), lvl[0, :, 9:16, 13:20])
    assert torch.equal(d[2].reshape(2, 7, 7), lvl[1, :, 5:12, 6:13])
    mean, std = R.channel_stats(d, 2)
    assert float(mean[0]) == pytest.approx(float(d[:, :49].mean())) and float(std[1]) == pytest.approx(float(d[:, 49:].std(unbiased=False)))
    dn = R.normalise(d, 2)
    assert float(dn[:, :49].mean()) == pytest.approx(0, abs=1e-12) and float(dn[:, 49:].pow(2).mean()) == pytest.approx(1, rel=1e-12)


def test_draw_order_and_ranges():
    from musicgan_amd import metrics
    sides = metrics.pyramid_sides(64, 128)
    assert sides == [(64, 128), (32, 64), (16, 32)]
    assert metrics.pyramid_sides(512, 512) == [(512 >> i, 512 >> i) for i in range(6)]
    a = metrics.draw(sides, 2, 5, 11, 7, 3, 4, seed=9)
    b = metrics.draw(sides, 2, 5, 11, 7, 3, 4, seed=9)
    c = metrics.draw(sides, 2, 5, 11, 7, 3, 4, seed=10)
    for (h, w), (ca, cb, d), (ca2, cb2, d2), (ca3, _, _) in zip(sides, a, b, c):
        assert ca.dtype == torch.int32 and tuple(ca.shape) == (5, 11, 2) and tuple(cb.shape) == (5, 11, 2)
        assert d.dtype == torch.float32 and tuple(d.shape) == (3, 4, 98)
        assert torch.equal(ca, ca2) and torch.equal(cb, cb2) and torch.equal(d, d2)
        assert not torch.equal(ca, cb) and not torch.equal(ca, ca3)
        for cen in (ca, cb):
            assert int(cen[..., 0].min()) >= 3 and int(cen[..., 0].max()) < h - 3
            assert int(cen[..., 1].min()) >= 3 and int(cen[..., 1].max()) < w - 3
        assert float((d.double().norm(dim=2) - 1).abs().max()) <= 1e-6
    # the stated order: one generator; per level rows then columns of A, those of B, then the directions
    gen = torch.Generator().manual_seed(9)
    for (h, w), (ca, cb, d) in zip(sides, a):
        for cen in (ca, cb):
            assert torch.equal(torch.randint(3, h - 3, (5, 11), generator=gen).int(), cen[..., 0])
            assert torch.equal(torch.randint(3, w - 3, (5, 11), generator=gen).int(), cen[..., 1])
        raw = torch.randn(3, 4, 98, generator=gen, dtype=torch.float32)
        assert torch.equal(raw / raw.norm(dim=2, keepdim=True), d)


def test_swd_object_takes_the_seed_derived_draws_and_checks_its_arguments():
    from musicgan_amd import metrics
    s = metrics.SWD(64, 64, images=6, patches_per_image=8, dir_repeats=2, dirs_per_repeat=4, seed=5)
    assert s.sides == [(64, 64), (32, 32), (16, 16)]
    ref = metrics.draw(s.sides, 2, 6, 8, 7, 2, 4, seed=5)
    assert all(torch.equal(x, y) for got, exp in zip(s.draws, ref) for x, y in zip(got, exp))
    with pytest.raises(ValueError):
        s.result()                                           # nothing fed: the counts do not reach `images`
    with pytest.raises(ValueError):
        s.feed_real(torch.zeros(2, 2, 32, 32))               # wrong image size
    with pytest.raises(ValueError):
        s.feed_fake(torch.zeros(7, 2, 64, 64))               # more than `images`
    with pytest.raises(ValueError):
        metrics.SWD(8, 8)                                    # smaller than the smallest level
    with pytest.raises(ValueError):
        metrics.SWD(64, 64, patch=7, min_side=4)             # a level smaller than the patch
    with pytest.raises(ValueError):
        metrics.SWD(64, 64, patch=6)
    with pytest.raises(ValueError):
        metrics.SWD(64, 64, images=0)


def test_argument_errors_are_value_errors_before_any_gpu_work():
    from musicgan_amd import metrics
    with pytest.raises(ValueError):
        metrics.laplacian_pyramid(torch.zeros(1, 2, 30, 32), 3)          # 30 is not divisible by 4
    with pytest.raises(ValueError):
        metrics.laplacian_pyramid(torch.zeros(1, 2, 32, 32), 0)
    with pytest.raises(ValueError):
        metrics.laplacian_pyramid(torch.zeros(2, 32, 32), 2)
    with pytest.raises(ValueError):
        metrics.patch_descriptors(torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 2, dtype=torch.int32))   # level smaller than the patch
    with pytest.raises(ValueError):
        metrics.patch_descriptors(torch.zeros(2, 2, 16, 16), torch.zeros(1, 3, 2, dtype=torch.int32))  # unequal counts
    with pytest.raises(ValueError):
        metrics.patch_descriptors(torch.zeros(1, 2, 16, 16), torch.zeros(1, 3, 2, dtype=torch.int32), row=3)
    d, st = torch.zeros(6, 98), torch.zeros(2, 2, 2, dtype=torch.float64)
    with pytest.raises(ValueError):
        metrics.patch_descriptors(torch.zeros(2, 2, 16, 16), torch.zeros(2, 3, 2, dtype=torch.int32), out=(d, st), row=3)  # does not fit
    with pytest.raises(ValueError):
        metrics.sliced_wasserstein(d, st, torch.zeros(9, 98), st, torch.zeros(4, 98))   # unequal counts
    with pytest.raises(ValueError):
        metrics.sliced_wasserstein(d, st, d, st, torch.zeros(4, 97))
    with pytest.raises(ValueError):
        metrics.segmented_sort_(torch.zeros(5))


def test_cpu_tensors_are_refused_loudly():
    from musicgan_amd import _lib, metrics
    d, st = torch.zeros(6, 98), torch.zeros(2, 2, 2, dtype=torch.float64)
    with pytest.raises(_lib.MusicGanHipError):
        metrics.laplacian_pyramid(torch.zeros(1, 2, 32, 32), 2)
    with pytest.raises(_lib.MusicGanHipError):
        metrics.laplacian_pyramid(torch.zeros(1, 2, 32, 32), 1)
    with pytest.raises(_lib.MusicGanHipError):
        metrics.patch_descriptors(torch.zeros(1, 2, 16, 16), torch.zeros(1, 3, 2, dtype=torch.int32))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.sliced_wasserstein(d, st, d, st, torch.zeros(4, 98))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.segmented_sort_(torch.zeros(2, 5))
    with pytest.raises(_lib.MusicGanHipError):
        metrics.SWD(16, 16, images=1).feed_real(torch.zeros(1, 2, 16, 16))


def test_evaluate_is_the_fifth_mode():
    from musicgan_amd.__main__ import _MODES, build_parser
    assert list(_MODES) == ["create_dataset", "train", "generate", "view_audio", "evaluate"]
    assert _MODES["evaluate"][:2] == ("evaluate", "evaluate")
    p = build_parser()
    a = p.parse_args(["evaluate", "gen_3.pt", "32", "-i", "data"])
    assert (a.mode, a.gen_dict_state, a.rand_channels, a.input_dataset) == ("evaluate", "gen_3.pt", 32, "data")
    assert (a.level, a.nb_images, a.batch_size, a.seed, a.output) == (7, 8192, 16, 0, None)
    a = p.parse_args(["evaluate", "g.pt", "8", "-i", "d", "--level", "2", "-n", "8", "--batch-size", "4", "--seed", "3", "-o", "swd.json"])
    _, _, _, pos, kw = _MODES["evaluate"]
    assert pos(a) == ("g.pt", 8, "d")
    assert kw(a) == dict(level=2, nb_images=8, batch_size=4, seed=3, output="swd.json")
    with pytest.raises(SystemExit):
        p.parse_args(["evaluate", "g.pt", "8"])
    import inspect
    import musicgan_amd
    sig = inspect.signature(musicgan_amd.evaluate)
    assert list(sig.parameters)[:3] == ["gen_dict_state", "rand_channels", "input_dataset"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == \
        dict(level=7, nb_images=8192, batch_size=16, seed=0, output=None)


def test_swd_kernels_do_not_use_scratch_memory():
    from musicgan_amd import _build
    _build.build()
    usage = _build.resource_usage()
    for pat in (r"swd_project_k", r"swd_sort_tile_k", r"swd_sort_global_k"):
        hits = {k: v for k, v in usage.items() if re.search(pat, k)}
        assert hits, f"no kernel matches {pat}"
        for name, u in hits.items():
            assert u.get("ScratchSize [bytes/lane]", 0) == 0, f"{name}: {u.get('ScratchSize [bytes/lane]')} B/lane of scratch memory"
            assert u.get("VGPRs", 0) > 0
