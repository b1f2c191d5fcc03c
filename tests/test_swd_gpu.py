"""GPU: the sliced-Wasserstein kernels (csrc/swd.hip) and musicgan_amd.metrics / evaluate against the float64 restatement of the
definition in tests/swd_ref.py.  Every bound is derived (rounding analysis of the float32 evaluation, or twice the float32 CPU
evaluation's own error), none is fitted to what the kernels give."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_ref as R  # noqa: E402
from eval_corpus import tiny_corpus  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24


def _corner_impulses(n, c, h, w):
    x = torch.zeros(n, c, h, w)
    for k, (y, xx) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
        x[k % n, k % c, y, xx] += 1.0 + k
    return x


@pytest.mark.parametrize("shape,levels", [((3, 2, 64, 64), 3), ((2, 2, 32, 96), 2), ((1, 1, 512, 512), 6)])
@pytest.mark.parametrize("kind", ["random", "corners"])
def test_pyramid_matches_the_float64_definition(shape, levels, kind):
    from musicgan_amd import metrics
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(11)) if kind == "random" else _corner_impulses(*shape)
    got = metrics.laplacian_pyramid(x.to(DEV), levels)
    f64, f32 = R.pyramid(x.double(), levels), R.pyramid(x, levels)
    assert len(got) == levels
    xmax = float(x.abs().max())
    for i, (g, e64, e32) in enumerate(zip(got, f64, f32)):
        assert g.shape == e64.shape and g.dtype == torch.float32
        err = float((g.cpu().double() - e64).abs().max())
        own = float((e32.double() - e64).abs().max())
        bound = max(32 * U * (i + 2) * xmax, 2 * own)
        print(f"pyramid {shape} {kind} level {i}: err {err:.3e} bound {bound:.3e} (fp32 CPU {own:.3e})")
        assert err <= bound, (i, err, bound)


@pytest.mark.parametrize("mean", [1.0, 100.0])
def test_gather_copies_patches_and_sums_in_float64(mean):
    from musicgan_amd import metrics
    gen = torch.Generator().manual_seed(12)
    n, c, h, w, p = 7, 2, 24, 40, 33
    lvl = torch.randn(n, c, h, w, generator=gen) + mean
    lvl[:, 1] *= 3.0
    cen = torch.stack((torch.randint(3, h - 3, (n, p), generator=gen), torch.randint(3, w - 3, (n, p), generator=gen)), 2).int()
    cen[0, 0], cen[0, 1], cen[1, 0], cen[1, 1] = (torch.tensor(v, dtype=torch.int32) for v in
                                                  ((3, 3), (h - 4, w - 4), (3, w - 4), (h - 4, 3)))
    exp = R.descriptors(lvl, cen)
    desc, stats = metrics.patch_descriptors(lvl.to(DEV), cen.to(DEV))
    assert torch.equal(desc.cpu(), exp)
    # appended in batches of 3, 3, 1 at row offsets: the same buffers, bit for bit
    out = (torch.zeros_like(desc), torch.zeros_like(stats))
    for lo in (0, 3, 6):
        metrics.patch_descriptors(lvl[lo:lo + 3].to(DEV), cen[lo:lo + 3].to(DEV), out=out, row=lo * p)
    assert torch.equal(out[0], desc) and torch.equal(out[1], stats)
    norm = metrics.channel_stats(stats, p * 49).cpu().double()
    m64, s64 = R.channel_stats(exp.double(), c)
    for ch in range(c):
        m_err, s_rel = abs(float(norm[ch, 0] - m64[ch])), abs(float(norm[ch, 2] / s64[ch]) - 1)
        r_rel = abs(float(norm[ch, 1] * s64[ch]) - 1)
        print(f"stats mean {mean} ch {ch}: mean err {m_err:.3e} (bound {4 * U * max(abs(float(m64[ch])), float(s64[ch])):.3e}), "
              f"std rel {s_rel:.3e}, 1/std rel {r_rel:.3e} (bound {4 * U:.3e})")
        assert m_err <= 4 * U * max(abs(float(m64[ch])), float(s64[ch]))
        assert s_rel <= 4 * U and r_rel <= 4 * U


@pytest.mark.parametrize("c", [1, 2, 3])
@pytest.mark.parametrize("d", [1, 128])
@pytest.mark.parametrize("m", [1, 63, 64, 1000, 128 * 37])
def test_projection_within_the_dot_product_bound(m, d, c):
    from musicgan_amd import ops
    gen = torch.Generator().manual_seed(13 + m + d + c)
    k = c * 49
    desc = torch.randn(m, k, generator=gen) * 2 + 0.5
    norm = torch.empty(c, 3)
    norm[:, 0] = torch.randn(c, generator=gen)
    norm[:, 1] = torch.rand(c, generator=gen) + 0.25
    norm[:, 2] = 1 / norm[:, 1]
    dirs = torch.randn(d, k, generator=gen)
    dirs = dirs / dirs.norm(dim=1, keepdim=True)
    out = torch.full((d, m), float("nan"), device=DEV)
    ops.swd_project(desc.to(DEV), norm.to(DEV), dirs.to(DEV), out, 7)
    a = (desc - norm[:, 0].repeat_interleave(49)[None]) * norm[:, 1].repeat_interleave(49)[None]  # float32, two roundings
    exact = a.double() @ dirs.double().T
    bound = R.projection_bound(a, dirs)
    err = (out.cpu().double().T - exact).abs()
    print(f"project M {m} D {d} C {c}: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def _patterns(m, gen):
    special = torch.tensor([float("inf"), float("-inf"), 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, 3.4028235e38,
                            -3.4028235e38, 1.0, -1.0])
    rows = [torch.rand(m, generator=gen) * 2 - 1,
            torch.full((m,), 0.375),
            torch.arange(m, dtype=torch.float32) - m / 2,
            m / 2 - torch.arange(m, dtype=torch.float32),
            (torch.rand(m, generator=gen) < 0.5).float() * 7 - 3,
            special[torch.randint(0, len(special), (m,), generator=gen)]]
    rows[5][:min(m, len(special))] = special[:min(m, len(special))]
    return rows


def _sort_case(s, m, shift, gen):
    from musicgan_amd import metrics
    pats = _patterns(m, gen)
    x = torch.stack([pats[(r + shift) % 6][torch.randperm(m, generator=gen)] if (r + shift) % 6 in (1, 4, 5) else pats[(r + shift) % 6]
                     for r in range(s)]).contiguous()
    got = metrics.segmented_sort_(x.to(DEV)).cpu()
    exp = torch.sort(x, dim=1).values
    assert torch.equal(got + 0.0, exp + 0.0), (s, m, shift)   # + 0.0 maps -0.0 to 0.0
    assert int(got.view(torch.int32).long().sum()) == int(x.view(torch.int32).long().sum()), (s, m, shift)  # the multiset is kept


@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 4095, 40961, 2 ** 17 + 11])
@pytest.mark.parametrize("s", [1, 3, 128])
def test_segmented_sort_equals_torch_sort(s, m):
    gen = torch.Generator().manual_seed(14 + s + m)
    for shift in range(0, 6, s if s < 6 else 6):   # every pattern meets every (S, M)
        _sort_case(s, m, shift, gen)


def test_segmented_sort_of_a_million_keys():
    gen = torch.Generator().manual_seed(15)
    _sort_case(4, 2 ** 20, 0, gen)
    _sort_case(4, 2 ** 20, 4, gen)


def _two_sets(n=32, side=128):
    gen = torch.Generator().manual_seed(16)
    return R.smooth_noise(n, 2, side, side, 2, gen), R.smooth_noise(n, 2, side, side, 1, gen)


def _feed(swd, a, b, batch):
    for lo in range(0, a.shape[0], batch):
        swd.feed_real(a[lo:lo + batch].to(DEV).contiguous())
        swd.feed_fake(b[lo:lo + batch].to(DEV).contiguous())
    return swd.result()


def _check_against_helper(got, a, b, draws):
    f64, sets = R.swd(a, b, draws)
    assert list(got) == list(f64)
    bounds = []
    for (name, exp), (da, db), (_, _, dirs) in zip(f64.items(), sets, draws):
        pb = max(float(R.projection_bound(s.float(), dirs.reshape(-1, dirs.shape[2])).max()) for s in (da, db))
        bound = 2 * pb * 1000 + 1e-6 * exp
        print(f"SWD level {name}: gpu {got[name]:.6f} f64 {exp:.6f} err {abs(got[name] - exp):.3e} bound {bound:.3e}")
        assert abs(got[name] - exp) <= bound, (name, got[name], exp, bound)
        bounds.append(bound)
    assert abs(got["avg"] - f64["avg"]) <= sum(bounds) / len(bounds) + 1e-12 * f64["avg"]   # the average of values within bounds
    return f64


def test_swd_end_to_end_matches_the_float64_definition_bit_stable_over_batching():
    from musicgan_amd import metrics
    a, b = _two_sets()
    mk = lambda: metrics.SWD(128, 128, images=32, seed=21)  # noqa: E731
    one = _feed(mk(), a, b, 32)
    assert list(one) == ["128", "64", "32", "16", "avg"]
    f64 = _check_against_helper(one, a, b, mk().draws)
    assert all(v > 1.0 for v in f64.values()), f64   # non-trivial distances
    assert _feed(mk(), a, b, 5) == one               # appending does not change the arithmetic
    assert _feed(mk(), a, b, 32) == one              # nor does running again


def test_sliced_wasserstein_one_repeat_is_symmetric_and_matches():
    from musicgan_amd import metrics
    a, b = _two_sets(8, 64)
    draws = metrics.draw([(64, 64)], 2, 8, 128, 7, 1, 128, seed=22)
    ca, cb, dirs = draws[0]
    da, sa = metrics.patch_descriptors(a.to(DEV), ca.to(DEV))
    db, sb = metrics.patch_descriptors(b.to(DEV), cb.to(DEV))
    ab = metrics.sliced_wasserstein(da, sa, db, sb, dirs[0].to(DEV))
    ba = metrics.sliced_wasserstein(db, sb, da, sa, dirs[0].to(DEV))
    assert ab.dim() == 0 and ab.is_cuda and float(ab) == float(ba)
    na, nb = R.normalise(R.descriptors(a.double(), ca), 2), R.normalise(R.descriptors(b.double(), cb), 2)
    exp = float(R.sliced_distance(na, nb, dirs[0].double()))
    bound = 2 * max(float(R.projection_bound(s.float(), dirs[0]).max()) for s in (na, nb)) + 1e-6 * exp
    print(f"one repeat: gpu {float(ab):.8f} f64 {exp:.8f} err {abs(float(ab) - exp):.3e} bound {bound:.3e}")
    assert abs(float(ab) - exp) <= bound


def test_swd_ranks_a_different_distribution_as_farther():
    from musicgan_amd import metrics
    gen = torch.Generator().manual_seed(17)
    same = R.smooth_noise(64, 2, 64, 64, 2, gen)
    a, a2, b = same[:32], same[32:], R.smooth_noise(32, 2, 64, 64, 1, gen)
    mk = lambda: metrics.SWD(64, 64, images=32, seed=23)  # noqa: E731
    near, far = _feed(mk(), a, a2, 16), _feed(mk(), a, b, 16)
    f_near, f_far = _check_against_helper(near, a, a2, mk().draws), _check_against_helper(far, a, b, mk().draws)
    print(f"finest level: same distribution {near['64']:.4f} (f64 {f_near['64']:.4f}), other {far['64']:.4f} (f64 {f_far['64']:.4f})")
    assert f_near["64"] < f_far["64"] and near["64"] < far["64"]


def test_feeding_does_not_synchronise():
    from musicgan_amd import metrics
    a, b = _two_sets(12, 64)
    a, b = a.to(DEV), b.to(DEV)
    swd = metrics.SWD(64, 64, images=12, seed=24)
    swd.feed_real(a[:4].contiguous())   # warm-up: library load, uploads of the draws, buffers
    swd.feed_fake(b[:4].contiguous())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for lo in (4, 8):
            swd.feed_real(a[lo:lo + 4])
            swd.feed_fake(b[lo:lo + 4])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = swd.result()
    assert all(v == v and v >= 0 for v in out.values())


def test_evaluate_on_a_tiny_corpus(tmp_path, capsys):
    import musicgan_amd
    from musicgan_amd.__main__ import main
    data_dir, ck = tiny_corpus(tmp_path, files=2, seed=5, level=2)      # 2 files x 2 samples
    capsys.readouterr()
    first = musicgan_amd.evaluate(ck, 8, str(data_dir), level=2, nb_images=8, batch_size=3, seed=1)
    text = capsys.readouterr().out
    assert "4 samples" in text and "instead of 8" in text     # -n clipped to the corpus
    assert list(first) == ["16", "avg"]                        # a 16 x 16 image has a one-level pyramid
    assert "[ 16]" in text and "[avg]" in text and "[ 32]" not in text
    assert all(isinstance(v, float) and v == v and 0 <= v < float("inf") for v in first.values())
    js = str(tmp_path / "swd.json")
    main(["evaluate", ck, "8", "-i", str(data_dir), "--level", "2", "-n", "8", "--batch-size", "3", "--seed", "1", "-o", js])
    with open(js) as f:
        assert json.load(f) == first                           # same seed: the identical result, through the CLI
    assert musicgan_amd.evaluate(ck, 8, str(data_dir), level=2, nb_images=8, batch_size=3, seed=1) == first
