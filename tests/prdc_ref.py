"""The float64 definition of precision / recall / density / coverage (musicgan_amd.metrics.PRDC) by direct
differences, built on tests/nn_ref.py, with the intervals the GPU's numbers must lie in.  Nothing here needs a GPU.

On squared distances d, with radius(x) = d(x, the k-th nearest OTHER member of x's own set) (leave-one-out by position):

    count_fake_i = #{ j : d(fake_i, real_j) <= radius(real_j) }          precision = mean_i [count_fake_i > 0]
    count_real_j = #{ i : d(real_j, fake_i) <= radius(fake_i) }          recall    = mean_j [count_real_j > 0]
    nearest_fake_j = min_i d(real_j, fake_i)                             density   = sum_i count_fake_i / (k n_fake)
                                                                         coverage  = mean_j [nearest_fake_j <= radius(real_j)]

What the GPU may differ by.  Every GPU distance lies within nn_ref.bound of its float64 value.  A k-th order statistic and a
minimum of values that each move by at most e move by at most e, so radius(x_j) is off by at most rb_j = max_i' bound(x_j, x_i')
over its own set, and nearest_fake_j by at most nb_j = max_i bound(real_j, fake_i).  A comparison d_ij <= radius_j is therefore
decided whenever |d_ij - radius_j| > m_ij = bound_ij + rb_j: surely true when d_ij + m_ij <= radius_j (the "- m" side: the
smallest count), surely false when d_ij - m_ij > radius_j (the "+ m" side counts everything not surely false).  Each of the four
numbers is monotone in those comparisons, so it lies between its value on the two sides."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402

KEYS = ("precision", "recall", "density", "coverage")
# (n_real, n_fake, shape, k): a square case, odd sizes with a D that is no multiple of 4, 128 chunks with ragged tiles, k = MAX_K
CASES = [(64, 64, (2, 32, 32), 3), (40, 56, (3, 7, 11), 2), (128, 96, (2, 128, 128), 5), (48, 48, (2, 16, 16), 16)]
IDS = ["x".join(map(str, (a, b) + s + (k,))) for a, b, s, k in CASES]
PAIR_CAP, WIDTH_CAP = 0.005, 0.05    # the share of undecided pairs and the widest interval the cases may show (test_prdc_cpu.py)


def inputs(n_real: int, n_fake: int, shape, seed: int):
    """8 cluster centres; reals around all of them; fakes around 4 of them at the data's spread, tighter, wider, and as near copies
    of real images: precision and recall both strictly inside (0, 1).  One generator, drawn in the order of this text."""
    gen = torch.Generator().manual_seed(seed)

    def u():
        return torch.rand(*shape, generator=gen) * 2 - 1

    centre = [u() for _ in range(8)]
    real = [centre[i % 8] + 0.5 * u() for i in range(n_real)]
    fake = []
    for i in range(n_fake):
        m = (i // 4) % 4
        if i % 4 == 3:
            fake.append(real[(7 * i) % n_real] + 0.05 * u())
        else:
            fake.append(centre[m] + (0.5, 0.25, 1.0)[i % 4] * u())
    return torch.stack(real), torch.stack(fake)


def radius(d_own: torch.Tensor, k: int) -> torch.Tensor:
    """the k-th smallest of every row of a set's own (n, n) distance matrix, the diagonal left out"""
    d = d_own.clone()
    d.fill_diagonal_(float("inf"))
    return torch.sort(d, dim=1).values[:, k - 1]


def numbers(count_fake, count_real, covered, k: int):
    """integer counts over integer divisors, divided once each"""
    n_fake, n_real = count_fake.shape[0], count_real.shape[0]
    return {"precision": int((count_fake > 0).sum()) / n_fake, "recall": int((count_real > 0).sum()) / n_real,
            "density": int(count_fake.sum()) / (k * n_fake), "coverage": int(covered.sum()) / n_real}


def prdc(real: torch.Tensor, fake: torch.Tensor, k: int):
    """the definition: (the four numbers, the per-sample tensors named as metrics.PRDC.per_sample names them)"""
    d_rf = R.sqdist(real, fake)                       # (n_real, n_fake)
    rad_r, rad_f = radius(R.sqdist(real, real), k), radius(R.sqdist(fake, fake), k)
    per = dict(radius_real=rad_r, radius_fake=rad_f, count_fake=(d_rf.T <= rad_r[None, :]).sum(1),
               count_real=(d_rf <= rad_f[None, :]).sum(1), nearest_fake=d_rf.min(1).values)
    return numbers(per["count_fake"], per["count_real"], per["nearest_fake"] <= rad_r, k), per


def intervals(real: torch.Tensor, fake: torch.Tensor, k: int, chunk: int):
    """everything test_prdc_gpu.py compares with: the definition's values (`per`, `exact`), the bounds of the radii and of the
    nearest-fake distance (`rb_real`, `rb_fake`, `nb`), the per-sample counts on both sides (`*_lo` surely inside, `*_hi` not
    surely outside), the four numbers on both sides (`lo`, `hi`) and the share of undecided pairs (`unsure`)."""
    exact, per = prdc(real, fake, k)
    d_rf, b_rf = R.sqdist(real, fake), R.bound(real, fake, chunk)
    rb_real, rb_fake = R.bound(real, real, chunk).max(1).values, R.bound(fake, fake, chunk).max(1).values
    nb = b_rf.max(1).values
    rad_r, rad_f = per["radius_real"], per["radius_fake"]
    m_fr = b_rf.T + rb_real[None, :]                  # fake rows against real balls
    m_rf = b_rf + rb_fake[None, :]                    # real rows against fake balls
    out = dict(exact=exact, per=per, rb_real=rb_real, rb_fake=rb_fake, nb=nb)
    out["count_fake_lo"], out["count_fake_hi"] = (d_rf.T + m_fr <= rad_r[None, :]).sum(1), (d_rf.T - m_fr <= rad_r[None, :]).sum(1)
    out["count_real_lo"], out["count_real_hi"] = (d_rf + m_rf <= rad_f[None, :]).sum(1), (d_rf - m_rf <= rad_f[None, :]).sum(1)
    out["covered_lo"] = per["nearest_fake"] + nb + rb_real <= rad_r
    out["covered_hi"] = per["nearest_fake"] - nb - rb_real <= rad_r
    out["lo"] = numbers(out["count_fake_lo"], out["count_real_lo"], out["covered_lo"], k)
    out["hi"] = numbers(out["count_fake_hi"], out["count_real_hi"], out["covered_hi"], k)
    undecided = int(((d_rf.T - rad_r[None, :]).abs() <= m_fr).sum()) + int(((d_rf - rad_f[None, :]).abs() <= m_rf).sum())
    out["unsure"] = undecided / (2 * d_rf.numel())
    return out


@functools.lru_cache(maxsize=None)
def case(index: int, chunk: int):
    """(real, fake, k, intervals) of CASES[index], computed once per process and shared; callers leave the tensors unchanged"""
    n_real, n_fake, shape, k = CASES[index]
    real, fake = inputs(n_real, n_fake, shape, 90 + n_real)
    return real, fake, k, intervals(real, fake, k, chunk)
