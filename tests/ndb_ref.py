"""The float64 restatement of the k-means of musicgan_amd.metrics.KMeans and of the NDB / JSD statistics, built on
tests/nn_ref.py, with the bound of the centroid update and the cases the tests share.  Nothing here needs a GPU.

k-means.  Distances by direct differences in float64 (nn_ref.sqdist: the yardstick, not the expansion the GPU evaluates); a point
goes to the column of its smallest distance, ties to the smaller column; a centroid is the mean of its members, rounded once to
float32; a bin without members keeps its centroid; T rounds of assignment and update, then one final assignment.

What the GPU's update may differ by, for one component of a bin with members x_1 .. x_m (float32, exact in float64).  The GPU
adds them in float64 in a fixed order (chunks of members, then the chunk sums): a recursive sum of m terms in ANY order has m - 1
additions, each with one rounding of relative size u = 2^-53, so (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.,
eq. 4.4, first order as in nn_ref.py)

    |fl(sum x_i) - sum x_i|  <=  (m - 1) u sum |x_i|.

The division by m is one more rounding of a value of size at most sum |x_i| / m, and so is the one rounding the yardstick itself
makes (it adds the members with an error-free transformation -- Knuth's TwoSum, the rounding errors kept in a second float64 --
and rounds when it forms the quotient): (m - 1) + 1 + 1 = m + 1 roundings of size u sum |x_i| / m in all.  The result is rounded
once to float32: relative size 2^-24 for a normal number, half the smallest subnormal, 2^-150 <= 2^-149, below that.  Hence

    |got - mean|  <=  2^-24 |mean| + (m + 1) 2^-53 sum |x_i| / m + 2^-149.

NDB / JSD.  With reference counts a (sum n_a) and query counts b (sum n_b) over the same K bins: P = a_j / n_a, Q = b_j / n_b,
p = (a_j + b_j) / (n_a + n_b), se = sqrt(p (1 - p) (1 / n_a + 1 / n_b)), z = (P - Q) / se (0 when se = 0); a bin is different when
|z| > 1.959963984540054; ndb = different bins / K; jsd = KL(P | M) / 2 + KL(Q | M) / 2, M = (P + Q) / 2, natural logarithm, terms
with a zero numerator 0."""
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref as R  # noqa: E402

Z = 1.959963984540054
KEYS = ("ndb", "jsd")
# (reference counts, query counts, different bins, ndb, jsd): checked by hand (z of the first: -+2.8867513459; the largest |z| of the
# third is 1.129 and its empty bin has se = 0)
HAND = [((50, 50), (70, 30), 2, 1.0, 0.0210059257),
        ((40, 30, 20, 10), (40, 30, 20, 10), 0, 0.0, 0.0),
        ((40, 30, 20, 10, 0), (38, 33, 14, 15, 0), 0, 0.0, 0.0056634083),
        ((25, 25, 25, 25), (100, 0, 0, 0), 4, 1.0, 0.3803956658)]
# planted blobs (n, d, k, T): odd d, so element-wise loads; bins of 42 - 43 members, and with labels % 2 two of 171 and 129 that
# cross any member chunk; the row length of `evaluate`
PLANTED = [(37, 231, 5, 4), (300, 1024, 7, 4), (64, 32768, 3, 3)]
PLANTED_IDS = ["x".join(map(str, c)) for c in PLANTED]
# uniform data (n, d, k) against k of its own rows: no structure, so near ties exist
GENERAL = [(96, 231, 6), (256, 1024, 16)]
GENERAL_IDS = ["x".join(map(str, c)) for c in GENERAL]
MARGIN, UNDECIDED_CAP = 100.0, 0.01   # conditions the cases must meet by the reference alone (test_ndb_cpu.py), not measurements


# ------------------------------------------------------------------ statistics
def statistics(a, b):
    """{"ndb", "jsd", "different", "z"} from two integer count vectors, as the text above defines them"""
    n_a, n_b, z, jsd = sum(a), sum(b), [], 0.0
    for a_j, b_j in zip(a, b):
        big_p, big_q, p = a_j / n_a, b_j / n_b, (a_j + b_j) / (n_a + n_b)
        se = math.sqrt(p * (1 - p) * (1 / n_a + 1 / n_b))
        z.append((big_p - big_q) / se if se > 0 else 0.0)
        m = (big_p + big_q) / 2
        jsd += (big_p * math.log(big_p / m) if big_p > 0 else 0.0) / 2 + (big_q * math.log(big_q / m) if big_q > 0 else 0.0) / 2
    different = sum(abs(v) > Z for v in z)
    return {"ndb": different / len(a), "jsd": jsd, "different": different, "z": z}


# ------------------------------------------------------------------ k-means
def argmin_first(d: torch.Tensor) -> torch.Tensor:
    """the column of every row's smallest entry, ties to the smaller column (argmax returns the first of several maxima)"""
    return (d == d.min(1, keepdim=True).values).to(torch.int8).argmax(1)


def mean_exact(rows: torch.Tensor) -> torch.Tensor:
    """(d,) float64: the mean of the float32 rows (m, d), summed in ascending order with TwoSum, one rounding at the quotient"""
    s = torch.zeros(rows.shape[1], dtype=torch.float64)
    e = torch.zeros_like(s)
    for v in rows.double():
        t = s + v
        z = t - s
        e += (s - (t - z)) + (v - z)
        s = t
    return (s + e) / rows.shape[0]


def means(x: torch.Tensor, labels: torch.Tensor, c: torch.Tensor):
    """(float64 means (k, d), per-component bound (k, d), member counts): the rows of bins without members are c's and bound 0"""
    k = c.shape[0]
    mean, bnd, count = c.double().clone(), torch.zeros(c.shape, dtype=torch.float64), []
    for j in range(k):
        rows = x[labels == j]
        m = rows.shape[0]
        count.append(m)
        if m:
            mean[j] = mean_exact(rows)
            bnd[j] = R.U32 * mean[j].abs() + (m + 1) * R.U64 * rows.double().abs().sum(0) / m + 2.0 ** -149
    return mean, bnd, count


def kmeans(x: torch.Tensor, init_ids, iterations: int):
    """the definition: (centroids (k, d) float32, labels (n,) int64, changed [iterations + 1], per assignment (d64, centroids))"""
    c = x[list(init_ids)].clone()
    labels = torch.full((x.shape[0],), -1, dtype=torch.int64)
    changed, steps = [], []
    for t in range(iterations + 1):
        d64 = R.sqdist(x, c)
        new = argmin_first(d64)
        changed.append(int((new != labels).sum()))
        labels = new
        steps.append((d64, c.clone()))
        if t < iterations:
            c = means(x, labels, c)[0].float()
    return c, labels, changed, steps


def ratios(x: torch.Tensor, c: torch.Tensor, d64: torch.Tensor, chunk: int) -> torch.Tensor:
    """(n, k) float64: (d_ij - d_i,best) / (bound_ij + bound_i,best), infinite at j = best: a GPU whose distances are within
    nn_ref.bound can prefer column j to the float64 choice only where this is <= 1"""
    b = R.bound(x, c, chunk)
    best = argmin_first(d64)[:, None]
    out = (d64 - d64.gather(1, best)) / (b + b.gather(1, best))
    return out.scatter(1, best, float("inf"))


def planted_inputs(n: int, d: int, k: int, seed=None, sigma: float = 0.25):
    """(x (n, d) float32, truth (n,) int64): k centres uniform in [-1, 1], point i = centre i % k + sigma * uniform[-1, 1]; one
    generator, the centres first.  The initial centroids of the tests are the rows 0 .. k-1: one point of every blob."""
    gen = torch.Generator().manual_seed(70 + n if seed is None else seed)
    centre = torch.rand(k, d, generator=gen) * 2 - 1
    truth = torch.arange(n) % k
    return centre[truth] + sigma * (torch.rand(n, d, generator=gen) * 2 - 1), truth


@functools.lru_cache(maxsize=None)
def planted(index: int, chunk: int):
    """the shared planted case PLANTED[index], computed once per process; callers leave the tensors unchanged.  `margin`: the
    smallest of `ratios` over every point, other column and assignment."""
    n, d, k, iters = PLANTED[index]
    x, truth = planted_inputs(n, d, k)
    c, labels, changed, steps = kmeans(x, range(k), iters)
    margin = min(float(ratios(x, cs, d64, chunk).min()) for d64, cs in steps)
    mean, bnd, count = means(x, truth, c)
    return dict(x=x, truth=truth, k=k, iterations=iters, init_ids=list(range(k)), centroids=c, labels=labels, changed=changed,
                margin=margin, mean=mean, bound=bnd, count=count)


@functools.lru_cache(maxsize=None)
def general(index: int, chunk: int):
    """the shared general case GENERAL[index]: x uniform in [-1, 1] (seed 5), the centroids its rows randperm(n)[:k] from the same
    generator; the float64 distances, labels and `ratios`, and the share of points with some other column at ratio <= 1 (the
    points whose label the GPU may choose differently: 0 of 96 and 1 of 256 = 0.39 %)"""
    n, d, k = GENERAL[index]
    gen = torch.Generator().manual_seed(5)
    x = torch.rand(n, d, generator=gen) * 2 - 1
    ids = torch.randperm(n, generator=gen)[:k].tolist()
    c = x[ids].clone()
    d64 = R.sqdist(x, c)
    ratio = ratios(x, c, d64, chunk)
    return dict(x=x, c=c, k=k, init_ids=ids, d64=d64, labels=argmin_first(d64), bound=R.bound(x, c, chunk), ratio=ratio,
                undecided=int((ratio <= 1.0).any(1).sum()) / n)
