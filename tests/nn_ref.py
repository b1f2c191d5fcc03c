"""The float64 definition of the nearest-neighbour search of musicgan_amd.metrics ("Evaluation: nearest training
neighbours"), the derived error bound of the GPU evaluation, and the inputs the tests use.  Nothing here needs a GPU.

    d(q, r) = sum_d (q_d - r_d)^2                       direct differences in float64: the yardstick, not the expansion

The GPU evaluates  max(0, |q|^2 + |r|^2 - 2 q.r).  Its only float32 arithmetic is the dot product inside a chunk of c consecutive
components: a chain of c fused multiply-adds starting from zero, one rounding of relative size u = 2^-24 each, in an order that is
fixed.  For ANY order of a recursive sum of c terms (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4 with
the product folded into the first rounding of each fma)

    |fl(sum_chunk q_d r_d) - sum_chunk q_d r_d|  <=  gamma_c sum_chunk |q_d r_d|,     gamma_c = c u / (1 - c u).

The float32 partial sums are stored as they are and added in float64 (at most ceil(D / c) additions), the squared norms are sums
of D exact float64 products, and the three terms are combined in float64: each of these steps is a float64 sum of at most D + 16
terms, so all of them together stay below (D + 16) 2^-53 times the sum of the absolute values.  Hence

    |d_gpu - d|  <=  gamma (|q|^2 + |r|^2 + 2 sum_d |q_d r_d|),     gamma = gamma_c + (D + 16) 2^-53,

and the clamp at 0 only moves a value towards d >= 0.  With c = 256, gamma = 1.53e-5."""
import torch

U32, U64 = 2.0 ** -24, 2.0 ** -53
NOISE = (0.3, 0.03, 0.003, 0.0)


def gamma(d: int, chunk: int) -> float:
    return chunk * U32 / (1.0 - chunk * U32) + (d + 16) * U64


def flat(x: torch.Tensor) -> torch.Tensor:
    return x.reshape(x.shape[0], -1)


def sqdist(q: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """(Q, M) float64: the definition, by direct differences"""
    q, r = flat(q).double(), flat(r).double()
    return torch.stack([((r - row) ** 2).sum(1) for row in q])


def expansion(q: torch.Tensor, r: torch.Tensor, dtype=torch.float64) -> torch.Tensor:
    """|q|^2 + |r|^2 - 2 q.r evaluated in `dtype` with torch's own operators on the CPU"""
    q, r = flat(q).to(dtype), flat(r).to(dtype)
    return ((q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] - 2 * (q @ r.T)).double()


def bound(q: torch.Tensor, r: torch.Tensor, chunk: int) -> torch.Tensor:
    """(Q, M) float64: the derived bound of every pair"""
    q, r = flat(q).double(), flat(r).double()
    return gamma(q.shape[1], chunk) * ((q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] + 2 * (q.abs() @ r.abs().T))


def inputs(nq: int, nr: int, shape, seed: int):
    """references (nr, *shape) uniform in [-1, 1]; queries (nq, *shape): the first nq // 2 are planted, query i = reference j_i +
    a_i noise with distinct j_i, a_i = NOISE[i % 4] and noise uniform in [-1, 1]; the others are unrelated uniform images.
    Returns (queries, references, [(i, j_i, a_i)]), float32."""
    gen = torch.Generator().manual_seed(seed)
    r = torch.rand(nr, *shape, generator=gen) * 2 - 1
    q = torch.rand(nq, *shape, generator=gen) * 2 - 1
    js = torch.randperm(nr, generator=gen)[:nq // 2].tolist()
    planted = []
    for i, j in enumerate(js):
        a = NOISE[i % len(NOISE)]
        q[i] = r[j] + a * (torch.rand(*shape, generator=gen) * 2 - 1) if a else r[j]
        planted.append((i, j, a))
    return q, r, planted


def ranking(d64: torch.Tensor, ids=None, query_ids=None):
    """the float64 neighbours: (sorted distances (Q, M'), their ids), ascending by (distance, id); a reference whose id is the
    query's own goes last with an infinite distance"""
    m = d64.shape[1]
    ids = torch.arange(m) if ids is None else torch.as_tensor(ids)
    order = torch.argsort(ids, stable=True)
    d, ids = d64[:, order].clone(), ids[order]
    if query_ids is not None:
        d[torch.as_tensor(query_ids)[:, None] == ids[None, :]] = float("inf")
    val, pos = torch.sort(d, dim=1, stable=True)   # stable on columns already ordered by id: ties go to the smaller id
    return val, ids[pos]
