"""NumPy restatement of the multi-scale L2 loss, the reference of tests/test_project_cpu.py and
tests/test_project_gpu.py.  The pyramid d_s is float32 with the kernel's own expression, so it is reproduced bit for bit; the loss and
the gradient g64 are float64 from those d_s.  The planner's constants are restated from musicgan_amd/csrc/pyrloss_plan.h."""
import math

import numpy as np

MAX_LEVELS = 7
TILE = 64
THREADS = 256
RED = 32
LDS_LIMIT = 160 * 1024   # one CU's LDS, which a single workgroup may declare in full

# the kernel shapes (N, C, H, W, L) of the issue
SHAPES = [(1, 1, 1, 1, 1), (5, 1, 2, 6, 2), (2, 2, 8, 8, 4), (1, 2, 96, 32, 6), (3, 2, 64, 64, 7), (2, 2, 128, 192, 7),
          (1, 2, 512, 512, 7)]


def default_weights(levels: int):
    return (1.0 / levels,) * levels


def pyramid(x: np.ndarray, t: np.ndarray, levels: int):
    """[d_0 .. d_{L-1}] float32: d_0 = x - t, d_{s+1} = ((a + b) + (c + d)) * 0.25f over the 2 x 2 blocks"""
    assert x.dtype == np.float32 and t.dtype == np.float32
    d = [x - t]
    q = np.float32(0.25)
    for _ in range(levels - 1):
        p = d[-1]
        d.append(((p[..., 0::2, 0::2] + p[..., 0::2, 1::2]) + (p[..., 1::2, 0::2] + p[..., 1::2, 1::2])) * q)
        assert d[-1].dtype == np.float32
    return d


def loss(d, weights):
    """(N,) float64: sum_s (double)(float)lambda_s / (C H_s W_s) * S_s, S_s the exactly rounded sum of the squares of d_s"""
    n = d[0].shape[0]
    out = np.zeros(n, dtype=np.float64)
    for i in range(n):
        acc = 0.0
        for s, lam in enumerate(weights):
            v = d[s][i].astype(np.float64).reshape(-1)
            acc += float(np.float32(lam)) / float(v.size) * math.fsum((v * v).tolist())
        out[i] = acc
    return out


def terms(shape, levels: int) -> int:
    """squares summed per sample: T of the loss bound"""
    _, c, h, w = shape
    return sum(c * (h >> s) * (w >> s) for s in range(levels))


def up(a: np.ndarray, s: int) -> np.ndarray:
    """level s brought back to the full grid: a[i >> s, j >> s]"""
    return a.repeat(1 << s, axis=-2).repeat(1 << s, axis=-1) if s else a


def grad64(d, weights):
    """float64 gradient (2 / (C H W)) sum_s lambda_s d_s[i >> s, j >> s] and the bound's scale k sum_s lambda_s |d_s|"""
    _, c, h, w = d[0].shape
    k = 2.0 / (c * h * w)
    g = np.zeros(d[0].shape, dtype=np.float64)
    mag = np.zeros(d[0].shape, dtype=np.float64)
    for s, lam in enumerate(weights):
        lam = float(np.float32(lam))
        g += lam * up(d[s].astype(np.float64), s)
        mag += lam * np.abs(up(d[s].astype(np.float64), s))
    return g * k, mag * k


def gamma(n: int) -> float:
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def inputs(shape, seed: int):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape, dtype=np.float32), rng.standard_normal(shape, dtype=np.float32)


# ------------------------------------------------------------------ the planner, restated
def plan(n: int, c: int, h: int, w: int, levels: int):
    """what pyr_plan returns, as a dict; None where it refuses"""
    if min(n, c, h, w) < 1 or not 1 <= levels <= MAX_LEVELS:
        return None
    g = 1 << (levels - 1)
    if h % g or w % g:
        return None
    ty, tx = -(-h // TILE), -(-w // TILE)
    per_sample = c * ty * tx
    if per_sample * n >= 1 << 31:
        return None
    pyr = sum((TILE >> s) ** 2 for s in range(1, levels))
    pyr += pyr & 1
    return {"tile_h": min(h, TILE), "tile_w": min(w, TILE), "tiles_y": ty, "tiles_x": tx, "tiles_per_sample": per_sample,
            "grid": per_sample * n, "elems": n * c * h * w, "lds_bytes": pyr * 4 + levels * (THREADS + RED) * 8,
            "ws_bytes": per_sample * n * levels * 8}
