"""The float64 yardstick of the perceptual path length in numpy: project.slerp's definition with its weights laid
open, the per-pair values, the percentile trimming of the StyleGAN protocol and every key metrics.PPL reports.  Nothing here touches a
device or the package."""
import math

import numpy as np

U64 = 2.0 ** -53
MIN_ANGLE = 1e-6


def gamma(k: int) -> float:
    return k * U64 / (1.0 - k * U64)


def slerp_weights(a, b, t: float):
    """(w0, w1, antipodal) of project.slerp for the flat vectors a, b at t: the sums, the angle and the sines in float64"""
    a64, b64 = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    na, nb = math.sqrt(float((a64 * a64).sum())), math.sqrt(float((b64 * b64).sum()))
    omega = 0.0
    if na > 0.0 and nb > 0.0:
        omega = math.acos(max(-1.0, min(1.0, float((a64 * b64).sum()) / (na * nb))))
    if math.pi - omega < MIN_ANGLE:
        return 0.0, 0.0, True
    if omega < MIN_ANGLE:
        return 1.0 - t, t, False
    s = math.sin(omega)
    return math.sin((1.0 - t) * omega) / s, math.sin(t * omega) / s, False


def slerp(a, b, t: float):
    """(the point in float64 before its one rounding, |w0 a| + |w1 b| per component, antipodal); zeros for an antipodal pair"""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w0, w1, antipodal = slerp_weights(a64, b64, float(t))
    return w0 * a64 + w1 * b64, np.abs(w0 * a64) + np.abs(w1 * b64), antipodal


def slerp_pairs(z0, z1, t, eps: float):
    """(za, zb float64 (n, d) unrounded, their magnitudes |w0 z0| + |w1 z1|, flag (n,) int) of the rows of z0, z1 at t and t + eps"""
    n = len(z0)
    za, zb = np.zeros(np.shape(z0)), np.zeros(np.shape(z0))
    ma, mb, flag = np.zeros(np.shape(z0)), np.zeros(np.shape(z0)), np.zeros(n, dtype=np.int64)
    for i in range(n):
        ti = float(t[i])
        za[i], ma[i], anti = slerp(z0[i], z1[i], ti)
        zb[i], mb[i], _ = slerp(z0[i], z1[i], ti + eps)
        flag[i] = int(anti)
    return za, zb, ma, mb, flag


def half_ulp32(x):
    """half the spacing of float32 at |x| (float64 array): 2^(e - 24) in the binade 2^e of x, 2^-150 below 2^-126"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(x)
    return np.ldexp(0.5, np.where(x > 0.0, np.maximum(e - 1, -126), -126) - 23)


def slerp_bound(ref, magnitude, d: int):
    """the element-wise bound of the GPU test: half a float32 ulp of the float64 reference plus gamma_{d + 8} (|w0 z0_j| + |w1 z1_j|)"""
    return half_ulp32(ref) + gamma(d + 8) * magnitude


def rows_sqdist(a, b, scale: float):
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return scale * ((a64 - b64) ** 2).sum(1)


def per_pair(rows_a, rows_b, eps: float):
    """d_i = |rows_a[i] - rows_b[i]|^2 / (D eps^2)"""
    return rows_sqdist(rows_a, rows_b, 1.0 / (np.shape(rows_a)[1] * eps * eps))


def trim(values):
    """(lo, hi): numpy's percentiles 1 'lower' and 99 'higher'"""
    v = np.asarray(values, dtype=np.float64)
    return float(np.percentile(v, 1, method="lower")), float(np.percentile(v, 99, method="higher"))


def aggregate(step, flag, chord=None):
    """every key of metrics.PPL.result() from the per-pair values: flagged pairs are left out of every mean"""
    step, keep = np.asarray(step, dtype=np.float64), np.asarray(flag) == 0
    kept = step[keep]
    lo, hi = trim(kept)
    inner = kept[(kept >= lo) & (kept <= hi)]
    result = {"ppl": math.fsum(inner.tolist()) / len(inner), "ppl_mean": math.fsum(kept.tolist()) / len(kept)}
    if chord is not None:
        result["ppl_chord"] = math.fsum(np.asarray(chord, dtype=np.float64)[keep].tolist()) / len(kept)
        result["ppl_ratio"] = result["ppl_mean"] / result["ppl_chord"] if result["ppl_chord"] > 0.0 else float("nan")
    result["ppl_pairs"] = int(keep.sum())
    return result
