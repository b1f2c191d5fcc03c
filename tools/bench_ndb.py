"""Times the k-means behind NDB / JSD (csrc/kmeans.hip, metrics.KMeans): the launches of one Lloyd iteration at the size `evaluate
--metrics ndb` runs by default (4 096 images of 2 x 128 x 128 = 32 768 components, 50 bins), the whole fit of 25 iterations, and the
same Lloyd loop in torch operators on the same device as the yardstick (the expansion |x|^2 + |c|^2 - 2 x c^T through torch.matmul,
argmin, index_add_ and bincount in float32: not the code under test, and neither deterministic nor float64).  For the update the
share of the HBM floor is given: one read of n x D x 4 bytes at 8 TB/s.  HIP-event timing, warmed up, median and spread.  The data is
synthetic: 50 blobs, centres uniform in [-1, 1], noise 0.5 x uniform[-1, 1].
   python tools/bench_ndb.py [--images 4096] [--bins 50] [--iterations 25] [--iters 10] [--out profiles/ndb_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_prdc import alternating, fmt, timed  # noqa: E402  (tools/ is on the path when this file is run)

HBM = 8e12  # bytes/s


def torch_lloyd(x, c0, iterations):
    """the yardstick: (centroids, labels) of the same loop in torch operators, float32"""
    c, xn, k = c0.clone(), (x * x).sum(1), c0.shape[0]
    for t in range(iterations + 1):
        labels = (xn[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T)).argmin(1)
        if t < iterations:
            count = torch.bincount(labels, minlength=k)
            mean = torch.zeros_like(c).index_add_(0, labels, x) / count.clamp_min(1)[:, None]
            c = torch.where(count[:, None] > 0, mean, c)
    return c, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4096)
    ap.add_argument("--bins", type=int, default=50)
    ap.add_argument("--iterations", type=int, default=25)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ndb needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import km_ops, metrics, nn_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median "
        f"[min .. max] ms")
    n, k, d = a.images, a.bins, 2 * 128 * 128
    gen = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand(k, d, device=dev, generator=gen) * 2 - 1
    blob = torch.randint(0, k, (n,), device=dev, generator=gen)
    x = centre[blob] + 0.5 * (torch.rand(n, d, device=dev, generator=gen) * 2 - 1)
    del centre
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:k].tolist()

    def fit():
        km = metrics.KMeans(bins=k, iterations=a.iterations, init_ids=ids)
        km.feed(x)
        return km.fit()

    km = fit()
    c0 = x[ids].clone()
    c_t, labels_t = torch_lloyd(x, c0, a.iterations)
    sizes = km.counts.tolist()
    agree = float((km.labels.long() == labels_t).double().mean())
    say(f"--- {n} rows of {d} components, {k} bins, {a.iterations} iterations: changed {km.changed.tolist()}; bin sizes {min(sizes)} .. "
        f"{max(sizes)}; labels equal to the torch loop's: {100 * agree:.2f} %; largest centroid difference "
        f"{float((km.centroids - c_t).abs().max()):.3e}")
    # one iteration, launch by launch, at the fitted state
    c, labels, xn = km.centroids.clone(), km.labels.clone(), nn_ops.nn_sqnorm(x)
    cn = nn_ops.nn_sqnorm(c)
    dist = nn_ops.nn_sqdist_tiled(x, c, xn, cn)
    mind, changed = torch.empty(n, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    start, order = km_ops.km_order(labels, k)
    macs = n * k * d
    say(f"--- one Lloyd iteration, launch by launch ({macs / 1e9:.1f} G multiply-adds in the distances; the update reads "
        f"{n * d * 4 / 1e6:.0f} MB and writes {km_ops.km_update_ws_bytes(n, d, k) / 1e6:.0f} MB of float64 chunk sums, which it reads back)")
    say("nn_sqnorm (centroids)".ljust(34) + fmt(timed(lambda: nn_ops.nn_sqnorm(c, cn), a.iters)))
    say("nn_sqdist_tiled (dot + finish)".ljust(34) + fmt(timed(lambda: nn_ops.nn_sqdist_tiled(x, c, xn, cn, dist), a.iters)))
    say("km_assign (zero + assign)".ljust(34) + fmt(timed(lambda: km_ops.km_assign(dist, labels, mind, changed), a.iters)))
    say("km_order (hist + place)".ljust(34) + fmt(timed(lambda: km_ops.km_order(labels, k, start, order), a.iters)))
    floor = n * d * 4 / HBM * 1e3
    t = timed(lambda: km_ops.km_update(x, order, start, c), a.iters)
    say("km_update (partial + finish)".ljust(34) + fmt(t) + f"   one read of x = {floor:.4f} ms at 8 TB/s: {floor / t[0] * 100:.1f} % of it")
    say("km_count".ljust(34) + fmt(timed(lambda: km_ops.km_count(labels, torch.zeros(k, dtype=torch.int64, device=dev)), a.iters)))
    # the same steps in torch operators
    lab64, xn32 = labels.long(), xn.float()
    say("--- the same steps in torch operators (float32)")
    say("expansion through torch.matmul".ljust(34) + fmt(timed(lambda: xn32[:, None] + (c * c).sum(1)[None, :] - 2.0 * (x @ c.T), a.iters)))
    d32 = dist.float()
    say("argmin".ljust(34) + fmt(timed(lambda: d32.argmin(1), a.iters)))
    tt = timed(lambda: torch.zeros_like(c).index_add_(0, lab64, x), a.iters)
    say("index_add_".ljust(34) + fmt(tt) + f"   {floor / tt[0] * 100:.1f} % of the same floor")
    verdict = "km_update is faster" if t[0] < tt[0] else "km_update LOSES to index_add_"
    say(f"km_update / index_add_ = {t[0] / tt[0]:.3f}: {verdict} (float64 in a fixed order against float32 atomics)")
    # the whole fit, alternating with the yardstick
    reps = max(3, a.iters // 3)
    ours, theirs = alternating(fit, lambda: torch_lloyd(x, c0, a.iterations), reps, warm=1)
    say(f"--- the whole fit ({a.iterations} iterations and the final assignment, feeding included), alternating, {reps} repeats")
    say("KMeans.feed + fit".ljust(34) + fmt(ours))
    say("torch loop".ljust(34) + fmt(theirs))
    spread = max(ours[2] - ours[1], theirs[2] - theirs[1])
    say(f"KMeans / torch loop = {ours[0] / theirs[0]:.3f}; difference of the medians {theirs[0] - ours[0]:.3f} ms, largest spread {spread:.3f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
