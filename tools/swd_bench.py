"""Times the five sliced-Wasserstein kernels (csrc/swd.hip) and a whole SWD.result() at the default evaluation size (8192 + 8192
images of 2 x 512 x 512, 128 patches each: M = 2^20 descriptors of 98 numbers per level and set, 128 directions, 4 repeats, 6
levels).  HIP-event timing, warmed up, median and spread over repeats; next to each kernel the bytes it has to move at least and
the fraction of 8 TB/s that makes.  The kernel rows run on SYNTHETIC data of the real shapes (normal descriptors, one random image
batch); the whole-evaluation row feeds that one random batch of 16 images 512 times per set (the timings do not depend on the
values: the sort is a fixed network).  As context only, never on the product path: torch.sort / torch.matmul on the same arrays,
and the generator's level-7 forward for a batch of 16, which an evaluation runs 512 times.
   python tools/swd_bench.py [--iters 10] [--images 8192] [--out profiles/swd_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM = 8e12  # bytes/s


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
    for i in range(iters):
        ev[2 * i].record()
        fn()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "swd_bench needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import metrics, ops
    from musicgan_amd.networks import Generator
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    mhz = getattr(props, "clock_rate", 0) / 1e3
    say(f"device: {props.name}, {props.multi_processor_count} CUs, " + (f"{mhz:.0f} MHz nominal" if mhz else "clock not reported by the runtime")
        + f"; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    p, pp, c, d, bs = 128, 49, 2, 128, 16
    m, k = a.images * p, c * pp

    def row(name, t, nbytes, note=""):
        med, lo, hi = t
        say(f"{name:<34} {med:9.3f} [{lo:8.3f} .. {hi:8.3f}] ms   {nbytes / 1e6:9.1f} MB min   {nbytes / (med * 1e-3) / HBM * 100:5.1f} % of 8 TB/s  {note}")

    # pyramid + gather on one batch of 16 images, as feed_real / feed_fake see it
    x = torch.randn(bs, c, 512, 512, device=dev, generator=gen)
    npx = x.numel() * 4
    row("pyramid 16x2x512x512, 6 levels", timed(lambda: metrics.laplacian_pyramid(x, 6), a.iters),
        int(npx * (1 + 1 / 4) * 4 / 3 + npx * (1 + 1 / 4 + 1) * 4 / 3), "(down: read G_i write G_i+1; lap: read both write L_i)")
    cen = torch.stack((torch.randint(3, 509, (bs, p), device=dev), torch.randint(3, 509, (bs, p), device=dev)), 2).int()
    buf = (torch.empty(bs * p, k, device=dev), torch.empty(bs, c, 2, dtype=torch.float64, device=dev))
    row("gather 16 x 128 patches @512", timed(lambda: metrics.patch_descriptors(x, cen, out=buf), a.iters), 2 * bs * p * k * 4,
        "(16 workgroups: latency-bound)")

    desc = torch.randn(m, k, device=dev, generator=gen)
    norm = torch.tensor([[0.1, 1.25, 0.8]] * c, device=dev)
    dirs = torch.randn(d, k, device=dev, generator=gen)
    dirs /= dirs.norm(dim=1, keepdim=True)
    proj = torch.empty(2, d, m, device=dev)
    row(f"project M={m} K={k} D={d}", timed(lambda: ops.swd_project(desc, norm, dirs, proj[0], 7), a.iters), (m * k + d * m) * 4,
        f"({2 * m * 100 * d / 1e9:.1f} GFLOP on fp32 MFMA)")
    ops.swd_project(desc, norm, dirs, proj[1], 7)
    keep = proj.clone()

    def sort_once():
        proj.copy_(keep)
        ops.swd_sort_segments_(proj[0])

    t_copy = timed(lambda: proj.copy_(keep), a.iters)
    t_sort = timed(sort_once, a.iters)
    say(f"(refill of the sort input, subtracted below: {t_copy[0]:.3f} ms for both halves)")
    row(f"sort S={d} M={m}", tuple(v - t_copy[0] for v in t_sort), 2 * d * m * 4, "(one read + one write of the keys as the floor)")
    ops.swd_sort_segments_(proj[1])
    out = torch.empty((), device=dev)
    row(f"distance 2 x ({d}, {m})", timed(lambda: ops.swd_distance(proj[0], proj[1], out), a.iters), 2 * d * m * 4)

    say("context (library composition on the same arrays, not used by the product):")
    tmp = torch.empty_like(keep[0])

    def torch_sort():
        torch.sort(keep[0], dim=1, out=(tmp, idx))

    idx = torch.empty(d, m, dtype=torch.long, device=dev)
    row("torch.sort (values + indices)", timed(torch_sort, a.iters), 2 * d * m * 4)
    del idx, tmp
    row("torch.matmul dirs @ desc.T", timed(lambda: torch.matmul(dirs, desc.t()), a.iters), (m * k + d * m) * 4, "(without the normalisation)")
    g7 = Generator(32, end_layer=7).to(dev).eval()
    z = torch.randn(bs, 32, 2, 2, device=dev, generator=gen)
    with torch.no_grad():
        t_gen = timed(lambda: g7(z, 1.0), a.iters)
    say(f"{'generator level 7, batch 16':<34} {t_gen[0]:9.3f} [{t_gen[1]:8.3f} .. {t_gen[2]:8.3f}] ms   x {a.images // bs} batches = "
        f"{t_gen[0] * (a.images // bs) / 1e3:.2f} s per evaluation")
    del desc, proj, keep, g7

    # the whole evaluation: feeding (pyramid + gather of every batch) and result() (6 levels x 4 repeats x project, sort, distance)
    swd = metrics.SWD(512, 512, images=a.images)
    swd.feed_real(x)
    swd.feed_fake(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.images // bs - 1):
        swd.feed_real(x)
        swd.feed_fake(x)
    e1.record()
    torch.cuda.synchronize()
    nb = 2 * (a.images // bs - 1)
    say(f"{'SWD.feed_* (one batch of 16)':<34} {e0.elapsed_time(e1) / nb:9.3f} ms mean over {nb} calls = {e0.elapsed_time(e1) / 1e3:.2f} s per evaluation")
    res = []
    for _ in range(3):
        e0.record()
        swd.result()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1))
    say(f"{'SWD.result() ' + str(a.images) + ' + ' + str(a.images):<34} {sorted(res)[1]:9.1f} [{min(res):8.1f} .. {max(res):8.1f}] ms (3 runs, the first includes "
        f"allocating the projection buffer); {len(swd.sides) * 4 * 2} sorts of ({d}, {m})")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
