"""Times the MS-SSIM kernels (csrc/ssim.hip) for --pairs pairs of 2 x 512 x 512 images (default 4096, what `evaluate --metrics
msssim` computes per set at its default size): one row per scale's launch, the finish, the mean, and the whole
ssim_ops.ms_ssim_into call.  HIP-event timing, warmed up, median and spread over repeats; next to each scale the bytes it has to
move at least (both images read once, the half-size pair written, the slots) and the fraction of 8 TB/s that makes.  The data
is synthetic (uniform noise in [-1, 1], b = (a + other noise) / 2; the timings do not depend on the values).  As the comparison, never on the product path:
the same definition composed from torch operators on the device (grouped conv2d, avg_pool2d), in chunks of --torch-chunk pairs.
   python tools/bench_msssim.py [--pairs 4096] [--iters 10] [--out profiles/msssim_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

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


def torch_ms_ssim(a, b, g, weights):
    """the definition of DESIGN.md in torch operators, float32 per pixel, float64 means"""
    c = a.shape[1]
    gh, gv = g.reshape(1, 1, 1, -1).repeat(c, 1, 1, 1), g.reshape(1, 1, -1, 1).repeat(c, 1, 1, 1)

    def filt(x):
        return F.conv2d(F.conv2d(x, gh, groups=c), gv, groups=c)

    terms = []
    for s in range(len(weights)):
        mua, mub = filt(a), filt(b)
        saa, sbb, sab = filt(a * a) - mua * mua, filt(b * b) - mub * mub, filt(a * b) - mua * mub
        cs = (2 * sab + 0.0036) / (saa + sbb + 0.0036)
        if s == len(weights) - 1:
            cs = cs * ((2 * mua * mub + 0.0004) / (mua * mua + mub * mub + 0.0004))
        terms.append(cs.double().mean((1, 2, 3)))
        if s < len(weights) - 1:
            a, b = F.avg_pool2d(a, 2), F.avg_pool2d(b, 2)
    return (torch.stack(terms, 1).clamp_min(0) ** weights[None]).prod(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-chunk", type=int, default=128)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_msssim needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import ssim_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    mhz = getattr(props, "clock_rate", 0) / 1e3
    say(f"device: {props.name}, {props.multi_processor_count} CUs, " + (f"{mhz:.0f} MHz nominal" if mhz else "clock not reported by the runtime")
        + f"; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    n, c, h, w = a.pairs, 2, 512, 512
    scales = ssim_ops.ssim_scales(h, w)
    gen = torch.Generator(device=dev).manual_seed(0)
    first = torch.rand(n, c, h, w, device=dev, generator=gen) * 2 - 1
    levels = [(first, (first + (torch.rand(n, c, h, w, device=dev, generator=gen) * 2 - 1)) * 0.5)]   # half shared, half independent
    del first
    for s in range(1, scales):
        levels.append(tuple(torch.empty(n, c, h >> s, w >> s, device=dev) for _ in range(2)))
    slots = [torch.empty(n, c, ssim_ops.ssim_tiles(h >> s, w >> s), 2, dtype=torch.float64, device=dev) for s in range(scales)]
    total = 0.0
    for s in range(scales):
        nxt = levels[s + 1] if s + 1 < scales else (None, None)
        t = timed(lambda: ssim_ops.ssim_scale(*levels[s], slots[s], *nxt), a.iters)
        nbytes = 2 * levels[s][0].numel() * 4 + (2 * nxt[0].numel() * 4 if nxt[0] is not None else 0) + slots[s].numel() * 8
        total += t[0]
        say(f"scale {s}: {n} x {c} x {h >> s} x {w >> s}".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms   {nbytes / 1e6:9.1f} MB min   "
            f"{nbytes / (t[0] * 1e-3) / HBM * 100:5.1f} % of 8 TB/s   {slots[s].shape[2]} tiles per plane")
    allslots = torch.cat([x.reshape(-1) for x in slots])
    values = torch.empty(n, dtype=torch.float64, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    t = timed(lambda: ssim_ops.ssim_finish(allslots, n, c, h, w, values), a.iters)
    say("finish (one thread per pair)".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms   {allslots.numel() * 8 / 1e6:9.1f} MB min")
    total += t[0]
    t = timed(lambda: ssim_ops.ssim_mean(values, out), a.iters)
    say("mean of the values".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms")
    say(f"sum of the kernel medians: {total:.3f} ms")
    del levels[1:], slots, allslots
    torch.cuda.empty_cache()
    x, y = levels[0]
    t = timed(lambda: ssim_ops.ms_ssim_into(x, y, values), max(3, a.iters // 2), warm=1)
    say(f"ms_ssim_into, {n} pairs in one call".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms   (allocates its scratch per call)")
    bs = 16
    t = timed(lambda: [ssim_ops.ms_ssim_into(x[lo:lo + bs], y[lo:lo + bs], values, None, lo) for lo in range(0, n, bs)], 3, warm=1)
    say(f"ms_ssim_into, {n // bs} calls of {bs} pairs".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms   (as evaluate feeds it)")
    mine = values.clone()
    say("comparison (library composition on the same images, not used by the product):")
    g = ssim_ops.ssim_window().to(dev)
    wts = torch.tensor((0.0448, 0.2856, 0.3001, 0.2363, 0.1333)[:scales], dtype=torch.float64, device=dev)
    wts = wts / wts.sum()
    ch = min(a.torch_chunk, n)
    ref = torch.empty_like(values)

    def run_torch():
        for lo in range(0, n, ch):
            ref[lo:lo + ch] = torch_ms_ssim(x[lo:lo + ch], y[lo:lo + ch], g, wts)

    t = timed(run_torch, 3, warm=1)
    say(f"torch operators, chunks of {ch} pairs".ljust(38) + f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms")
    say(f"largest difference between the two over the {n} pairs: {float((ref - mine).abs().max()):.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
