"""Times the kernels of precision / recall / density / coverage (csrc/prdc.hip).  The tiled distance launch next to nn_ops.nn_sqdist
(the one-wave-per-chunk path of csrc/nn.hip) on the same operands in the same process, alternating, at 1 024 x 1 024 and 2 048 x
2 048 rows of 32 768 components, with the outputs compared bit for bit at those sizes; the ball-membership scan at 2 048 x 8 192
next to the bytes it reads at 8 TB/s; then the whole metric as `evaluate --metrics prdc` runs it (--images real and as many fake
images of 2 x 128 x 128) next to the generator forwards of an evaluation of that size.  HIP-event timing, warmed up, median and
spread.  The data is synthetic (uniform in [-1, 1]).
   python tools/bench_prdc.py [--images 8192] [--iters 10] [--launches-only] [--out profiles/prdc_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM, MFMA_F32 = 8e12, 157.3e12  # bytes/s, FLOP/s


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def stats(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = events(2 * iters)
    for i in range(iters):
        ev[2 * i].record()
        fn()
        ev[2 * i + 1].record()
    torch.cuda.synchronize()
    return stats([ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters)])


def alternating(fa, fb, iters, warm=2):
    """fa and fb taking turns, so that whatever else the machine does falls on both"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = events(3 * iters)
    for i in range(iters):
        ev[3 * i].record()
        fa()
        ev[3 * i + 1].record()
        fb()
        ev[3 * i + 2].record()
    torch.cuda.synchronize()
    return (stats([ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(iters)]),
            stats([ev[3 * i + 1].elapsed_time(ev[3 * i + 2]) for i in range(iters)]))


def fmt(t):
    return f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--launches-only", action="store_true", help="the per-launch part alone (for a kernel trace)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_prdc needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import metrics, nn_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median "
        f"[min .. max] ms; chunk {nn_ops.nn_chunk()}")
    gen = torch.Generator(device=dev).manual_seed(0)
    d = 2 * 128 * 128
    for n in (1024, 2048):
        q = torch.rand(n, d, device=dev, generator=gen) * 2 - 1
        r = torch.rand(n, d, device=dev, generator=gen) * 2 - 1
        qn, rn = nn_ops.nn_sqnorm(q), nn_ops.nn_sqnorm(r)
        out_t = torch.empty(n, n, dtype=torch.float64, device=dev)
        out_p = torch.empty(n, n, dtype=torch.float64, device=dev)
        macs = n * n * d
        fl = 2 * macs / MFMA_F32 * 1e3
        ws_t, ws_p = nn_ops.nn_tiled_ws_bytes(n, n, d), nn_ops.nn_ws_bytes(n, n, d)
        say(f"--- {n} x {n} rows of {d} components: {macs / 1e9:.1f} G multiply-adds = {fl:.3f} ms at the fp32-MFMA peak; workspace "
            f"tiled {ws_t / 1e6:.0f} MB, per-chunk {ws_p / 1e6:.0f} MB")
        tt, tp = alternating(lambda: nn_ops.nn_sqdist_tiled(q, r, qn, rn, out_t), lambda: nn_ops.nn_sqdist(q, r, qn, rn, out_p), a.iters)
        say("nn_sqdist_tiled (dot + finish)".ljust(34) + fmt(tt) + f"   {fl / tt[0] * 100:.1f} % of the fp32-MFMA peak")
        say("nn_sqdist (dot + dist)".ljust(34) + fmt(tp) + f"   {fl / tp[0] * 100:.1f} % of the fp32-MFMA peak")
        spread = max(tt[2] - tt[1], tp[2] - tp[1])
        verdict = "faster by more than the spread" if tp[0] - tt[0] > spread else "NOT faster by more than the spread"
        say(f"tiled / per-chunk = {tt[0] / tp[0]:.3f}; difference of the medians {tp[0] - tt[0]:.3f} ms, largest spread {spread:.3f} ms: "
            f"tiled is {verdict}; outputs bit-identical: {torch.equal(out_t, out_p)}")
        del q, r, out_t, out_p
        torch.cuda.empty_cache()
    nq, nr = 2048, 8192
    dist = torch.rand(nq, nr, device=dev, generator=gen, dtype=torch.float64)
    radius = torch.rand(nr, device=dev, generator=gen, dtype=torch.float64)
    count = torch.zeros(nq, dtype=torch.int64, device=dev)
    rowmin = torch.full((nq,), float("inf"), dtype=torch.float64, device=dev)
    t = timed(lambda: nn_ops.prdc_scan(dist, radius, count, rowmin), a.iters)
    nbytes = nq * nr * 8 + nr * 8 + nq * 32
    say(f"--- the scan at {nq} x {nr}")
    say("prdc_scan".ljust(34) + fmt(t) + f"   {nbytes / 1e6:8.1f} MB min = {nbytes / HBM * 1e3:.4f} ms at 8 TB/s: {nbytes / HBM * 1e3 / t[0] * 100:.1f} % of it")
    del dist
    if not a.launches_only:
        from musicgan_amd.networks import Generator
        side, bs, n = 128, 16, a.images
        real = torch.rand(n, 2, side, side, device=dev, generator=gen) * 2 - 1
        fake = torch.rand(n, 2, side, side, device=dev, generator=gen) * 2 - 1

        def whole():
            prdc = metrics.PRDC(k=3)
            for lo in range(0, n, bs):
                prdc.feed_real(real[lo:lo + bs])
                prdc.feed_fake(fake[lo:lo + bs])
            return prdc.result()

        say(f"--- the whole metric: {n} real + {n} fake images of 2 x {side} x {side} in batches of {bs}, k = 3: four matrices, "
            f"{4 * 2 * n * n * d / 1e12:.1f} TFLOP = {4 * 2 * n * n * d / MFMA_F32 * 1e3:.1f} ms at the fp32-MFMA peak")
        t = timed(whole, 3, warm=1)
        say("PRDC fed + result".ljust(34) + fmt(t))
        torch.manual_seed(0)
        g = Generator(32, end_layer=5).to(dev).eval()
        lat = torch.randn(n, 32, 2, 2, device=dev, generator=gen)

        def forwards():
            with torch.no_grad():
                for lo in range(0, n, bs):
                    g(lat[lo:lo + bs].contiguous(), 1.0)

        t = timed(forwards, 3, warm=1)
        say(f"generator forwards, {n} images".ljust(34) + fmt(t))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
