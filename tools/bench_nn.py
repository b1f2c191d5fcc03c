"""Times the nearest-neighbour kernels (csrc/nn.hip) at the shape `evaluate --metrics nn` feeds them (256 queries x 16 references of
2 x 128 x 128) and at full size (2 x 512 x 512): the squared norms of a batch, the distance launches (dot + dist) and the merge,
each next to what it has to move at least at 8 TB/s and its multiply-adds at the fp32-MFMA peak.  Then the whole metric as
`evaluate` runs it (2 x 256 queries, --refs references in batches of 16) next to the generator forwards and the SWD of an
evaluation of that size, in the same run.  HIP-event timing, warmed up, median and spread.  As the comparison, never on the product
path: the same definition in torch operators on the device (float32 matmul expansion, topk), with both forms' largest error against
float64 direct differences.  The data is synthetic (uniform in [-1, 1]).
   python tools/bench_nn.py [--refs 8192] [--iters 20] [--launches-only] [--out profiles/nn_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM, MFMA_F32 = 8e12, 157.3e12  # bytes/s, FLOP/s


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


def fmt(t):
    return f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms"


def direct64(q, r):
    return torch.stack([((r.double() - row.double()) ** 2).sum(1) for row in q])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refs", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--launches-only", action="store_true", help="the per-launch part alone (for a kernel trace)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nn needs the GPU: a CPU run says nothing about these kernels"
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
    nq, nr, k = 256, 16, 1
    for d in (2 * 128 * 128, 2 * 512 * 512):
        q = torch.rand(nq, d, device=dev, generator=gen) * 2 - 1
        r = torch.rand(nr, d, device=dev, generator=gen) * 2 - 1
        qn, rn = nn_ops.nn_sqnorm(q), nn_ops.nn_sqnorm(r)
        dist = torch.empty(nq, nr, dtype=torch.float64, device=dev)
        best_d = torch.full((nq, k), nn_ops.EMPTY, dtype=torch.float64, device=dev)
        best_i = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        rid = torch.arange(nr, device=dev)
        part = nn_ops.nn_ws_bytes(nq, nr, d)
        nbytes, macs = (nq + nr) * d * 4 + 2 * part, nq * nr * d
        say(f"--- {nq} queries x {nr} references x {d} components (workspace {part / 1e6:.1f} MB)")
        t = timed(lambda: nn_ops.nn_sqnorm(r, rn), a.iters)
        say(f"nn_sqnorm of the batch".ljust(34) + fmt(t) + f"   {nr * d * 4 / 1e6:8.1f} MB min = {nr * d * 4 / HBM * 1e3:.4f} ms at 8 TB/s")
        t = timed(lambda: nn_ops.nn_sqdist(q, r, qn, rn, dist), a.iters)
        bw, fl = nbytes / HBM * 1e3, 2 * macs / MFMA_F32 * 1e3
        say(f"nn_sqdist (dot + dist launches)".ljust(34) + fmt(t) + f"   {nbytes / 1e6:8.1f} MB min = {bw:.4f} ms at 8 TB/s; {macs / 1e9:.3f} G "
            f"multiply-adds = {fl:.4f} ms at the fp32-MFMA peak; {'HBM' if bw > fl else 'MFMA'} governs: {max(bw, fl) / t[0] * 100:.1f} % of it")
        t = timed(lambda: nn_ops.nn_merge(dist, rid, best_d, best_i), a.iters)
        say(f"nn_merge".ljust(34) + fmt(t))
        if a.launches_only:
            continue
        # the same definition in torch operators, float32
        qn32 = (q * q).sum(1)

        def torch_form():
            d32 = qn32[:, None] + (r * r).sum(1)[None, :] - 2 * (q @ r.T)
            return d32, d32.topk(k, dim=1, largest=False)

        t = timed(torch_form, a.iters)
        say(f"torch: fp32 matmul expansion + topk".ljust(34) + fmt(t) + "   (comparison, not used by the product; the query norms are not timed)")
        d64 = direct64(q, r)
        say(f"largest error against float64 direct differences over the {nq * nr} pairs: ours {float((dist - d64).abs().max()):.3e}, torch "
            f"{float((torch_form()[0].double() - d64).abs().max()):.3e}; distances {float(d64.min()):.1f} .. {float(d64.max()):.1f}")
        del q, r, d64
        torch.cuda.empty_cache()
    if not a.launches_only:
        from musicgan_amd.networks import Generator
        side, bs, n = 128, 16, a.refs
        refs = torch.rand(n, 2, side, side, device=dev, generator=gen) * 2 - 1
        queries = [torch.rand(nq, 2, side, side, device=dev, generator=gen) * 2 - 1 for _ in range(2)]
        ids = [torch.arange(lo, min(lo + bs, n)) for lo in range(0, n, bs)]

        def whole():
            nns = [metrics.NearestNeighbours(x, k=1, query_ids=qi) for x, qi in zip(queries, (None, list(range(nq))))]
            for i, lo in enumerate(range(0, n, bs)):
                for nn in nns:
                    nn.feed(refs[lo:lo + bs], ids[i])
            return [nn.result() for nn in nns]

        say(f"--- the whole metric: 2 x {nq} queries, {n} references of 2 x {side} x {side} in batches of {bs}")
        t = timed(whole, 3, warm=1)
        say(f"NearestNeighbours x 2, fed + result".ljust(34) + fmt(t))
        torch.manual_seed(0)
        g = Generator(32, end_layer=5).to(dev).eval()
        lat = torch.randn(n, 32, 2, 2, device=dev, generator=gen)

        def forwards():
            with torch.no_grad():
                for lo in range(0, n, bs):
                    g(lat[lo:lo + bs].contiguous(), 1.0)

        t = timed(forwards, 3, warm=1)
        say(f"generator forwards, {n} images".ljust(34) + fmt(t))

        def swd():
            s = metrics.SWD(side, side, channels=2, images=n, seed=0)
            with torch.no_grad():
                for lo in range(0, n, bs):
                    s.feed_real(refs[lo:lo + bs])
                    s.feed_fake(g(lat[lo:lo + bs].contiguous(), 1.0).contiguous())
            return s.result()

        t = timed(swd, 2, warm=1)
        say(f"SWD fed (incl. forwards) + result".ljust(34) + fmt(t))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
