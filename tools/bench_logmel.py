"""Times the kernels of the log-mel feature space (csrc/logmel.hip, csrc/moments.hip) through musicgan_amd.mel_ops: logmel_rows at
(16, 2, 512, 512) and (64, 2, 512, 512) with evaluate_mel's two row shapes (64 bands x 32 pools for nn / prdc / ndb, 64 x 8 for fd), and
moments at 8192 x 512 (fd's default size).  Each next to the same definition in torch operators on the same device, alternating (a
dense float32 matmul with the zero-padded filterbank, float64 logarithm and mean; float64 centring and matmul: not the code under
test), with the largest difference between the two, and next to the bytes the launch has to move at 8 TB/s: one read of the
magnitude plane and one write of the rows; one read of the rows per pass plus the float64 partial sums written and read back.
Every timed window holds --calls calls between two HIP events (one call is a few microseconds of kernel: a window of one would
measure the launch); warmed up, median and spread of --iters windows, per call.  The data is synthetic (uniform in [-1.2, 1.2]).
   python tools/bench_logmel.py [--iters 10] [--calls 20] [--out profiles/logmel_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_prdc import alternating, fmt  # noqa: E402  (tools/ is on the path when this file is run)

HBM = 8e12  # bytes/s


def torch_logmel(x, scale, dense, floor, pools):
    """the yardstick: the definition in torch operators (the filterbank as a dense (M, H) matrix with zeros outside the bands)"""
    t = x[:, 0] * scale[None, :, None] + scale[None, :, None]
    s = torch.matmul(dense, t * t)
    v = torch.log(s.double() + floor)
    n, m, w = v.shape
    return v.view(n, m, pools, w // pools).mean(3).float().view(n, m * pools)


def torch_moments(x):
    x = x.double()
    mean = x.mean(0)
    c = x - mean
    return mean, c.T @ c / (x.shape[0] - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_logmel needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import mel_ops, metrics
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def per_call(fn):
        def window():
            for _ in range(a.calls):
                fn()
        return window

    def both(ours, theirs):
        """(ours, theirs) per call, from alternating windows of a.calls calls"""
        to, tt = alternating(per_call(ours), per_call(theirs), a.iters)
        return tuple(v / a.calls for v in to), tuple(v / a.calls for v in tt)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events around {a.calls} calls, {a.iters} windows alternating with the "
        f"torch form after 2 warm-up windows: per call, median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    for n in (16, 64):
        x = torch.rand(n, 2, 512, 512, device=dev, generator=gen) * 2.4 - 1.2
        for pools in (32, 8):
            lm = metrics.LogMel(512, 512, pools=pools)
            scale, weight = lm.scale.to(dev), lm.weight.to(dev)
            out = torch.empty(n, lm.dims, device=dev)
            ours = lambda: mel_ops.logmel_rows(x, 0, scale, weight, lm.lo, lm.hi, lm.floor, pools, out)  # noqa: E731
            theirs = lambda: torch_logmel(x, scale, weight, lm.floor, pools)  # noqa: E731
            diff = float((ours() - theirs()).abs().max())
            to, tt = both(ours, theirs)
            nbytes = n * 512 * 512 * 4 + n * lm.dims * 4
            floor_ms = nbytes / HBM * 1e3
            say(f"--- logmel_rows ({n}, 2, 512, 512) -> ({n}, 64 x {pools}): {nbytes / 1e6:.1f} MB = {floor_ms:.4f} ms at 8 TB/s; largest "
                f"difference to the torch form {diff:.2e}")
            say("mel_ops.logmel_rows".ljust(34) + fmt(to) + f"   {floor_ms / to[0] * 100:.1f} % of the byte floor")
            say("torch (matmul, log, mean)".ljust(34) + fmt(tt) + f"   logmel_rows / torch = {to[0] / tt[0]:.3f}")
    n, d = 8192, 512
    rows = torch.randn(n, d, device=dev, generator=gen) - 3.0
    mean = torch.empty(d, dtype=torch.float64, device=dev)
    cov = torch.empty(d, d, dtype=torch.float64, device=dev)
    ours = lambda: mel_ops.moments(rows, mean, cov)  # noqa: E731
    theirs = lambda: torch_moments(rows)  # noqa: E731
    want = theirs()
    ours()
    diff = max(float((mean - want[0]).abs().max()), float((cov - want[1]).abs().max()))
    ws = mel_ops.moments_ws_bytes(n, d)
    nbytes = 2 * n * d * 4 + 2 * ws + d * d * 8
    floor_ms = nbytes / HBM * 1e3
    to, tt = both(ours, theirs)
    say(f"--- moments {n} x {d}: {n * d * d / 1e9:.1f} G float64 multiply-adds; two reads of the rows, {ws / 1e6:.1f} MB of partial "
        f"sums written and read, the matrix written = {nbytes / 1e6:.1f} MB = {floor_ms:.4f} ms at 8 TB/s; largest difference to the torch "
        f"form {diff:.2e}")
    say("mel_ops.moments (4 launches)".ljust(34) + fmt(to) + f"   {floor_ms / to[0] * 100:.1f} % of the byte floor")
    say("torch (float64 centring, matmul)".ljust(34) + fmt(tt) + f"   moments / torch = {to[0] / tt[0]:.3f}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
