"""Times the kernels of the kernel distance (csrc/kid.hip) through musicgan_amd.kid_ops: polyk_rowsums at 100 subsets x 1000 x 1000 x
512 (the published KID protocol on evaluate_mel's rows: the lists are gathered by the kernel) and at 8192 x 8192 x 512 (kid_full at the
default set size), with and without the skipped diagonal, and standardise_rows at 8192 x 512.  Each next to the same definition in
torch operators on the same device, alternating (float32 `matmul`, cube and `sum`, with the gather as an indexing operation first: not
the code under test; it stores every kernel matrix, rounds the whole dot product in float32 and adds in an order that is not
fixed), with the largest relative difference between the two, and next to the fp32-MFMA peak and the bytes the launch has to move at
8 TB/s.  Then the whole metrics.KID.result() at 8192 + 8192 rows.  The data is synthetic (standard normal rows).
   python tools/bench_kid.py [--iters 10] [--out profiles/kid_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_prdc import alternating, fmt  # noqa: E402  (tools/ is on the path when this file is run)

HBM = 8e12          # bytes/s
PEAK_F32 = 157.3e12  # fp32 matrix FLOP/s of the MI355X (256 CUs x 256 FLOP/clock x 2.4 GHz)


def torch_rowsums(a, b, ia, ib, skip_diag):
    """the yardstick: gather, float32 matmul, cube, sum -- one (m, m) matrix per subset, all subsets batched"""
    x = a if ia is None else a[ia.long()]
    y = b if ib is None else b[ib.long()]
    u = torch.matmul(x, y.transpose(-1, -2)) / a.shape[1] + 1.0
    k = u * u * u
    if skip_diag:
        k = k - torch.diag_embed(torch.diagonal(k, dim1=-2, dim2=-1))
    return k.sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_kid needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import kid_ops, metrics
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events around one call, {a.iters} calls alternating with the torch "
        f"form after 2 warm-up calls: median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    n, d = 8192, 512
    x, y = torch.randn(n, d, device=dev, generator=gen), torch.randn(n, d, device=dev, generator=gen)
    host = torch.Generator().manual_seed(0)
    ix = torch.stack([torch.randperm(n, generator=host)[:1000] for _ in range(100)]).to(torch.int32).to(dev)
    iy = torch.stack([torch.randperm(n, generator=host)[:1000] for _ in range(100)]).to(torch.int32).to(dev)
    cases = (("100 subsets x 1000 x 1000 x 512 (gathered)", ix, iy, 100, 1000), ("8192 x 8192 x 512", None, None, 1, n))
    for what, ia, ib, subsets, m in cases:
        for skip in (False, True):
            out = torch.empty(subsets, m, dtype=torch.float64, device=dev)
            ours = lambda: kid_ops.polyk_rowsums(x, y, ia, ib, skip_diag=skip, out=out)  # noqa: E731
            theirs = lambda: torch_rowsums(x, y, ia, ib, skip)  # noqa: E731
            want = theirs().double()
            diff = float(((ours() - want).abs() / want.abs()).max())
            to, tt = alternating(ours, theirs, a.iters)
            macs = subsets * m * m * d
            blocks = (m + 127) // 128
            ws = kid_ops.polyk_ws_bytes(subsets, m, m)
            # every workgroup stages its 2 x 128 rows once (from the cache, mostly: a set is 16.8 MB); from HBM at least one read
            # of the rows that are named, the partial sums written and read, the row sums written
            staged = subsets * blocks * blocks * 2 * 128 * d * 4
            least = min(subsets * 2 * m, 2 * n) * d * 4 + 2 * ws + subsets * m * 8
            peak_ms = 2 * macs / PEAK_F32 * 1e3
            say(f"--- polyk_rowsums {what}, skip_diag={skip}: {macs / 1e9:.1f} G multiply-adds = {peak_ms:.3f} ms at the fp32-MFMA peak; "
                f"{staged / 1e6:.0f} MB staged through LDS, at least {least / 1e6:.1f} MB from and to HBM = {least / HBM * 1e3:.4f} ms at "
                f"8 TB/s; workspace {ws / 1e6:.1f} MB; the torch form stores {3 * subsets * m * m * 4 / 1e6:.0f} MB of matrices; largest "
                f"relative difference of a row sum {diff:.2e}")
            say("kid_ops.polyk_rowsums (2 launches)".ljust(38) + fmt(to) + f"   {peak_ms / to[0] * 100:.1f} % of the fp32-MFMA peak")
            say("torch (gather, matmul, cube, sum)".ljust(38) + fmt(tt) + f"   polyk_rowsums / torch = {to[0] / tt[0]:.3f}")
    mean, sd = x.double().mean(0), x.double().std(0)
    z = torch.empty_like(x)
    ours = lambda: kid_ops.standardise_rows(x, mean, sd, z)  # noqa: E731
    theirs = lambda: ((x.double() - mean) / sd).float()  # noqa: E731
    same = bool(torch.equal(ours(), theirs()))
    to, tt = alternating(ours, theirs, a.iters)
    nbytes = 2 * n * d * 4
    say(f"--- standardise_rows {n} x {d}: {nbytes / 1e6:.1f} MB = {nbytes / HBM * 1e3:.4f} ms at 8 TB/s; equal to the torch form bit for "
        f"bit: {same}")
    say("kid_ops.standardise_rows".ljust(38) + fmt(to) + f"   {nbytes / HBM * 1e3 / to[0] * 100:.1f} % of the byte floor")
    say("torch (float64 operators)".ljust(38) + fmt(tt) + f"   standardise_rows / torch = {to[0] / tt[0]:.3f}")

    def whole():
        kid = metrics.KID()
        kid.feed_real(x)
        kid.feed_fake(y)
        return kid.result()

    def whole_torch():
        mean, sd = x.double().mean(0), x.double().std(0)
        zx, zy = ((x.double() - mean) / sd).float(), ((y.double() - mean) / sd).float()
        parts = [torch_rowsums(zx, zx, ix, ix, True).sum(1), torch_rowsums(zy, zy, iy, iy, True).sum(1),
                 torch_rowsums(zy, zx, iy, ix, False).sum(1), torch_rowsums(zx, zx, None, None, True).sum(),
                 torch_rowsums(zy, zy, None, None, True).sum(), torch_rowsums(zy, zx, None, None, False).sum()]
        return [p.tolist() for p in parts]

    result = whole()
    to, tt = alternating(whole, whole_torch, max(3, a.iters // 2))
    say(f"--- metrics.KID().result() at {n} + {n} rows of {d}: moments, two standardisations, 3 batched launches of 100 subsets x 1000 x "
        f"1000, 3 launches of 8192 x 8192, the permutations drawn on the host, two read-backs: {result}")
    say("metrics.KID (feeds and result)".ljust(38) + fmt(to))
    say("torch (the same sums, float32)".ljust(38) + fmt(tt) + f"   KID / torch = {to[0] / tt[0]:.3f}")
    say("    (the KID call clones both sets as it is fed them, takes the float64 moments and draws its 200 permutations of 8192 on the "
        "host inside the timed window; the torch form is handed ready index lists and takes a float64 mean and deviation instead)")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
