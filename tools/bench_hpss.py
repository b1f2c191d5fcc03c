"""Times the harmonic / percussive separation (csrc/hpss.hip, one fused launch) at T = 512 and T = 103 360 frames (BASELINE config 5's
10-minute track), for the default kernel lengths 31 / 31 (the selection network of 32 inputs, no padding) and for 17 / 9 (the same
network, padded windows) and 63 / 63 (the network of 64 inputs), next to its bytes at 8 TB/s; `mg_ola_stretch` on 10 minutes of samples; and the same definition written with torch
operators on the device (reflected index, `unfold` + `median`, element-wise masks) at the largest T that fits, whose medians are
also compared bit for bit with the kernel's at that size.  Bytes are computed from the shapes; per-kernel times come from a kernel
trace of this script.  HIP-event timing, warmed up, median and spread.  The data is synthetic (complex normal).
   python tools/bench_hpss.py [--iters 20] [--out profiles/hpss_kernels.txt]
   rocprofv3 --kernel-trace --stats -- python tools/bench_hpss.py --iters 5"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM = 8e12  # bytes/s
TILE = 64


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
    return f"{t[0]:9.4f} [{t[1]:8.4f} .. {t[2]:8.4f}] ms"


def counts(frames, lh, lp):
    """(floor bytes, bytes with the halo, magnitudes staged per output bin): the floor reads X once and writes the two spectra (24 B
    per bin); a tile of 64 x 64 bins stages 64 x (64 + lh - 1) + (lp - 1) x 64 bins, each read once from HBM or L2"""
    bins = 512 * frames
    tiles = 8 * (-(-frames // TILE))
    staged = tiles * (TILE * (TILE + lh - 1) + (lp - 1) * TILE)
    return 24 * bins, 8 * staged + 8 * bins + 16 * bins, staged / bins


def _reflected(n, half, device):
    j = torch.arange(-half, n + half, device=device) % (2 * n)
    return torch.where(j < n, j, 2 * n - 1 - j)


def torch_hpss(X, lh=31, lp=31, S=None):
    """the definition (power 2, margins 1) in torch operators on the device; S: |X| where the device's own is not wanted"""
    S = X.abs() if S is None else S
    H = S[:, _reflected(S.shape[1], lh // 2, S.device)].unfold(1, lh, 1).median(dim=-1).values
    P = S[_reflected(S.shape[0], lp // 2, S.device), :].unfold(0, lp, 1).median(dim=-1).values
    Z = torch.maximum(H, P)
    bad = Z < torch.finfo(torch.float32).tiny
    Z = torch.where(bad, torch.ones_like(Z), Z)
    a, b = (H / Z) ** 2, (P / Z) ** 2
    mh = torch.where(bad, torch.full_like(a, 0.5), a / torch.where(bad, torch.ones_like(a), a + b))
    mp = torch.where(bad, torch.full_like(a, 0.5), b / torch.where(bad, torch.ones_like(a), a + b))
    return X * mh, X * mp, H, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hpss needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import hpss_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    for frames in (512, 103360):
        X = torch.view_as_complex(torch.randn(512, frames, 2, device=dev, generator=gen))
        say(f"--- T = {frames} frames ({512 * frames / 1e6:.2f} M bins)")
        for lh, lp in ((31, 31), (17, 9), (63, 63)):
            floor, moved, staged = counts(frames, lh, lp)
            t = timed(lambda: hpss_ops.hpss(X, (lh, lp)), a.iters if (lh, lp) == (31, 31) else max(3, a.iters // 4))
            say(f"mg_hpss {lh} x {lp} ({'32' if max(lh, lp) <= 31 else '64'} inputs{'' if lh == lp == 31 else ', padded' if max(lh, lp) < 63 else ''})".ljust(38) + fmt(t) +
                f"   floor 24 B/bin = {floor / 1e6:8.1f} MB = {floor / HBM * 1e3:.4f} ms at 8 TB/s ({floor / HBM * 1e3 / t[0] * 100:.1f} % of the time); "
                f"with the halo {moved / 1e6:8.1f} MB = {moved / HBM * 1e3:.4f} ms; {staged:.2f} magnitudes staged per bin; "
                f"{512 * frames / t[0] / 1e6:.2f} G bins/s")
        del X
        torch.cuda.empty_cache()
    samples = 10 * 60 * 44100
    x = torch.rand(samples, device=dev, generator=gen) - 0.5
    for p, q in ((1, 1), (9, 10), (10, 9)):
        n = -((-samples * q) // p)
        t = timed(lambda: hpss_ops.ola_stretch(x, p, q, n), a.iters)
        moved = 4 * min(samples, 2 * n) + 4 * n
        say(f"mg_ola_stretch {p}/{q}: {n} samples".ljust(42) + fmt(t) + f"   {moved / 1e6:7.1f} MB = {moved / HBM * 1e3:.4f} ms at 8 TB/s "
            f"({moved / HBM * 1e3 / t[0] * 100:.1f} % of the time)")
    del x
    frames = 103360
    while frames >= 512:
        try:
            X = torch.view_as_complex(torch.randn(512, frames, 2, device=dev, generator=gen))
            t = timed(lambda: torch_hpss(X), max(3, a.iters // 4), warm=1)
            break
        except torch.cuda.OutOfMemoryError:
            del X
            torch.cuda.empty_cache()
            frames //= 2
    say(f"--- torch operators (index, unfold + median, masks), T = {frames}")
    mine = timed(lambda: hpss_ops.hpss(X), a.iters)
    say("torch operators 31 x 31".ljust(38) + fmt(t) + f"   {t[0] / mine[0]:.1f} x mg_hpss at the same T ({mine[0]:.4f} ms)")
    ref = torch_hpss(X, S=X.cpu().abs().to(dev))     # |X| with the CPU's bits, which the kernel restates: the selections are compared
    got = hpss_ops.hpss(X, want=("harmonic", "percussive", "H", "P"))
    same = [bool(torch.equal(u.view(torch.int32), v.view(torch.int32))) for u, v in zip(ref[2:], got[2:])]
    err = max(float((u - v).abs().max()) for u, v in zip(ref[:2], got[:2]))
    say(f"at T = {frames}: H bit-identical to torch's median: {same[0]}, P: {same[1]}; largest |component - torch's| = {err:.3e}")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
