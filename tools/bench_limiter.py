"""Times the limiter kernels (csrc/limiter.hip) on a 10-minute stereo file at 44.1 kHz (C = 2, L = 26 460 000) and on 30 s of it:
the envelope alone, the whole `limit` (five launches), the trim, and `audio.normalize_loudness` with and without the limiter in the
same call, each next to the bytes it has to move at 8 TB/s.  HIP-event timing, warmed up, median and spread.  The data is synthetic:
the prototype's kind of signal (a sine, noise and sparse spikes), so that the limiter has peaks to hold.
   python tools/bench_limiter.py [--iters 20] [--out FILE]     (profiles/limiter_kernels.txt holds its lines)
   rocprofv3 --kernel-trace --stats -- python tools/bench_limiter.py --iters 5 --seconds 600"""
import argparse
import math
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


def launch_bytes(channels, length, lookahead, tile):
    """{launch: (bytes read, bytes written)} of one `limit`, from the kernels' loops (halos included)"""
    tiles = -(-(length + lookahead) // tile)
    halo = 1 + lookahead / tile
    return {"lim_env_k": (4 * channels * length, 4 * length),
            "lim_release_k<false>": (4 * length * halo, 8 * tiles),
            "lim_carry_k": (16 * tiles, 8 * tiles),
            "lim_release_k<true>": (4 * length * halo + 8 * tiles, 8 * (length + lookahead)),
            "lim_out_k": (8 * length * halo + 4 * length + 4 * channels * length, 4 * channels * length)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seconds", type=int, nargs="*", default=[30, 600])
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_limiter needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import audio, lim_ops, loud_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(name, t, nbytes):
        floor = nbytes / HBM * 1e3
        say(f"{name:<58}{t[0]:9.4f} [{t[1]:8.4f} .. {t[2]:8.4f}] ms   {nbytes / 1e6:8.1f} MB = {floor:.4f} ms at 8 TB/s "
            f"({floor / t[0] * 100:.1f} % of the time)")

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    fs, target = 44100, -20.0
    ceiling, lookahead, rho = lim_ops.check_arguments(fs)
    say(f"TILE = {lim_ops.TILE}, look-ahead {lookahead} samples, rho = {rho:.9f}, ceiling {ceiling:.6f}; target {target} LUFS")
    gen = torch.Generator(device=dev).manual_seed(0)
    for seconds in a.seconds:
        n = seconds * fs
        t = torch.arange(n, device=dev, dtype=torch.float64) / fs
        x = (0.2 * torch.sin(2 * math.pi * 220.0 * t)).float()[None, :].repeat(2, 1)
        x += 0.1 * torch.randn(2, n, device=dev, generator=gen)
        spikes = torch.randint(0, n, (100 * seconds,), device=dev, generator=gen)
        x[0, spikes] += 0.8 * torch.randn(spikes.numel(), device=dev, generator=gen)
        del t
        signal = 4 * x.numel()
        say(f"--- {seconds} s stereo at {fs} Hz: C = 2, L = {n} ({signal / 1e6:.1f} MB)")
        per = launch_bytes(2, n, lookahead, lim_ops.TILE)
        total = sum(r + w for r, w in per.values())
        record = loud_ops.gate(loud_ops.segment_energies(x, fs), fs)
        pre = lim_ops.pregain(record, target)
        y = lim_ops.limit(x, pre, ceiling, lookahead, rho)
        peak = loud_ops.true_peak(y)
        row("envelope (1 launch)", timed(lambda: lim_ops.envelope(x), a.iters), sum(per["lim_env_k"]))
        row("limit (5 launches: what they move)", timed(lambda: lim_ops.limit(x, pre, ceiling, lookahead, rho), a.iters), total)
        row("limit (the least: x twice, y once)", timed(lambda: lim_ops.limit(x, pre, ceiling, lookahead, rho), a.iters), 3 * signal)
        row("trim (1 launch)", timed(lambda: lim_ops.trim(y, peak, ceiling), a.iters), 2 * signal)
        plain = timed(lambda: audio.normalize_loudness(x, fs, target_lufs=target), a.iters)
        limited = timed(lambda: audio.normalize_loudness(x, fs, target_lufs=target, limiter=True), a.iters)
        row("audio.normalize_loudness", plain, 5 * signal)
        row("audio.normalize_loudness(limiter=True, passes=2)", limited, 7 * signal + 2 * total)
        out, (lufs, peak_db, reduction) = audio.normalize_loudness(x, fs, target_lufs=target, limiter=True, return_details=True)
        static = float(audio.loudness(audio.normalize_loudness(x, fs, target_lufs=target), fs))
        say(f"    reached: {float(lufs):.3f} LUFS at {float(peak_db):.4f} dBTP, largest reduction {float(reduction):.2f} dB; "
            f"one gain reaches {static:.3f} LUFS; pre-gain {float(pre):.4f}")
        del x, y, out
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
