"""Times the loudness kernels (csrc/loudness.hip) on a 10-minute stereo file at 44.1 kHz (C = 2, L = 26 460 000) and on 30 s of it:
the segment energies (two passes over the signal), the gates, true peak (one pass) and the gain with its scaling (one pass read,
one written), each next to its HBM floor of 4 B x C x L per pass that reads or writes the signal at 8 TB/s.  HIP-event timing,
warmed up, median and spread.  The data is synthetic (uniform noise).
   python tools/bench_loudness.py [--iters 20] [--out profiles/loudness_kernels.txt]
   rocprofv3 --kernel-trace --stats -- python tools/bench_loudness.py --iters 5"""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loudness needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import audio, loud_ops
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def row(name, t, passes, nbytes):
        floor = passes * nbytes / HBM * 1e3
        say(f"{name:<46}{t[0]:9.4f} [{t[1]:8.4f} .. {t[2]:8.4f}] ms   floor {passes} x {nbytes / 1e6:.1f} MB = {floor:.4f} ms "
            f"({floor / t[0] * 100:.1f} % of the time)")

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    say(f"CHUNK = {loud_ops.CHUNK}; floor = passes over the signal x 4 B x C x L at 8 TB/s")
    gen = torch.Generator(device=dev).manual_seed(0)
    fs = 44100
    for seconds in (30, 600):
        x = torch.rand(2, seconds * fs, device=dev, generator=gen) - 0.5
        nbytes = 4 * x.numel()
        say(f"--- {seconds} s stereo at {fs} Hz: C = 2, L = {x.shape[1]} ({nbytes / 1e6:.1f} MB)")
        energies = loud_ops.segment_energies(x, fs)
        record, peak = loud_ops.gate(energies, fs), loud_ops.true_peak(x)
        row("segment_energies (4 launches, reads twice)", timed(lambda: loud_ops.segment_energies(x, fs), a.iters), 2, nbytes)
        say(f"{'gate (1 launch, ' + str(energies.shape[1] - 3) + ' blocks)':<46}{timed(lambda: loud_ops.gate(energies, fs), a.iters)[0]:9.4f} ms")
        row("true_peak (2 launches, reads once)", timed(lambda: loud_ops.true_peak(x), a.iters), 1, nbytes)
        row("normalize (2 launches, reads and writes once)", timed(lambda: loud_ops.normalize(x, record, peak, -14.0, -1.0), a.iters), 2, nbytes)
        row("audio.loudness (energies + gate)", timed(lambda: audio.loudness(x, fs), a.iters), 2, nbytes)
        row("audio.normalize_loudness (all of the above)", timed(lambda: audio.normalize_loudness(x, fs), a.iters), 5, nbytes)
        say(f"    measured: {float(record[0]):.3f} LUFS, true peak {float(peak):.6f}")
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
