"""Times the kernels of the waveform log-mel rows (csrc/melspec.hip) through musicgan_amd.mel_ops: mel_power on a 10-minute file
(1, 26 460 000) and on (16, 130 816) -- what evaluate_mel --waveform launches per batch --, each next to the unfused route on the same
device, alternating: ops.stft_1024 per row (the spectrum written to memory), abs() ** 2, and a float32 matmul with the dense bank
(zeros outside the bands; not the code under test).  Then logmel_pool on the power of both shapes, on its own.  Beside every figure
the bytes the launch has to move at 8 TB/s: the samples read once and the (M, T) power written for mel_power; the power read and the
rows written for logmel_pool.  Every timed window holds --calls calls between two HIP events; warmed up, median and spread of --iters
windows, per call.  The data is synthetic (uniform in [-1, 1]).
   python tools/bench_melspec.py [--iters 10] [--calls 10] [--out profiles/melspec_kernels.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_prdc import alternating, fmt  # noqa: E402  (tools/ is on the path when this file is run)

HBM = 8e12  # bytes/s


def unfused(ops, waves, dense):
    """the yardstick: one STFT launch per row, the power of the spectrum, a dense float32 matmul with the (M, 512) bank"""
    return torch.stack([torch.matmul(dense, ops.stft_1024(row).abs() ** 2) for row in waves])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_melspec needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import mel_ops, metrics, ops
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

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events around {a.calls} calls, {a.iters} windows alternating with the "
        f"unfused form after 2 warm-up windows: per call, median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    wl = metrics.WaveLogMel()
    weight = wl.weight.to(dev)
    dense = torch.nan_to_num(weight)
    for b, length, what in ((1, 600 * 44100, "a 10-minute file"), (16, 130816, "16 decoded images")):
        waves = torch.rand(b, length, device=dev, generator=gen) * 2 - 1
        frames = mel_ops.mel_frames(length)
        power = torch.empty(b, wl.bands, frames, device=dev)
        ours = lambda: mel_ops.mel_power(waves, weight, wl.lo, wl.hi, power)  # noqa: E731
        theirs = lambda: unfused(ops, waves, dense)  # noqa: E731
        want = theirs()
        diff = float(((ours() - want).abs() / want.abs().max()).max())
        to, tt = alternating(per_call(ours), per_call(theirs), a.iters)
        to, tt = tuple(v / a.calls for v in to), tuple(v / a.calls for v in tt)
        nbytes = b * length * 4 + b * wl.bands * frames * 4
        floor_ms = nbytes / HBM * 1e3
        spectrum = b * 512 * frames * 8
        say(f"--- mel_power ({b}, {length}) -> ({b}, 64, {frames}), {what}: {nbytes / 1e6:.1f} MB = {floor_ms:.4f} ms at 8 TB/s (the "
            f"unfused route also writes and reads a spectrum of {spectrum / 1e6:.1f} MB); largest difference to it / largest value "
            f"{diff:.2e}")
        say("mel_ops.mel_power (1 launch)".ljust(34) + fmt(to) + f"   {floor_ms / to[0] * 100:.1f} % of the byte floor")
        say(f"stft_1024 x {b}, abs ** 2, matmul".ljust(34) + fmt(tt) + f"   mel_power / unfused = {to[0] / tt[0]:.3f}")
        for pools in (32, 8):
            rows = torch.empty(b * mel_ops.pool_windows(frames, 512, 512), wl.bands * pools, device=dev)
            pool = lambda: mel_ops.logmel_pool(power, 512, 512, pools, wl.floor, rows)  # noqa: E731
            tp, _ = alternating(per_call(pool), per_call(pool), a.iters)
            tp = tuple(v / a.calls for v in tp)
            nbytes = power.numel() * 4 + rows.numel() * 4
            floor_ms = nbytes / HBM * 1e3
            say(f"logmel_pool -> {tuple(rows.shape)}".ljust(34) + fmt(tp) + f"   {nbytes / 1e6:.1f} MB = {floor_ms:.4f} ms at 8 TB/s: "
                f"{floor_ms / tp[0] * 100:.1f} % of the byte floor")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
