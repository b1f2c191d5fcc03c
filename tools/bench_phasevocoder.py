"""Times the phase vocoder (csrc/phasevocoder.hip) at T = 103 360 frames (BASELINE config 5's 10-minute track) and T = 5 120 for the
rates 9/10 and 10/9 (and 2/1, the other form of the first launch): the whole call of four launches next to its bytes at 8 TB/s,
and beside it `codec_fwd` on the same frame count (codec_row_pass: the same scan shape and the same atan2 per bin).  Per launch
the bytes and the atan2 / sincos counts are computed from the shapes; per-launch times come from a kernel trace of this script.
With identity phase locking (`lock=True`, the pvl_* launches) the same shapes again, next to the unlocked time of the same run, to
codec_fwd and to the device work of one create_dataset file (STFT of the track + codec_fwd); its launches step through their frames
one barrier at a time, so the bytes say little about their time.
HIP-event timing, warmed up, median and spread.  The data is synthetic (complex normal).
   python tools/bench_phasevocoder.py [--iters 20] [--out profiles/phasevocoder_kernels.txt]
   rocprofv3 --kernel-trace --stats -- python tools/bench_phasevocoder.py --iters 5"""
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


def fmt(t):
    return f"{t[0]:9.4f} [{t[1]:8.4f} .. {t[2]:8.4f}] ms"


def counts(frames, p, q, tile):
    """per launch: (name, bytes read, bytes written, atan2 + hypot pairs, sincos) from the shapes alone"""
    n = -((-frames * q) // p)
    polar = 512 * (min(frames, 2 * n) if p >= 2 * q else frames)
    tiles = 512 * (-(-n // tile))
    touched = 512 * min(frames, 2 * n)   # staged bins the two tile passes read (each once from HBM or L2, neighbours share them)
    return n, [("pv_polar", 8 * polar, 8 * polar, polar, 0),
               ("pv_tile_sums", 8 * touched, 8 * tiles, 0, 0),
               ("pv_row_scan", 8 * tiles, 8 * tiles, 0, 0),
               ("pv_finish", 8 * touched + 8 * tiles, 8 * 512 * n, 0, 512 * n)]


def locked_counts(frames, p, q, tile):
    """the launches of the locked vocoder: (name, bytes read, bytes written, workgroups, sequential frame steps per workgroup)"""
    n = -((-frames * q) // p)
    polar = 512 * (min(frames, 2 * n) if p >= 2 * q else frames)
    touched = 512 * min(frames, 2 * n)
    bins, tiles = 512 * n, -(-n // tile)
    return n, [("pv_polar", 8 * polar, 8 * polar, -(-polar // 256), 0),
               ("pvl_prepare", 8 * touched, 18 * bins, -(-n // 4), 4),
               ("pvl_tile_map", 10 * 512 * tile * (tiles - 1), 11 * 512 * (tiles - 1), tiles - 1, tile),
               ("pvl_carry", 11 * 512 * (tiles - 1), 9 * 512 * tiles, 1, tiles),
               ("pvl_finish", 18 * bins + 9 * 512 * tiles, 8 * bins, tiles, tile)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_phasevocoder needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import _lib, ops, pv_ops
    from musicgan_amd.audio.functions import _bark_vector
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events, {a.iters} repeats after 2 warm-up runs: median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    bark = _bark_vector(512, dev)
    for frames in (5120, 103360):
        X = torch.view_as_complex(torch.randn(512, frames, 2, device=dev, generator=gen))
        say(f"--- T = {frames} frames ({512 * frames / 1e6:.2f} M input bins)")
        t_codec = timed(lambda: ops.codec_fwd(X, bark, 512), a.iters)
        wav = torch.randn(256 * (frames - 1), device=dev, generator=gen)
        t_file = timed(lambda: ops.codec_fwd(ops.stft_1024(wav), bark, 512), a.iters)
        del wav
        unlocked = {}
        say("codec_fwd (codec_row_pass + normalise), same T".ljust(52) + fmt(t_codec) + "   (comparison: the same scan shape, one atan2 per bin)")
        for p, q in ((9, 10), (10, 9), (2, 1)):
            n, per = counts(frames, p, q, pv_ops.TIME_TILE)
            t = timed(lambda: pv_ops.phase_vocoder(X, p, q), a.iters)
            unlocked[p, q] = t
            total = sum(r + w for _, r, w, _, _ in per)
            floor = 16 * 512 * n   # the input read once (8 B per output bin at rate 1) and the output written
            say(f"phase_vocoder {p}/{q}: {n} output frames".ljust(52) + fmt(t) + f"   {total / 1e6:8.1f} MB moved = {total / HBM * 1e3:.4f} ms at 8 TB/s "
                f"({total / HBM * 1e3 / t[0] * 100:.1f} % of the time); floor 16 B per output bin = {floor / HBM * 1e3:.4f} ms "
                f"({floor / HBM * 1e3 / t[0] * 100:.1f} %); {t[0] / t_codec[0]:.2f} x codec_fwd")
            for name, r, w, at, sc in per:
                say(f"    {name:<14} reads {r / 1e6:9.2f} MB, writes {w / 1e6:9.2f} MB, atan2+hypot {at / 1e6:7.2f} M, sincos (float64) {sc / 1e6:7.2f} M")
        say("one create_dataset file on the device (stft_1024 + codec_fwd), same T".ljust(52) + fmt(t_file))
        for p, q in ((9, 10), (10, 9), (2, 1)):
            n, per = locked_counts(frames, p, q, pv_ops.LOCK_TILE)
            t = timed(lambda: pv_ops.phase_vocoder(X, p, q, lock=True), a.iters)
            total = sum(r + w for _, r, w, _, _ in per)
            ws = int(_lib.load().mg_phase_vocoder_locked_ws_bytes(frames, p, q))
            say(f"phase_vocoder {p}/{q}, lock=True: {n} output frames".ljust(52) + fmt(t) + f"   {total / 1e6:8.1f} MB moved = {total / HBM * 1e3:.4f} ms at 8 TB/s "
                f"({total / HBM * 1e3 / t[0] * 100:.1f} % of the time); {t[0] / unlocked[p, q][0]:.2f} x the unlocked call, "
                f"{t[0] / t_codec[0]:.2f} x codec_fwd, {t[0] / t_file[0]:.2f} x one file's device work; workspace {ws / 1e6:.1f} MB")
            for name, r, w, groups, steps in per:
                say(f"    {name:<14} reads {r / 1e6:9.2f} MB, writes {w / 1e6:9.2f} MB = {(r + w) / HBM * 1e3:.4f} ms at 8 TB/s; "
                    f"{groups} workgroups x {steps} sequential frame steps")
        del X
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
