"""Times the Griffin-Lim kernels (csrc/griffinlim.hip) at TT = 5 120 frames (generate's default -n 10) and TT = 103 360 (BASELINE
config 5's 10-minute track): the inverse STFT alone, the forward STFT, the projection, and whole loops of 8 and 32 iterations, each
next to what it has to move at least at 8 TB/s.  As the comparison, never on the product path: what the tree had before -- the
codec's own inverse (inv_frames + inv_overlap_add, timed as `ops.codec_inv` minus its front half `gl_ops.codec_inv_spectrum`), and an
iteration made of that inverse's cost, `ops.stft_1024` and the projection in torch operators.  HIP-event timing, warmed up, median
and spread; per-launch times come from a kernel trace of `--launches-only`.  The data is synthetic (uniform in [-1, 1]).
   python tools/bench_griffinlim.py [--iters 20] [--launches-only] [--out profiles/griffinlim_kernels.txt]"""
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
    return f"{t[0]:9.3f} [{t[1]:8.3f} .. {t[2]:8.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--launches-only", action="store_true", help="the per-launch part alone (for a kernel trace)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_griffinlim needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import gl_ops, ops
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
    for n, w in ((10, 512), (190, 544)):
        tt = n * w
        bins, frames = 512 * tt, tt
        mp = torch.rand(n, 2, 512, w, device=dev, generator=gen) * 2 - 1
        M, Z0 = gl_ops.codec_inv_spectrum(mp, bark)
        wav = gl_ops.istft_1024(Z0)
        say(f"--- TT = {tt} frames ({bins / 1e6:.2f} M bins, {wav.numel() / 44100:.0f} s of audio)")
        b_inv = 8 * bins + 1024 * frames
        t_new = timed(lambda: gl_ops.istft_1024(Z0), a.iters)
        say("istft1024_kernel (new inverse)".ljust(44) + fmt(t_new) + f"   {b_inv / 1e6:8.1f} MB min = {b_inv / HBM * 1e3:.4f} ms at 8 TB/s: "
            f"{b_inv / HBM * 1e3 / t_new[0] * 100:.1f} % of it")
        t_fwd = timed(lambda: ops.stft_1024(wav), a.iters)
        say("stft1024_kernel (forward, unchanged)".ljust(44) + fmt(t_fwd) + f"   {b_inv / 1e6:8.1f} MB min = {b_inv / HBM * 1e3:.4f} ms")
        Z = Z0.clone()
        t_one = timed(lambda: gl_ops.griffin_lim(M, Z, 1, 0.99), a.iters)
        say("1 iteration + final inverse (5 launches)".ljust(44) + fmt(t_one))
        if a.launches_only:
            continue
        t_whole, t_front = timed(lambda: ops.codec_inv(mp, bark), a.iters), timed(lambda: gl_ops.codec_inv_spectrum(mp, bark), a.iters)
        old_inv = t_whole[0] - t_front[0]
        b_old = 8 * 2 * bins + (4096 + 4 * 4096 + 1024) * frames   # Z read twice (Hermitian extension), frames written and gathered 4 x
        say("codec_inv, whole (6 launches)".ljust(44) + fmt(t_whole))
        say("codec_inv_spectrum, its front (4 launches)".ljust(44) + fmt(t_front))
        say(f"  => inv_frames + inv_overlap_add (old inverse): {old_inv:9.3f} ms; {b_old / 1e6:.1f} MB requested; the new inverse is "
            f"{old_inv / t_new[0]:.2f} x as fast")
        R, prev = ops.stft_1024(wav), ops.stft_1024(wav)
        Mc = M

        def torch_project():
            c = R - 0.4975 * prev
            return Mc * (c / (c.abs() + 1e-16)), R.clone()

        t_tp = timed(torch_project, a.iters)
        say("projection in torch operators".ljust(44) + fmt(t_tp) + "   (comparison, not used by the product)")
        for k in (8, 32):
            t_loop = timed(lambda: gl_ops.griffin_lim(M, Z, k, 0.99, return_convergence=True), max(3, a.iters // 4), warm=1)
            new_it = (t_loop[0] - t_new[0]) / k
            old_it = old_inv + t_fwd[0] + t_tp[0]
            b_it = (8 + 8) * bins + 2 * 1024 * frames + (8 + 8 + 4 + 8) * bins
            say(f"griffin_lim, {k} iterations + final inverse".ljust(44) + fmt(t_loop) + f"   {new_it:.3f} ms per iteration ({b_it / 1e6:.1f} MB min = "
                f"{b_it / HBM * 1e3:.4f} ms at 8 TB/s); the parent's means: {old_it:.3f} ms per iteration, {old_it / new_it:.2f} x")
        del mp, M, Z0, Z, R, prev, wav
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
