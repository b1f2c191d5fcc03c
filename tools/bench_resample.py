"""mg_resample_pcm on synthetic 10-minute stereo int16 files at 48 and 96 kHz (-> 44.1 kHz), warmed up: kernel time from HIP
events, bytes moved (PCM in + float32 mono out), fraction of 8 TB/s; then create_dataset files/s on eight 48 kHz files against the
same eight at 44.1 kHz (set-up excluded, as tools/bench_create_dataset.py reports it).
   python tools/bench_resample.py [--seconds 600] [--iters 50] [--files 8] [--kernel-only]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

HBM = 8e12  # bytes/s


def kernel_rows(seconds: int, iters: int):
    from musicgan_amd import ops
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(3)
    for orig in (48000, 96000):
        frames = orig * seconds
        pcm = torch.randint(-32768, 32767, (frames, 2), dtype=torch.int16, device="cuda", generator=gen)
        for _ in range(5):
            out = ops.resample_pcm(pcm, orig, 44100)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * iters)]
        for i in range(iters):
            ev[2 * i].record()
            out = ops.resample_pcm(pcm, orig, 44100)
            ev[2 * i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(iters))
        nbytes = pcm.numel() * 2 + out.numel() * 4
        med = ms[len(ms) // 2]
        rows.append({"orig_hz": orig, "frames": frames, "out_samples": out.numel(), "bytes": nbytes, "ms_median": round(med, 4),
                     "ms_min": round(ms[0], 4), "hbm_fraction": round(nbytes / (med * 1e-3) / HBM, 3)})
        del pcm, out
    return rows


def create_dataset_rows(seconds: int, nfiles: int, reps: int = 2):
    from scipy.io import wavfile
    from musicgan_amd import create_dataset
    tmp = tempfile.mkdtemp(prefix="mg_rs_")
    rows = []
    try:
        rng = np.random.default_rng(7)
        for sr in (48000, 44100):
            d = os.path.join(tmp, f"wav{sr}")
            os.mkdir(d)
            for i in range(nfiles):
                wavfile.write(os.path.join(d, f"track_{i}.wav"), sr, rng.integers(-20000, 20000, (sr * seconds, 2), dtype=np.int16))
        for r in range(reps):
            for sr in (48000, 44100):
                out = os.path.join(tmp, "data")
                st = {}
                t0 = time.perf_counter()
                create_dataset(os.path.join(tmp, f"wav{sr}", "track_*.wav"), out, stats=st, resample=True)
                wall = time.perf_counter() - t0
                rows.append({"rate_hz": sr, "rep": r, "files": st["files"], "samples": st["samples"],
                             "files_per_s_after_setup": round(nfiles / (wall - st["setup_s"]), 2), "wall_s": round(wall, 3),
                             "load_stft_s": round(st["load_stft_s"], 3)})
                shutil.rmtree(out)
                os.sync()
                time.sleep(1.0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    for row in kernel_rows(a.seconds, a.iters):
        print(json.dumps({"resample_kernel": row}), flush=True)
    if not a.kernel_only:
        for row in create_dataset_rows(a.seconds, a.files):
            print(json.dumps({"create_dataset_resample": row}), flush=True)


if __name__ == "__main__":
    main()
