"""Ogg Vorbis encode on the GPU: the 10-minute stereo 44.1 kHz music-like signal of tools/bench_flac.py (26.5 M frames) at the
default quality (3).  Prints one JSON line: the device encode time (every launch of mg_vorbis_encode between HIP events, median;
the upload and the download of the bytes excluded and timed on their own), the time of each phase (the `phases` mask, each
timed alone after the phases before it have run), the end-to-end ops.vorbis_encode wall time, and the output size in kb/s.

    python tools/bench_vorbis_encode.py [--minutes 10] [--reps 20] [--quality 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quality", type=float, default=3.0)
    a = ap.parse_args()
    import torch
    from bench_flac import music
    from musicgan_amd import ops
    n = int(44100 * a.minutes * 60)
    host = torch.from_numpy(np.ascontiguousarray(music(n).T.astype(np.int16))).pin_memory()
    dev = torch.device("cuda", 0)
    x = host.to(dev)
    j = ops.vorbis_encode_prepare(x, 44100, a.quality, "<bench>")
    times = {"upload": [], "encode": [], "download": []}
    for r in range(a.reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        x.copy_(host, non_blocking=True)
        ev[1].record()
        ops.vorbis_encode_run(j)
        ev[2].record()
        st = j.ws[:128].view(torch.int64).cpu().tolist()
        ev[3].record()
        data = j.out[:st[3]].cpu()
        ev[4].record()
        torch.cuda.synchronize()
        assert st[0] == -1 and st[1] == -1 and st[6] == -1 and st[3] > 0, st[:7]
        if r >= 3:
            times["upload"].append(ev[0].elapsed_time(ev[1]))
            times["encode"].append(ev[1].elapsed_time(ev[2]))
            times["download"].append(ev[3].elapsed_time(ev[4]))
    phases = {}
    for name, bit in ops.VORBIS_ENC_PHASES:
        ts = []
        for r in range(a.reps + 3):
            ops.vorbis_encode_run(j, bit - 1)  # the phases before this one (their outputs are its inputs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.vorbis_encode_run(j, bit)
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                ts.append(e0.elapsed_time(e1))
        phases[name + "_ms"] = float(np.median(ts))
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole = ops.vorbis_encode(x, 44100, a.quality)
        walls.append((time.perf_counter() - t0) * 1e3)
    assert bytes(whole[len(j.head):].numpy()) == bytes(data.numpy())
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"samples": n, "channels": 2, "quality": a.quality, "file_bytes": int(whole.numel()),
           "kbps": whole.numel() * 8 / (n / 44100) / 1000, "encode_ms_median": med["encode"], **phases,
           "upload_ms": med["upload"], "download_ms": med["download"], "vorbis_encode_wall_ms_min": min(walls)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
