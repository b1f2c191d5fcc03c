"""FLAC decode on the GPU: a 10-minute stereo 16-bit 44.1 kHz stream (block 4096, LPC order 8, a music-like signal) written by
tests/flac_writer.py; prints its compression ratio, the decode time (scan + chain + decode launches between HIP events, median,
upload excluded) and the compressed GB/s.  Per-kernel shares: run this under `rocprofv3 --kernel-trace --stats`.
`--dataset N`: also times create_dataset on N one-minute files as WAV and as FLAC (files/s).

    python tools/bench_flac.py [--file cache.flac] [--reps 50] [--dataset 8]
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def music(n, seed=0):
    """a few partials with slow amplitude and pitch drift, a decaying noise burst every half second, stereo spread"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = np.zeros((n, 2))
    for k in range(6):
        f = rng.uniform(80, 2000)
        env = 0.5 + 0.5 * np.sin(2 * np.pi * rng.uniform(0.05, 0.5) * t + rng.uniform(0, 6))
        ph = 2 * np.pi * f * t + 3 * np.sin(2 * np.pi * 0.2 * t)
        pan = rng.uniform(0.2, 0.8)
        x[:, 0] += pan * env * np.sin(ph) / 6
        x[:, 1] += (1 - pan) * env * np.sin(ph + 0.3) / 6
    burst = np.exp(-(t % 0.5) * 30)[:, None] * rng.normal(0, 0.05, (n, 2))
    return np.clip(np.round((x + burst) * 20000), -32768, 32767).astype(np.int64)


def write(path, seconds, seed=0):
    import flac_writer as W
    pcm = music(int(44100 * seconds), seed)
    sub = W.SubSpec(kind="lpc", order=8, precision=12, porder=4)
    data = W.encode(pcm, 44100, 16, W.plain_frames(len(pcm), 4096, assign="mid_side", subs=[sub, sub]))
    with open(path, "wb") as fh:
        fh.write(data)
    return pcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default="")
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dataset", type=int, default=0)
    a = ap.parse_args()
    import torch
    from musicgan_amd import _lib, ops
    from musicgan_amd.audio import flac, wavio
    path = a.file or os.path.join(tempfile.mkdtemp(), "bench.flac")
    if not os.path.exists(path):
        write(path, a.minutes * 60)
    info = flac.read_header(path)
    pcm_bytes = info.total_samples * info.channels * 2
    dev = torch.device("cuda", 0)
    buf, n, _ = wavio._flac_region(path, dev)
    ref = ops.flac_decode(buf, info, nbytes=n, name=path)  # also checks the stream
    lib = _lib.load()
    cap = n // 64 + 256
    ws = torch.empty(lib.mg_flac_ws_bytes(n, cap), dtype=torch.uint8, device=dev)
    out = torch.empty_like(ref)
    planar = torch.empty(ref.numel(), dtype=torch.int32, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def scan():
        _lib.check(lib.mg_flac_scan(P(buf), n, P(ws), ws.numel(), cap, s), "scan")

    def decode():
        _lib.check(lib.mg_flac_decode(P(buf), n, P(ws), ws.numel(), cap, info.channels, info.bits, info.sample_rate, P(planar), P(out),
                                      info.total_samples, s), "decode")

    times = {"scan_chain": [], "decode": [], "total": []}
    for r in range(a.reps + 5):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        scan()
        ev[1].record()
        decode()
        ev[2].record()
        torch.cuda.synchronize()
        if r >= 5:
            times["scan_chain"].append(ev[0].elapsed_time(ev[1]))
            times["decode"].append(ev[1].elapsed_time(ev[2]))
            times["total"].append(ev[0].elapsed_time(ev[2]))
    assert torch.equal(out, ref)
    st = ws[:128].view(torch.int64).cpu().tolist()
    med = {k: float(np.median(v)) for k, v in times.items()}
    res = {"file_bytes": os.path.getsize(path), "pcm_bytes": pcm_bytes, "ratio": os.path.getsize(path) / pcm_bytes,
           "frames": st[1], "samples": st[2], "decode_ms_median": med["total"], "scan_chain_ms": med["scan_chain"],
           "frames_ms": med["decode"], "compressed_GBps": n / (med["total"] * 1e-3) / 1e9}
    if a.dataset:
        import musicgan_amd
        from scipy.io import wavfile
        root = tempfile.mkdtemp()
        try:
            for sub in ("wav", "flac"):
                os.makedirs(os.path.join(root, sub))
            for i in range(a.dataset):
                pcm = write(os.path.join(root, "flac", f"f{i}.flac"), 60, seed=i + 1)
                wavfile.write(os.path.join(root, "wav", f"f{i}.wav"), 44100, pcm.astype(np.int16))
            for sub in ("wav", "flac", "wav", "flac"):
                out_dir = os.path.join(root, "out_" + sub)
                shutil.rmtree(out_dir, ignore_errors=True)
                t0 = time.perf_counter()
                musicgan_amd.create_dataset(os.path.join(root, sub, "*." + sub), out_dir)
                res[f"create_dataset_{sub}_files_per_s"] = a.dataset / (time.perf_counter() - t0)  # (second run kept)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
