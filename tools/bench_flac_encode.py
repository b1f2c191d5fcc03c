"""FLAC encode on the GPU: the 10-minute stereo 16-bit 44.1 kHz music-like signal of tools/bench_flac.py (26.5 M frames, 106 MB of
PCM).  Prints one JSON line: the device encode time (quantise + analyse + offsets + pack + CRC launches between HIP events, median;
the upload and the download of the bytes excluded and timed on their own), its split into the quantise launch and the frame
launches, the host MD5 time, the end-to-end ops.flac_encode wall time, and the compression ratio against the PCM and against
tests/flac_writer.py's LPC order 8 encoding (the file tools/bench_flac.py decodes).  Per-kernel shares: run this under
`rocprofv3 --kernel-trace --stats`.

    python tools/bench_flac_encode.py [--minutes 10] [--reps 20] [--no-writer]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-writer", action="store_true", help="skip the flac_writer LPC-8 comparison (it takes a while)")
    a = ap.parse_args()
    import torch
    from bench_flac import music
    from musicgan_amd import _lib, ops
    n = int(44100 * a.minutes * 60)
    pcm = music(n)
    host = torch.from_numpy(np.ascontiguousarray(pcm.T.astype(np.int16))).pin_memory()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ch, bits = 2, 16
    ws_bytes = int(lib.mg_flac_enc_ws_bytes(n, ch))
    out_bytes = (int(lib.mg_flac_enc_max_bytes(n, ch, bits)) - 42 + 3) // 4 * 4
    x = torch.empty(host.shape, dtype=torch.int16, device=dev)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    planar = torch.empty(ch * n, dtype=torch.int32, device=dev)
    pcm_dev = torch.empty(n * ch * 2, dtype=torch.uint8, device=dev)
    out = torch.zeros(out_bytes, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    times = {"upload": [], "zero_out": [], "quantise": [], "frames": [], "encode": [], "download": []}
    total = 0
    for r in range(a.reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        ev[0].record()
        x.copy_(host, non_blocking=True)
        ev[1].record()
        out.zero_()
        ev[2].record()
        _lib.check(lib.mg_flac_enc_quantise(P(x), 2, n, ch, n, bits, P(planar), P(pcm_dev), P(ws), ws_bytes, s), "quantise")
        ev[3].record()
        _lib.check(lib.mg_flac_enc_frames(P(planar), ch, n, bits, 44100, P(ws), ws_bytes, P(out), out_bytes, s), "frames")
        ev[4].record()
        st = ws[:128].view(torch.int64).cpu().tolist()
        total = st[0]
        ev5 = torch.cuda.Event(enable_timing=True)
        ev5.record()
        data = out[:total].cpu()
        ev[5].record()
        torch.cuda.synchronize()
        if r >= 3:
            times["upload"].append(ev[0].elapsed_time(ev[1]))
            times["zero_out"].append(ev[1].elapsed_time(ev[2]))
            times["quantise"].append(ev[2].elapsed_time(ev[3]))
            times["frames"].append(ev[3].elapsed_time(ev[4]))
            times["encode"].append(ev[2].elapsed_time(ev[4]))
            times["download"].append(ev5.elapsed_time(ev[5]))
        assert st[5] == 0 and st[3] == 0, st[:6]
    med = {k: float(np.median(v)) for k, v in times.items()}
    raw = pcm_dev.cpu().numpy()
    t0 = time.perf_counter()
    md5 = hashlib.md5(memoryview(raw)).digest()
    md5_ms = (time.perf_counter() - t0) * 1e3
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        whole = ops.flac_encode(x, 44100)
        walls.append((time.perf_counter() - t0) * 1e3)
    whole16 = ops.flac_encode(x, 44100, 16)
    assert bytes(whole16[42:].numpy()) == bytes(data.numpy()) and bytes(whole16[26:42].numpy()) == md5
    file_bytes = 42 + total
    res = {"samples": n, "channels": ch, "bits": bits, "pcm_bytes": 4 * n, "file_bytes": file_bytes,
           "ratio_vs_pcm": file_bytes / (4 * n), "encode_ms_median": med["encode"], "quantise_ms": med["quantise"],
           "frames_ms": med["frames"], "upload_ms": med["upload"], "zero_output_ms": med["zero_out"],
           "download_ms": med["download"], "md5_host_ms": md5_ms, "flac_encode_wall_ms_min": min(walls),
           "flac_encode_bytes": int(whole.numel())}
    if not a.no_writer:
        import flac_writer as W
        sub = W.SubSpec(kind="lpc", order=8, precision=12, porder=4)
        ref = W.encode(pcm, 44100, 16, W.plain_frames(n, 4096, assign="mid_side", subs=[sub, sub]))
        res["writer_lpc8_bytes"] = len(ref)
        res["ratio_vs_writer_lpc8"] = file_bytes / len(ref)
        res["writer_lpc8_ratio_vs_pcm"] = len(ref) / (4 * n)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
