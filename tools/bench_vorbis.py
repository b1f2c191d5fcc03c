"""Ogg Vorbis decode on the GPU: a 10-minute stereo 44.1 kHz stream laid out by tests/vorbis_writer.py from the libvorbis fixture's
non-silent long-block packets (real codebooks, floors and residue 2), repeated; prints the host parse time (page walk, headers,
packet table), the device decode time (every phase between HIP events, median, upload excluded) and its split by phase.
`--dataset N`: also times create_dataset on N one-minute files as WAV and as OGG (files/s).

    python tools/bench_vorbis.py [--file cache.ogg] [--reps 30] [--dataset 8]
"""
import argparse
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


def write(path, seconds, seed=0):
    import vorbis_writer as W
    _, audio, _ = W.fixture_packets()
    long_voiced = audio[5:14]  # 79-209 bytes each, both floors used
    rng = np.random.default_rng(seed)
    n = int(seconds * 44100 / 1024) + 1
    pk = [audio[4]] + [long_voiced[i] for i in rng.integers(0, len(long_voiced), n)]
    data = W.stream(pk, max_segments=255)
    with open(path, "wb") as fh:
        fh.write(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--file", default="")
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dataset", type=int, default=0)
    a = ap.parse_args()
    import torch
    from musicgan_amd import ops
    from musicgan_amd.audio import vorbis
    path = a.file or os.path.join(tempfile.mkdtemp(), "bench.ogg")
    if not os.path.exists(path):
        write(path, a.minutes * 60)
    raw = np.fromfile(path, dtype=np.uint8)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        vs = vorbis.parse(raw, path)
        vorbis.pack_setup(vs.setup)
        host.append((time.perf_counter() - t0) * 1e3)
    dev = torch.device("cuda", 0)
    data = torch.from_numpy(raw).to(dev)
    ref = ops.vorbis_decode(data, vs, name=path)  # also checks the stream
    job = ops.vorbis_prepare(data, vs, name=path)
    names = [n for n, _ in ops.VORBIS_PHASES]
    times = {n: [] for n in names + ["total"]}
    for r in range(a.reps + 3):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        ev[0].record()
        for i, (_, bit) in enumerate(ops.VORBIS_PHASES):
            ops.vorbis_run(job, bit)
            ev[i + 1].record()
        torch.cuda.synchronize()
        if r >= 3:
            for i, nm in enumerate(names):
                times[nm].append(ev[i].elapsed_time(ev[i + 1]))
            times["total"].append(ev[0].elapsed_time(ev[-1]))
    assert torch.equal(job.out, ref)
    med = {k: float(np.median(v)) for k, v in times.items()}
    secs = vs.frames / vs.setup.rate
    res = {"file_bytes": int(raw.size), "seconds": secs, "kbps": raw.size * 8 / secs / 1e3, "packets": int(len(vs.pkt_len)),
           "pages": int(len(vs.pages.offset)), "host_parse_ms_median": float(np.median(host)),
           "decode_ms_median": med["total"], **{f"{k}_ms": med[k] for k in names}}
    if a.dataset:
        import musicgan_amd
        from musicgan_amd.audio import wavio
        root = tempfile.mkdtemp()
        try:
            for sub in ("wav", "ogg"):
                os.makedirs(os.path.join(root, sub))
            for i in range(a.dataset):
                p = os.path.join(root, "ogg", f"f{i}.ogg")
                write(p, 60, seed=i + 1)
                pcm, sr = wavio.load_pcm(p)
                wavio.save(os.path.join(root, "wav", f"f{i}.wav"), torch.from_numpy(np.ascontiguousarray(pcm.T)), sr)
            for sub in ("wav", "ogg", "wav", "ogg"):
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
