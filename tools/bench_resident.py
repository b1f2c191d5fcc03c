"""Training from the dataset in device memory: what the windowed input transform and the resident loader cost.

  python tools/bench_resident.py [--out profiles/resident_loader.txt] [--repeats 3] [--no-train]

(1) `window_ops.input_transform_windows` on a batch of 64 windows of a resident array against `ops.input_transform` on the same
    windows laid out in memory, 512 -> 128 and 512 -> 512, at offset 0, at an odd offset (a 4-byte aligned start of every row) and at a
    multiple of four (16-byte aligned): device events around 20 calls, median and spread of 15 such timings after a warm-up.
(2) `train()` on the synthetic corpus of bench.py's `train_loop` record (two 10-minute files, 402 samples), parked at level 5 with
    that record's schedule overrides, batch 64, 200 iterations between two synchronised marks: the packed loader, `resident`, and
    `resident` + `random_offset`, alternated in this order in one process and repeated; per variant the median and the spread
    (max - min) of the repeats.  The profiler is off."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"


def event_ms(fn, calls=20, rounds=15, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), max(out) - min(out)


def kernel_rows(lines):
    from musicgan_amd import ops, window_ops
    n, rows = 64, 96
    g = torch.Generator(device=DEV).manual_seed(3)
    base = torch.rand(rows, 2, 512, 512, device=DEV, generator=g) * 2 - 1
    ra = torch.arange(n, dtype=torch.int32, device=DEV)
    rb = ra + 1
    lines.append(f"kernel: batch {n} windows out of {rows} resident samples (2, 512, 512) float32; ms per call, median (spread) of "
                 f"15 timings of 20 calls, device events")
    lines.append(f"{'side':>5} {'offset':>7} {'input_transform':>22} {'input_transform_windows':>26} {'ratio':>7} {'read GB/s':>10}")
    for side in (128, 512):
        for off in (0, 255, 256):
            of = torch.full((n,), off, dtype=torch.int32, device=DEV)
            mat = torch.cat([base[ra.long()], base[rb.long()]], -1)[..., off:off + 512].contiguous()
            assert torch.equal(window_ops.input_transform_windows(base, ra, rb, of, side), ops.input_transform(mat, side))
            old = event_ms(lambda: ops.input_transform(mat, side))
            new = event_ms(lambda: window_ops.input_transform_windows(base, ra, rb, of, side))
            gbs = 2 * n * 2 * 512 * 512 * 4 / (new[0] * 1e-3) / 1e9  # the batch is read twice (min / max, then the resize)
            lines.append(f"{side:>5} {off:>7} {old[0]:>14.4f} ({old[1]:.4f}) {new[0]:>18.4f} ({new[1]:.4f}) {new[0] / old[0]:>7.3f} "
                         f"{gbs:>10.0f}")
            del mat


def train_rows(lines, repeats):
    import importlib
    from musicgan_amd.audio import wavio
    from musicgan_amd.train import train
    create_dataset = importlib.import_module("musicgan_amd.create_dataset").create_dataset
    tmp = tempfile.mkdtemp(prefix="mg_resident_")
    try:
        wav_dir, data = os.path.join(tmp, "wav"), os.path.join(tmp, "data")
        os.mkdir(wav_dir)
        g = torch.Generator().manual_seed(7)
        for i in range(2):
            wavio.save(os.path.join(wav_dir, f"track_{i}.wav"), torch.rand(1, 44100 * 600, generator=g) - 0.5, 44100)
        create_dataset(os.path.join(wav_dir, "*.wav"), data)
        shutil.rmtree(wav_dir)
        first, last, big = 30, 230, 10 ** 9
        variants = [("PackedLoader", {}), ("resident", {"resident": True}),
                    ("resident + random_offset", {"resident": True, "random_offset": True})]
        rates = {name: [] for name, _ in variants}
        for rep in range(repeats + 1):  # (repeat 0: warm-up of every variant, not recorded)
            for name, kw in variants:
                marks = {}

                def hook(it):
                    if it in (first, last):
                        torch.cuda.synchronize()
                        marks[it] = time.perf_counter()

                devnull = open(os.devnull, "w")
                stderr, stdout, sys.stderr, sys.stdout = sys.stderr, sys.stdout, devnull, devnull
                try:
                    torch.manual_seed(11)
                    train("bench", data, os.path.join(tmp, f"out_{rep}_{len(rates[name])}_{name.replace(' ', '')}"), nb_epoch=1000,
                          batch_size=64, max_iters=last, save_every=big, rand_channels=32,
                          fadein_lengths=[1, 1, 1, 1, 1, 10 ** 7, big, big], train_lengths=[1, 1, 1, 1, 1, big, big],
                          progress_hook=hook, **kw)
                finally:
                    sys.stderr, sys.stdout = stderr, stdout
                    devnull.close()
                if rep:
                    rates[name].append((last - first) / (marks[last] - marks[first]))
        lines.append("")
        lines.append(f"train(): level 5 (2x128x128), batch 64, 200 iterations between synchronised marks, 402 samples; iterations/s, "
                     f"median of {repeats} alternated repeats after one warm-up round (spread = max - min)")
        for name, _ in variants:
            r = rates[name]
            lines.append(f"{name:>26}: {statistics.median(r):8.2f} it/s (spread {max(r) - min(r):.2f}; "
                         f"{64 * statistics.median(r):7.0f} img/s)   repeats: {' '.join(f'{v:.2f}' for v in r)}")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-train", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    lines = ["python tools/bench_resident.py " + " ".join(sys.argv[1:]), torch.cuda.get_device_name(0), ""]
    kernel_rows(lines)
    if not args.no_train:
        train_rows(lines, args.repeats)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
