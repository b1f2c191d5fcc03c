"""Timing and launch count of the generator's optimizer step with and without the running average of the weights
(profiles/ema_adam.txt).

    python tools/bench_ema_adam.py time OUT.txt          # HIP events: optim_gen.step() at levels 3, 5, 7; g_step replay at level 5
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_A -- python tools/bench_ema_adam.py count 0
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR_B -- python tools/bench_ema_adam.py count 0.999
    python tools/bench_ema_adam.py summary OUT.txt DIR_A DIR_B   # launches of both runs; fails unless the counts are equal
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from musicgan_amd.optim import FusedAdam  # noqa: E402
from musicgan_amd.train_step import ProGANStepper  # noqa: E402

DEV = "cuda:0"
RC = 32


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / reps   # us per call


def fmt(xs):
    return f"{statistics.median(xs):9.2f} [{min(xs):8.2f} .. {max(xs):8.2f}] us"


def optimizer(level, decay):
    gen, _ = bench.build_nets(level, RC, DEV)
    opt = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=decay)
    g = torch.Generator(device=DEV).manual_seed(1)
    for p in gen.parameters():
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
    for _ in range(20):
        opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for _ in range(20):
        graph.replay()
    torch.cuda.synchronize()
    n = sum(p.numel() for p in gen.parameters())
    return opt, graph, n, len(list(gen.parameters()))


def time_mode(out):
    lines = []
    for level in (3, 5, 7):
        a, ga, n, nt = optimizer(level, 0.0)
        b, gb, _, _ = optimizer(level, 0.999)
        eager = {0: [], 1: []}
        replay = {0: [], 1: []}
        for _ in range(9):   # alternating blocks on one box
            eager[0].append(events(a.step, 200))
            eager[1].append(events(b.step, 200))
            replay[0].append(events(ga.replay, 500))
            replay[1].append(events(gb.replay, 500))
        lines.append(f"level {level}: generator of {nt} tensors, {n} weights = {n * 4 / 1e6:.2f} MB; launches per step: "
                     f"{2 * -(-nt // 56)} plain, {2 * -(-nt // 48)} averaged (update + tick per chunk)")
        lines.append(f"  traffic: 28 B/weight = {n * 28 / 1e6:.2f} MB = {n * 28 / 8e6:.2f} us at 8 TB/s; 36 B/weight = {n * 36 / 1e6:.2f} MB = "
                     f"{n * 36 / 8e6:.2f} us")
        lines.append(f"  optim_gen.step() eager, events around 200 calls   plain {fmt(eager[0])}   averaged {fmt(eager[1])}   "
                     f"ratio {statistics.median(eager[1]) / statistics.median(eager[0]):.3f}")
        lines.append(f"  the same step as a graph replay, 500 replays      plain {fmt(replay[0])}   averaged {fmt(replay[1])}   "
                     f"ratio {statistics.median(replay[1]) / statistics.median(replay[0]):.3f}   (predicted from traffic: {36 / 28:.3f})")
        del a, b, ga, gb
    # level-5 batch-64 generator update as the stepper replays it
    steppers = []
    for decay in (0.0, 0.999):
        gen, disc = bench.build_nets(5, RC, DEV)
        og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=decay)
        od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
        st = ProGANStepper(gen, disc, og, od, RC, noise=torch.Generator(device=DEV).manual_seed(3))
        for _ in range(6):
            st.g_step(64, 0.5, DEV)
        torch.cuda.synchronize()
        assert any("graph" in e for e in st._graphs.values()), "the generator update was not captured"
        steppers.append(st)
    t = {0: [], 1: []}
    for _ in range(7):
        for i, st in enumerate(steppers):
            t[i].append(events(lambda: st.g_step(64, 0.5, DEV), 40))
    lines.append(f"level 5, batch 64, g_step (one graph replay), events around 40 calls   plain {fmt(t[0])}   averaged {fmt(t[1])}   "
                 f"difference {statistics.median(t[1]) - statistics.median(t[0]):+.2f} us")
    text = "\n".join(lines)
    print(text)
    with open(out, "w") as f:
        f.write(text + "\n")


def count_mode(decay):
    os.environ["MG_GRAPHS"] = "0"
    gen, disc = bench.build_nets(5, RC, DEV)
    og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9), ema_decay=decay)
    od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
    st = ProGANStepper(gen, disc, og, od, RC, noise=torch.Generator(device=DEV).manual_seed(3))
    for _ in range(3):
        st.g_step(64, 0.5, DEV)
    torch.cuda.synchronize()
    print("counted 3 eager generator updates at level 5, batch 64, decay", decay)


def summary_mode(out, dirs):
    import csv
    import glob
    lines = []
    totals = {}
    for tag, d in zip(("plain", "averaged"), dirs):
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        assert files, f"no kernel stats for {tag}"
        rows = list(csv.DictReader(open(files[0])))
        calls = sum(int(r["Calls"]) for r in rows)
        totals[tag] = calls
        lines.append(f"rocprofv3 --kernel-trace --stats, 3 eager generator updates at level 5, batch 64, {tag}: {calls} kernel launches, "
                     f"{len(rows)} distinct kernels")
        for r in rows:
            if "adam" in r["Name"]:
                lines.append(f"    {r['Name'][:90]:90s} calls {r['Calls']:>4s}  total {int(float(r['TotalDurationNs'])) / 1e3:9.2f} us  "
                             f"average {float(r['AverageNs']) / 1e3:7.2f} us")
    lines.append(f"launch count with averaging on {'==' if totals['plain'] == totals['averaged'] else '!='} the count with it off "
                 f"({totals['averaged']} vs {totals['plain']})")
    text = "\n".join(lines)
    print(text)
    with open(out, "w") as f:
        f.write(text + "\n")
    assert totals["plain"] == totals["averaged"]


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "time":
        time_mode(sys.argv[2])
    elif mode == "count":
        count_mode(float(sys.argv[2]))
    else:
        summary_mode(sys.argv[2], sys.argv[3:5])
