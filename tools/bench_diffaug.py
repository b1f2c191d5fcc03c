"""DiffAugment on one MI355X: what the two launches cost, and what they add to a whole update.

  kernels   mg_diffaug_fwd / mg_diffaug_bwd at (192, 2, 128, 128), (64, 2, 128, 128) and (6, 2, 512, 512) next to `copy_` of the same
            tensor (the yardstick: both read and write the same bytes), alternating in one loop, HIP events around groups of
            launches, warm; median and spread of >= 100 groups.  Under a random u (every alignment of the shifted source) and under
            p = 0 (the identity: aligned on both sides).
  updates   one critic + one generator update through ProGANStepper under graphs at level 5 batch 64 and level 7 batch 6, without
            and with augment="translation,cutout", alternating in blocks; host clock around blocks that end in a synchronise; the
            spread between blocks is the run-to-run spread a difference has to exceed.

`--tree DIR` imports musicgan_amd from DIR instead of this tool's own tree: on a tree without DiffAugment only the un-augmented update is
timed (the comparison the un-augmented path must pass: that path must not have changed).  `--out FILE` also writes the report there
(profiles/diffaug.txt is this tool's output).  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time


def _stats(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def bench_kernels(torch, aug_ops, dev, lines, groups, per_group):
    lines.append("kernels: one launch each, us (median [10th .. 90th percentile] of %d groups of %d launches), HIP events" % (groups, per_group))
    lines.append(f"{'shape':>18} {'MB':>6} {'u':>8} | {'copy_':>22} | {'diffaug_fwd':>22} {'x copy':>6} | {'diffaug_bwd':>22} {'x copy':>6}")
    gen = torch.Generator(device=dev).manual_seed(1)
    for shape in ((192, 2, 128, 128), (64, 2, 128, 128), (6, 2, 512, 512)):
        x = torch.randn(shape, device=dev, generator=gen)
        y = torch.empty_like(x)
        for label, u, p in (("random", torch.rand(shape[0], 8, device=dev, generator=gen), 1.0),
                            ("p = 0", torch.rand(shape[0], 8, device=dev, generator=gen), 0.0)):
            fns = {"copy": lambda: y.copy_(x), "fwd": lambda: aug_ops.diffaug_fwd(x, u, 3, p, out=y),
                   "bwd": lambda: aug_ops.diffaug_bwd(x, u, 3, p, out=y)}
            for fn in fns.values():
                for _ in range(50):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(groups):
                for k, fn in fns.items():   # alternating: the three see the same machine
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(per_group):
                        fn()
                    b.record()
                    b.synchronize()
                    times[k].append(a.elapsed_time(b) * 1e3 / per_group)
            s = {k: _stats(v) for k, v in times.items()}
            cell = lambda k: f"{s[k][0]:7.2f} [{s[k][1]:6.2f} .. {s[k][2]:6.2f}]"
            mb = x.numel() * 4 / 1e6
            lines.append(f"{str(shape):>18} {mb:6.1f} {label:>8} | {cell('copy')} | {cell('fwd')} {s['fwd'][0] / s['copy'][0]:6.2f} | "
                         f"{cell('bwd')} {s['bwd'][0] / s['copy'][0]:6.2f}")


def bench_updates(torch, dev, lines, blocks, per_block, have_aug):
    import bench
    from musicgan_amd.optim import FusedAdam
    from musicgan_amd.train_step import ProGANStepper
    lines.append("")
    lines.append("updates: one critic + one generator update under graphs, ms (median [min .. max] of %d blocks of %d), host clock around "
                 "blocks ending in a synchronise" % (blocks, per_block))
    for level, batch in ((5, 64), (7, 6)):
        side = bench.LEVEL_SIDE[level]
        variants = {}
        for name in ["plain"] + (["augmented"] if have_aug else []):
            gen, disc = bench.build_nets(level, 32, dev)
            og = FusedAdam(gen.parameters(), lr=1e-3, betas=(0.0, 0.9))
            od = FusedAdam(disc.parameters(), lr=1e-3, betas=(0.0, 0.9))
            noise = torch.Generator(device=dev).manual_seed(5)
            kw = {}
            if name == "augmented":
                from musicgan_amd.networks import DiffAugment
                kw["augment"] = DiffAugment("translation,cutout", 1.0)
            variants[name] = ProGANStepper(gen, disc, og, od, 32, noise=noise, **kw)
        x = torch.rand(batch, 2, side, side, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) * 2 - 1

        def block(st, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                st.d_step(x, 0.5)
                st.g_step(batch, 0.5, dev)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n
        for st in variants.values():
            block(st, 10)   # two eager calls, the capture, replays
            assert st.use_graphs and sum("graph" in e for e in st._graphs.values()) == 2, "the updates were not captured"
        times = {k: [] for k in variants}
        for _ in range(blocks):
            for k, st in variants.items():
                times[k].append(block(st, per_block))
        for k, v in times.items():
            lines.append(f"  level {level} batch {batch:3d} {k:>10}: {statistics.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]")
        if have_aug:
            p, a = statistics.median(times["plain"]), statistics.median(times["augmented"])
            lines.append(f"  level {level} batch {batch:3d}   overhead: {a - p:+.3f} ms = {100 * (a - p) / p:+.2f} % "
                         f"(spread of the plain blocks: {100 * (max(times['plain']) - min(times['plain'])) / p:.2f} %)")
        del variants
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=120)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=20)
    ap.add_argument("--skip", choices=("kernels", "updates"), default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_diffaug.py measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    try:
        from musicgan_amd import aug_ops
    except ImportError:
        aug_ops = None
    lines = [f"tools/bench_diffaug.py on {torch.cuda.get_device_name(0)}, tree: {'this one' if aug_ops is not None else 'one without DiffAugment'}", ""]
    if aug_ops is not None and args.skip != "kernels":
        bench_kernels(torch, aug_ops, dev, lines, args.groups, args.per_group)
    if args.skip != "updates":
        bench_updates(torch, dev, lines, args.blocks, args.per_block, aug_ops is not None)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
