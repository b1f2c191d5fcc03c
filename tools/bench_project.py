"""The latent projector on one MI355X: what the loss launch costs, and what the data-only backward pass saves.

  loss      proj_ops.pyramid_l2 at (6, 2, 512, 512), 7 levels: loss with gradient, and the loss alone; next to the same loss and
            gradient as a chain of torch operators (x - t, avg_pool2d per level, float64 squares and means, autograd back to x) and
            next to `copy_` of one such tensor.  Alternating in one loop, HIP events around groups of launches, warm; median and
            spread of the groups.  Bytes per launch are counted from the shapes: 12 B per element (x and t read, g written) with the
            gradient, 8 B without, plus the float64 partials; the floor is those bytes at 8 TB/s.
  step      one projection step at level 7, batch 6, 32 latent channels -- engine.gen_forward(save=True), pyramid_l2,
            engine.gen_backward(need_gz=True), FusedAdam on the latent -- with engine.DataOnlySink and with a plain engine.GradSink
            (every weight gradient computed and dropped: what a frozen generator cost before), alternating in blocks; host clock
            around blocks that end in a synchronise; and the three parts of a step under HIP events.

`--out FILE` also writes the report there (profiles/project_kernels.txt is this tool's output).  A run without a GPU fails."""
import argparse
import os
import statistics
import sys
import time

HBM_BYTES_PER_S = 8e12


def _stats(v):
    v = sorted(v)
    return statistics.median(v), v[len(v) // 10], v[-1 - len(v) // 10]


def _cell(s):
    return f"{s[0]:8.2f} [{s[1]:7.2f} .. {s[2]:7.2f}]"


def _groups(torch, fns, groups, per_group):
    for fn in fns.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(groups):
        for k, fn in fns.items():   # alternating: all see the same machine
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_group):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / per_group)
    return {k: _stats(v) for k, v in times.items()}


def bench_loss(torch, dev, lines, groups, per_group):
    from musicgan_amd import proj_ops
    shape, levels = (6, 2, 512, 512), 7
    lam = proj_ops.check_weights(shape[2], shape[3])
    gen = torch.Generator(device=dev).manual_seed(1)
    x, t = torch.randn(shape, device=dev, generator=gen), torch.randn(shape, device=dev, generator=gen)
    g = torch.empty_like(x)
    xa = x.clone().requires_grad_(True)

    def chain():
        xa.grad = None
        cur, total = xa - t, 0.0
        for s in range(levels):
            if s:
                cur = torch.nn.functional.avg_pool2d(cur, 2)
            total = total + lam[s] * cur.double().square().mean(dim=(1, 2, 3))
        total.sum().backward()

    s = _groups(torch, {"copy": lambda: g.copy_(x), "grad": lambda: proj_ops.pyramid_l2(x, t, lam, out=g),
                        "loss": lambda: proj_ops.pyramid_l2(x, t, lam, need_grad=False), "chain": chain}, groups, per_group)
    n = x.numel()
    ws = proj_ops.pyramid_l2_ws_bytes(*shape, levels)
    lines.append(f"loss: {shape}, {levels} levels, us per call (median [10th .. 90th percentile] of {groups} groups of {per_group}), HIP events")
    for key, label, nbytes in (("grad", "pyramid_l2, loss and gradient (2 launches)", 12 * n + 2 * ws),
                               ("loss", "pyramid_l2, loss alone (2 launches)", 8 * n + 2 * ws),
                               ("copy", "copy_ of one tensor", 8 * n)):
        floor = nbytes / HBM_BYTES_PER_S * 1e6
        lines.append(f"  {label:<44} {_cell(s[key])}   {nbytes / 1e6:7.2f} MB   floor at 8 TB/s {floor:5.2f} us   "
                     f"{nbytes / s[key][0] / 1e6:6.2f} TB/s   {s[key][0] / floor:5.2f} x floor")
    lines.append(f"  {'torch operator chain, forward and autograd':<44} {_cell(s['chain'])}   "
                 f"{s['chain'][0] / s['grad'][0]:6.1f} x pyramid_l2")
    lines.append(f"  (workspace: {ws} bytes of float64 partials, written by the tile launch and read by the reduce launch)")


def bench_step(torch, dev, lines, blocks, per_block):
    from musicgan_amd import proj_ops
    from musicgan_amd.networks import Generator, engine
    from musicgan_amd.optim import FusedAdam
    level, batch, rc = 7, 6, 32
    torch.manual_seed(2)
    gen = Generator(rc, end_layer=level).to(dev).eval()
    for p in gen.parameters():
        p.requires_grad_(False)
    W, cache = gen._weights(), gen._pack_cache
    rng = torch.Generator(device=dev).manual_seed(3)
    tgt = torch.rand(batch, 2, 512, 512, device=dev, generator=rng) * 2 - 1
    lam = proj_ops.check_weights(512, 512)
    z = torch.randn(batch, rc, 2, 2, device=dev, generator=rng).requires_grad_(True)
    opt = FusedAdam([z], lr=0.01, betas=(0.9, 0.999))
    sinks = {"data-only": engine.DataOnlySink, "plain": engine.GradSink}

    def step(sink):
        with torch.no_grad():
            img, ctx = engine.gen_forward(W, z, 1.0, cache, save=True)
            _, g = proj_ops.pyramid_l2(img, tgt, lam)
            z.grad = engine.gen_backward(W, ctx, g, cache, sink(), need_gz=True)
            opt.step()

    def block(sink, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step(sink)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    for sink in sinks.values():
        block(sink, 5)
    times = {k: [] for k in sinks}
    for _ in range(blocks):
        for k, sink in sinks.items():
            times[k].append(block(sink, per_block))
    lines.append("")
    lines.append(f"step: level {level}, batch {batch}, {rc} latent channels, ms per step (median [min .. max] of {blocks} blocks of "
                 f"{per_block}), host clock around blocks ending in a synchronise")
    for k, v in times.items():
        lines.append(f"  {k:>10} sink: {statistics.median(v):8.3f} [{min(v):8.3f} .. {max(v):8.3f}]")
    d, p = statistics.median(times["data-only"]), statistics.median(times["plain"])
    lines.append(f"  data-only against plain: {d - p:+.3f} ms = {100 * (d - p) / p:+.1f} % (spread of the plain blocks: "
                 f"{100 * (max(times['plain']) - min(times['plain'])) / p:.2f} %)")
    # the parts of a step, each under its own pair of events (a step's launches run back to back on one stream)
    parts = {"forward": [], "loss": [], "backward data-only": [], "backward plain": [], "adam": []}
    with torch.no_grad():
        for _ in range(blocks * 2):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
            ev[0].record()
            img, ctx = engine.gen_forward(W, z, 1.0, cache, save=True)
            ev[1].record()
            _, g = proj_ops.pyramid_l2(img, tgt, lam)
            ev[2].record()
            gz = engine.gen_backward(W, ctx, g, cache, engine.DataOnlySink(), need_gz=True)
            ev[3].record()
            engine.gen_backward(W, ctx, g, cache, engine.GradSink(), need_gz=True)
            ev[4].record()
            z.grad = gz
            opt.step()
            ev[5].record()
            ev[5].synchronize()
            for name, i in zip(parts, range(5)):
                parts[name].append(ev[i].elapsed_time(ev[i + 1]))
    lines.append("  parts of a step, ms (median of %d), HIP events:" % (blocks * 2))
    for name, v in parts.items():
        lines.append(f"    {name:<20} {statistics.median(v):8.3f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--groups", type=int, default=120)
    ap.add_argument("--per-group", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--per-block", type=int, default=10)
    ap.add_argument("--skip", choices=("loss", "step"), default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_project.py measures on the GPU; none is available")
    dev = torch.device("cuda", 0)
    lines = [f"tools/bench_project.py on {torch.cuda.get_device_name(0)}", ""]
    if args.skip != "loss":
        bench_loss(torch, dev, lines, args.groups, args.per_group)
    if args.skip != "step":
        bench_step(torch, dev, lines, args.blocks, args.per_block)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
