"""Times the kernels of the perceptual path length (csrc/ppl.hip) through musicgan_amd.ppl_ops: slerp_pairs and rows_sqdist at
8192 x 128 (the latents of rand_channels = 32) and 8192 x 512 (the rows of level 7).  Each next to the same definition in torch
operators on the same device, alternating (float64 `acos` / `sin` slerp without the straight-line and antipodal branches, and `(a.double()
- b.double()).pow(2).sum(1)`: not the code under test; their sums run in an order that is not fixed), with the largest difference
between the two, and next to the bytes the launch has to move at 8 TB/s.  Then the whole `path_length` at level 7 on a freshly
initialised generator against the same generator calls alone, and `ppl_mean` of a seeded level-5 generator at epsilon = 1e-3, 1e-4
and 1e-5 (the floor under which the float32 rounding of the images drowns the step) next to its spread over two seeds at 1e-3.
   python tools/bench_ppl.py [--iters 10] [--pairs 8192] [--sweep-pairs 2048] [--out profiles/ppl_kernels.txt]"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bench_prdc import alternating, fmt  # noqa: E402  (tools/ is on the path when this file is run)

HBM = 8e12   # bytes/s
CALLS = 20   # launches per timed window: one launch is a few microseconds


def torch_slerp(z0, z1, t, eps):
    """the yardstick: the sine weights in float64 operators (no straight line, no flag)"""
    a, b = z0.double(), z1.double()
    omega = torch.acos(((a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).clamp(-1.0, 1.0))
    s = torch.sin(omega)
    out = []
    for u in (t, t + eps):
        out.append(((torch.sin((1.0 - u) * omega) / s)[:, None] * a + (torch.sin(u * omega) / s)[:, None] * b).float())
    return out


def torch_sqdist(a, b, scale):
    return (a.double() - b.double()).pow(2).sum(1) * scale


def times(fn, calls=CALLS):
    def run():
        for _ in range(calls):
            fn()
    return run


def per_call(t, calls=CALLS):
    return tuple(v / calls for v in t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=8192)
    ap.add_argument("--sweep-pairs", dest="sweep_pairs", type=int, default=2048)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppl needs the GPU: a CPU run says nothing about these kernels"
    from musicgan_amd import path_length, ppl_ops
    from musicgan_amd.networks import Generator
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    props = torch.cuda.get_device_properties(0)
    say(f"device: {props.name}, {props.multi_processor_count} CUs; HIP events around {CALLS} calls, {a.iters} windows alternating with "
        f"the torch form after 2 warm-up windows: per call, median [min .. max] ms")
    gen = torch.Generator(device=dev).manual_seed(0)
    n, eps = 8192, 1e-4
    for d in (128, 512):
        z0, z1 = torch.randn(n, d, device=dev, generator=gen), torch.randn(n, d, device=dev, generator=gen)
        t = torch.rand(n, dtype=torch.float64, device=dev, generator=gen)
        za, zb, flag = ppl_ops.slerp_pairs(z0, z1, t, eps)
        ta, tb = torch_slerp(z0, z1, t, eps)
        diff = max(float((za - ta).abs().max()), float((zb - tb).abs().max()))
        to, tt = alternating(times(lambda: ppl_ops.slerp_pairs(z0, z1, t, eps)), times(lambda: torch_slerp(z0, z1, t, eps)), a.iters)
        to, tt = per_call(to), per_call(tt)
        nbytes = 4 * n * d * 4 + n * 12
        say(f"--- slerp_pairs {n} x {d}: {nbytes / 1e6:.1f} MB = {nbytes / HBM * 1e3:.4f} ms at 8 TB/s; {int(flag.sum())} pairs flagged; "
            f"largest difference from the torch form {diff:.2e}")
        say("ppl_ops.slerp_pairs (1 launch)".ljust(38) + fmt(to) + f"   {nbytes / HBM * 1e3 / to[0] * 100:.1f} % of the byte floor")
        say("torch (float64 acos / sin)".ljust(38) + fmt(tt) + f"   slerp_pairs / torch = {to[0] / tt[0]:.3f}")
        scale = 1.0 / (d * eps * eps)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        want = torch_sqdist(za, zb, scale)
        diff = float(((ppl_ops.rows_sqdist(za, zb, scale) - want).abs() / want).max())
        to, tt = alternating(times(lambda: ppl_ops.rows_sqdist(za, zb, scale, out)), times(lambda: torch_sqdist(za, zb, scale)), a.iters)
        to, tt = per_call(to), per_call(tt)
        nbytes = 2 * n * d * 4 + n * 8
        say(f"--- rows_sqdist {n} x {d}: {nbytes / 1e6:.1f} MB = {nbytes / HBM * 1e3:.4f} ms at 8 TB/s; largest relative difference from "
            f"the torch form {diff:.2e}")
        say("ppl_ops.rows_sqdist (1 launch)".ljust(38) + fmt(to) + f"   {nbytes / HBM * 1e3 / to[0] * 100:.1f} % of the byte floor")
        say("torch (float64 operators)".ljust(38) + fmt(tt) + f"   rows_sqdist / torch = {to[0] / tt[0]:.3f}")

    def quiet(**kw):
        with contextlib.redirect_stdout(io.StringIO()):
            return path_length(**kw)

    with tempfile.TemporaryDirectory() as tmp:
        # the whole driver at level 7 against its generator calls alone
        torch.manual_seed(0)
        ck7 = os.path.join(tmp, "gen7.pt")
        g7 = Generator(32, end_layer=7)
        torch.save(g7.state_dict(), ck7)
        g7 = g7.to(dev).eval()
        quiet(gen_dict_state=ck7, rand_channels=32, level=7, nb_pairs=16)   # warm-up: every shape of the timed run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = quiet(gen_dict_state=ck7, rand_channels=32, level=7, nb_pairs=a.pairs)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
        z = torch.randn(16, 32, 2, 2, device=dev, generator=gen)
        calls = 2 * ((a.pairs + 7) // 8)
        with torch.no_grad():
            g7(z, 1.0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                g7(z, 1.0)
            torch.cuda.synchronize()
        forwards = time.perf_counter() - t0
        say(f"--- path_length at level 7, rand_channels 32, {a.pairs} pairs ({4 * a.pairs} images of 512 x 512 in {calls} generator calls "
            f"of 16), host clock around the call ending in a synchronise, one run after a warm-up run of 16 pairs: {result}")
        say("path_length (load, draws, rows, keys)".ljust(38) + f"{whole:9.3f} s")
        say("the generator calls alone".ljust(38) + f"{forwards:9.3f} s   path_length / forwards = {whole / forwards:.3f}")
        # the epsilon floor: ppl_mean of one seeded generator at level 5
        torch.manual_seed(1)
        ck5 = os.path.join(tmp, "gen5.pt")
        torch.save(Generator(32, end_layer=5).state_dict(), ck5)
        say(f"--- the epsilon floor: ppl_mean (ppl) of a freshly initialised generator at level 5 (torch.manual_seed(1), rand_channels "
            f"32), {a.sweep_pairs} pairs, full sampling")
        means = {}
        for e, seed in ((1e-3, 0), (1e-3, 1), (1e-4, 0), (1e-4, 1), (1e-5, 0), (1e-5, 1)):
            r = quiet(gen_dict_state=ck5, rand_channels=32, level=5, nb_pairs=a.sweep_pairs, epsilon=e, seed=seed)
            means[(e, seed)] = r["ppl_mean"]
            say(f"epsilon {e:g}, seed {seed}: ppl_mean {r['ppl_mean']:.6f}  ppl {r['ppl']:.6f}  ppl_chord {r['ppl_chord']:.6f}  "
                f"ppl_ratio {r['ppl_ratio']:.4f}  pairs {r['ppl_pairs']}")
        spread = abs(means[(1e-3, 0)] - means[(1e-3, 1)])
        for e in (1e-4, 1e-5):
            gap = abs(means[(e, 0)] - means[(1e-3, 0)])
            say(f"|ppl_mean(eps = {e:g}) - ppl_mean(eps = 1e-3)| at seed 0 = {gap:.6f}; the spread between seeds 0 and 1 at 1e-3 = "
                f"{spread:.6f}: {'within' if gap <= spread else 'MORE than'} the spread")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
