"""The per-launch fixed cost of the wave-per-tile-block Winograd kernels (csrc/wino_strip.hip, csrc/wino_ups.hip): what a launch spends
before its first MFMA -- the filter bank's way into LDS, the first block's rows -- next to the dispatch itself.  The same op is timed at
N and at 2N images (HIP events around 200 back-to-back launches behind 30 warm ones); the part that does not double is
    fixed = 2 T(N) - T(2N).
Three repeats per shape: median and spread (max - min) of the fixed part, us.   python tools/bench_conv_fixed_cost.py [label]"""
import math, os, statistics, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the planner shim: which kernel takes a call
import numpy as np
import torch
import wino_plan_shim as shim
from musicgan_amd import ops

LABEL = sys.argv[1] if len(sys.argv) > 1 else "run"
WARM, TIMED, REPEATS = 30, 200, 3
dev = torch.device("cuda", 0)
g = torch.Generator(device=dev).manual_seed(3)
R = lambda *s: torch.randn(*s, device=dev, generator=g)
plan_lib = shim.load(tempfile.mkdtemp(prefix="wino_plan_"))
N_CU = torch.cuda.get_device_properties(0).multi_processor_count
F = shim.FLAGS


def timeit(fn):
    for _ in range(WARM): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(TIMED): fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / TIMED * 1e3


def route(n, ci, co, h, w, flags, bias, y=1):
    p = shim.plan(plan_lib, np.array([(n, ci, co, h, w, flags, bias, y)]), N_CU, 1, shim.switches(plan_lib))
    return "strip" if p.strip[0] else "staged"


def conv(ci, co, hw, kind):
    """n -> (launch, kernel) of one conv3x3 call of `kind` on n images"""
    def make(n):
        wt, b = R(co, ci, 3, 3) / math.sqrt(9 * ci), R(co)
        x = R(n, ci, hw, hw)
        if kind == "plain":
            up = ops.pack_wino3x3(wt, dgrad=False)
            return (lambda: ops.conv3x3(x, None, b, co, lrelu=True, wino=up)), route(n, ci, co, hw, hw, F["LRELU"], 1)
        if kind == "lrelu+pixnorm":
            up = ops.pack_wino3x3(wt, dgrad=False)
            return (lambda: ops.conv3x3(x, None, b, co, lrelu=True, pixnorm=True, want_y=False, wino=up)), \
                route(n, ci, co, hw, hw, F["LRELU"] | F["PIXNORM"], 1, 0)
        if kind == "lrelu+pool+mask_out":
            up = ops.pack_wino3x3(wt, dgrad=False)
            return (lambda: ops.conv3x3(x, None, b, co, lrelu=True, pool=True, wino=up, mask_out=True)), \
                route(n, ci, co, hw, hw, F["LRELU"] | F["POOL_OUT"] | F["MASK_OUT"], 1)
        assert kind == "unpool_mask"  # the data gradient co <- ci of the layer, spread over the map of twice the size
        upd = ops.pack_wino3x3(R(ci, co, 3, 3) / math.sqrt(9 * ci), dgrad=True)
        m = torch.randint(0, 16, (n, co, hw, hw), device=dev, generator=g, dtype=torch.uint8)
        return (lambda: ops.conv3x3(x, None, None, co, wino=upd, unpool_mask=m)), route(n, ci, co, hw, hw, F["UNPOOL"], 0)
    return make


def winoups(ci, co, hl, dgrad):
    def make(n):
        wt, b = R(co, ci, 3, 3) / math.sqrt(9 * ci), R(co)
        assert ops.winoups3x3_supported(n, ci, co, hl, hl, dgrad=dgrad)
        if not dgrad:
            x, up = R(n, ci, hl, hl), ops.pack_winoups3x3(wt, False)
            return (lambda: ops.winoups3x3(x, up, b, co, lrelu=True, pixnorm=True, want_y=False)), "winoups"
        gy, upd = R(n, co, 2 * hl, 2 * hl), ops.pack_winoups3x3(wt, True)
        return (lambda: ops.winoups3x3_dgrad(gy, upd, ci)), "winoups"
    return make


CASES = [("conv3x3 64->64 @64 plain", conv(64, 64, 64, "plain"), 64),
         ("conv3x3 64->64 @64 lrelu+pixnorm", conv(64, 64, 64, "lrelu+pixnorm"), 64),  # (four out tiles: not a strip shape -- a control row)
         ("conv3x3 32->32 @64 lrelu+pixnorm", conv(32, 32, 64, "lrelu+pixnorm"), 64),
         ("conv3x3 64->64 @64 unpool_mask", conv(64, 64, 64, "unpool_mask"), 64),
         ("conv3x3 48->64 @128 lrelu+pool+mask_out", conv(48, 64, 128, "lrelu+pool+mask_out"), 32),
         ("conv3x3 160->160 @32 plain (one tile)", conv(160, 160, 32, "plain"), 128),
         ("winoups3x3 64->48 from 64", winoups(64, 48, 64, False), 32),
         ("winoups3x3_dgrad 64<-48 from 64", winoups(64, 48, 64, True), 32)]

print(f"# {LABEL}: us per launch at N and 2N images, fixed = 2 T(N) - T(2N); {REPEATS} repeats of {TIMED} launches behind {WARM} warm ones",
      flush=True)
print(f"# {'label':12s} {'op':42s} {'kernel':8s} {'N':>4s} {'T(N)':>8s} {'T(2N)':>8s}   fixed per repeat        median  spread", flush=True)
for name, make, n in CASES:
    (f1, k1), (f2, k2) = make(n), make(2 * n)
    assert k1 == k2, (name, k1, k2)
    t1, t2, fixed = [], [], []
    for _ in range(REPEATS):
        a, b = timeit(f1), timeit(f2)
        t1.append(a); t2.append(b); fixed.append(2 * a - b)
    reps = " ".join(f"{v:7.2f}" for v in fixed)
    print(f"{LABEL:14s} {name:42s} {k1:8s} {n:4d} {statistics.median(t1):8.2f} {statistics.median(t2):8.2f}   {reps}  {statistics.median(fixed):7.2f} "
          f"{max(fixed) - min(fixed):7.2f}", flush=True)
    del f1, f2
    torch.cuda.empty_cache()
