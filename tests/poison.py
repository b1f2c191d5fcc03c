"""Poisoned memory with guard bands: what a kernel does to memory that is not its own, and what it assumes about memory nobody
has written yet.

`poisoned(fill)` is a context manager in the style of `routing_census.census` (it is built on it and on
`pytest.MonkeyPatch.context()`; it is no conftest, adds no fixture and changes no pytest setting).  Inside it

* every tensor the package allocates with `torch.empty / empty_like / zeros / zeros_like / full` is cut from a larger uint8 buffer
  `[guard | payload | guard]`: the name `torch` (or `th`) seen by `musicgan_amd.ops` and by every other loaded `musicgan_amd`
  module is replaced by a forwarding proxy -- `torch.empty` itself stays what it is.  The front guard is GUARD (4096) bytes, the
  rear one GUARD bytes plus what rounds the payload up to 512, so the payload keeps the allocator's 512-byte alignment.  Guards
  hold the byte `fill`; so does the payload of `empty` / `empty_like` (0xFF: a quiet NaN as float32 / float64, -1 as int32, 255 as
  a mask byte); `zeros` / `full` keep their value.  CPU tensors are left alone unless `guard_cpu` (the self-test), pinned ones always;
* `_ws_cache` (and the caches of uploaded tables) of every one of those modules that has it is emptied on entry -- the package
  has one, `ops._ws_cache`, which the side modules reach through `ops.workspace`, so it is watched whichever module is wrapped --
  and before every wrapped call the payload of every live workspace buffer (those caches, and the buffers of every `WgradDefer`
  seen that holds no job waiting for its flush) is filled with `fill` again;
* every public function of the ops module, `WgradDefer.flush` and `SmallNet.run` are wrapped through the census' `pre` / `post`
  hooks.  Before the call each device tensor argument is copied into a guarded allocation of its own (arguments that overlap in
  memory share one, at their mutual offsets) and the op receives the copy.  After the call the harness synchronises, checks
  every guard of every allocation made or re-homed during the call and of every live workspace, checks that every argument not in
  `INPLACE` is bit for bit what it was, records the digest entry of the call, copies the declared in-place arguments back into
  the caller's tensors and returns the caller's own object wherever the op returned a re-homed one.  The tensors a deferred
  weight gradient points into stay re-homed until the `WgradDefer.flush` that consumes them; those of a `SmallNet` are re-homed at
  `run` (the op list's pointers are patched for the launch and restored).  Nested wrapped calls (an op calling `workspace` or
  another op) belong to the outermost one.
* the `spec` line of every wrapped call is appended to the file named by the environment variable POISON_LOG (only read here),
  flushed before the call: after a fault or a time limit the last line names the launch.

`Poison.calls` holds one entry per outermost call, in call order: (op, spec, [(buffer, bits, finite)]) for every returned tensor
("return[i]") and every declared in-place argument (by name; of `INPLACE_ROWS` the rows the call writes); `bits` is a clone (`digest="clone"`, with byte offsets in the report)
or a 64-bit sum of the words times odd multipliers (`digest="hash"`: any single changed bit changes it).  `compare(a, b)` fails
on the first entry that differs; `assert_finite(p)` on the first floating output with a NaN or an infinity (outputs of a call whose
own floating arguments were not all finite are not judged on that point).
`Poison.post(name, record, result)` (optional) may change the values a launch produced, never the addressing, before they are
recorded -- to check that the comparison notices.

A failure raises PoisonError naming the op, the spec line of the call, the buffer (argument name, return position, "workspace" or
"allocation k") and the signed byte offsets of the first and last damaged byte relative to the payload (-4: one float before it).

Nothing here needs a GPU: the harness works on CPU tensors too (tests/test_poison_cpu.py)."""
from __future__ import annotations

import contextlib
import os
import sys
import threading
import weakref

import torch

from routing_census import census, spec

GUARD = 4096
ALIGN = 512

# op -> the tensor arguments it writes, each justified by the op's docstring / code in musicgan_amd/ops.py
INPLACE = {
    "conv3x3": ("out", "pool_out"),            # "`out` (optional) receives y ... `pool_out` (optional) receives the pooled tensor"
    "conv3x3_fade": ("out",),                  # y = out if out is not None
    "conv3x3_small": ("out", "pool_out"),      # "`out` receives y (may alias mask_aux)"; p = pool_out
    "conv3x3_wgrad": ("gw", "gb"),             # "gw (+)= wgrad(x, gy); gb (+)= ..."
    "conv1x1": ("out",),                       # y = out; "accumulate: out += result"
    "conv1x1_wgrad": ("gw", "gb"),             # "gw (+)= sum gy x, gb (+)= ..."
    "winoups3x3_head": ("mp_out",),            # "written into `mp_out` if given"
    "stem_pair": ("h0", "xp", "o"),            # outputs when given; masked: "receive (w x) * lrelu'(activation) in place"
    "stem_pair_gx": ("out",),
    "head_pair": ("out",),
    "head_pair_from_mp": ("out",),
    "gen_head_bwd": ("gw", "gb"),              # "gw (2,C) (+)= sum t p, gb (2) (+)= sum t"
    "gp_apply": ("out",),
    "avgpool2_fwd": ("out",),
    "lrelu_bwd": ("out",),
    "axpby": ("out",),
    "blend_up": ("out",),
    "linear1_bwd": ("gw", "gb"),
    "gp_interp": ("out",),
    "scale_per_sample": ("out",),
    "channel_sum": ("out",),                   # "accumulate": out += sums
    "swd_gather": ("desc", "stats"),           # "rows row .. row + N P of desc ... and the per-image float64 pairs stats[...]"
    "swd_project": ("out",),
    "swd_sort_segments_": ("x",),              # "ascending in-place sort"
    "swd_distance": ("out",),
}
# (op, argument) -> the rows along dimension 0 that the call writes, where the docstring says it writes only a part
INPLACE_ROWS = {
    ("swd_gather", "desc"): lambda a: (a["row"], a["row"] + a["level"].shape[0] * a["centres"].shape[1]),   # "rows row .. row + N P"
    ("swd_gather", "stats"): lambda a: (a["row"] // a["centres"].shape[1],
                                        a["row"] // a["centres"].shape[1] + a["level"].shape[0]),          # "stats[row / P + n, c]"
}
_SN_WRITTEN = ("out", "out2")                  # the fields of an op of a SmallNet list that the launch writes
_SN_FIELDS = ("inp", "aux", "bias", "out", "out2")


class PoisonError(AssertionError):
    pass


def _bytes_of(t: torch.Tensor) -> torch.Tensor:
    """the values of `t` as a flat uint8 tensor (a copy where `t` is not contiguous)"""
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.contiguous()
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    return t.reshape(-1).view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8, device=t.device)


def hash_bits(t: torch.Tensor) -> int:
    """sum over the 64-bit words of `t` times 2 i + 1, modulo 2^64: one changed bit moves word i by +-2^k, times an odd number"""
    b = _bytes_of(t)
    n8 = b.numel() // 8 * 8
    total = b.numel()
    if n8:
        w = b[:n8].clone().view(torch.int64)
        total += int((w * (2 * torch.arange(w.numel(), device=w.device, dtype=torch.int64) + 1)).sum())
    if b.numel() > n8:
        tail = b[n8:].to(torch.int64)
        total += int((tail * (2 * torch.arange(tail.numel(), device=b.device, dtype=torch.int64) + 1)).sum()) * 0x9E3779B1
    return total & 0xFFFFFFFFFFFFFFFF


def _span(diff: torch.Tensor):
    idx = diff.nonzero().reshape(-1)
    return int(idx[0]), int(idx[-1])


class _Alloc:
    """one [guard | payload | guard] buffer"""

    def __init__(self, buf, front, size, fill, what):
        self.buf, self.front, self.size, self.fill, self.what = buf, front, size, fill, what

    def payload(self):
        return self.buf[self.front:self.front + self.size]

    def guards(self):
        return self.buf[:self.front], self.buf[self.front + self.size:]

    def damage(self):
        """None, or the signed byte offsets (first, last) of the damaged guard bytes relative to the payload"""
        lo, hi = self.guards()
        bad = []
        d = lo != self.fill
        if bool(d.any()):
            a, b = _span(d)
            bad += [a - self.front, b - self.front]
        d = hi != self.fill
        if bool(d.any()):
            a, b = _span(d)
            bad += [self.size + a, self.size + b]
        return (bad[0], bad[-1]) if bad else None


class _Proxy:
    """stands for the module `torch` in the package's modules: the allocating functions go through the harness, the rest is torch's"""

    def __init__(self, real, harness):
        self.__dict__["_real"], self.__dict__["_h"] = real, harness

    def __getattr__(self, name):
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def _shape(self, size):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        return tuple(int(s) for s in size)

    def _new(self, fn, shape, kw, value, like=None):
        dtype = kw.get("dtype") or (like.dtype if like is not None else self._real.get_default_dtype())
        device = kw.get("device")
        device = self._real.device(device) if device is not None else (like.device if like is not None else self._real.device("cpu"))
        extra = set(kw) - {"dtype", "device", "memory_format", "requires_grad", "pin_memory"}
        if (extra or kw.get("pin_memory") or kw.get("requires_grad") or not self._h.guards(device)
                or (like is not None and not like.is_contiguous())):
            return None
        return self._h.allocate(shape, dtype, device, value)

    def empty(self, *size, **kw):
        t = self._new("empty", self._shape(size), kw, None)
        return self._real.empty(*size, **kw) if t is None else t

    def zeros(self, *size, **kw):
        t = self._new("zeros", self._shape(size), kw, 0)
        return self._real.zeros(*size, **kw) if t is None else t

    def full(self, size, fill_value, **kw):
        if "dtype" not in kw or isinstance(fill_value, self._real.Tensor):
            return self._real.full(size, fill_value, **kw)
        t = self._new("full", self._shape((size,)), kw, fill_value)
        return self._real.full(size, fill_value, **kw) if t is None else t

    def empty_like(self, x, **kw):
        t = self._new("empty_like", tuple(x.shape), kw, None, like=x)
        return self._real.empty_like(x, **kw) if t is None else t

    def zeros_like(self, x, **kw):
        t = self._new("zeros_like", tuple(x.shape), kw, 0, like=x)
        return self._real.zeros_like(x, **kw) if t is None else t


class Poison:
    def __init__(self, fill, module, inplace, guard_cpu, digest, modules):
        self.fill, self.module, self.inplace, self.guard_cpu, self.digest = int(fill), module, inplace, guard_cpu, digest
        self.modules = modules
        self.calls = []          # (op, spec line, [(buffer, bits, finite)]) per outermost call
        self.launches = 0        # wrapped calls, nested ones included
        self.post = None
        self._tls = threading.local()   # per thread: the open wrapped calls; [0] is the outermost one and owns the state
        self._lock = threading.RLock()  # held from the outermost pre to its post: calls of other threads wait
        self._live = weakref.WeakSet()
        self._defers = weakref.WeakSet()
        self._pending = {}       # id(WgradDefer) -> clusters re-homed for its deferred jobs
        self._log = None
        path = os.environ.get("POISON_LOG")
        if path:
            self._log = open(path, "a")

    @property
    def _stack(self):
        if not hasattr(self._tls, "stack"):
            self._tls.stack = []
        return self._tls.stack

    # ---------------------------------------------------------------- allocations
    def guards(self, device) -> bool:
        return device.type == "cuda" or (self.guard_cpu and device.type == "cpu")

    def _buffer(self, nbytes, device, phase=0):
        """a filled [guard | payload | guard] buffer whose payload starts `phase` bytes after a 512-byte boundary"""
        front = GUARD + phase
        total = (front + nbytes + ALIGN - 1) // ALIGN * ALIGN + GUARD
        buf = torch.empty(total, dtype=torch.uint8, device=device)
        buf.fill_(self.fill)
        a = _Alloc(buf, front, nbytes, self.fill, None)
        self._live.add(a)
        if self._stack:
            self._stack[0]["allocs"].append(a)
        return a

    def allocate(self, shape, dtype, device, value):
        n = 1
        for s in shape:
            n *= s
        with torch.no_grad():
            a = self._buffer(n * torch.empty(0, dtype=dtype).element_size(), device)
            t = a.payload().view(dtype).view(shape) if n else torch.empty(shape, dtype=dtype, device=device)
            if value is not None and n:
                t.fill_(value)
        t._poison = a            # the buffer lives as long as a view of it; the record as long as this object
        return t

    def workspaces(self):
        """(label, _Alloc) of every live workspace buffer that may be poisoned now"""
        out = []
        for m in self.modules:
            for t in getattr(m, "_ws_cache", {}).values():
                if getattr(t, "_poison", None) is not None:
                    out.append(("workspace", t._poison))
        for d in list(self._defers):
            busy = bool(d._jobs or d._jobs_d or d._lazy)
            for t in d._bufs:
                if getattr(t, "_poison", None) is not None:
                    out.append(("workspace" if not busy else "workspace (deferred jobs)", t._poison))
        return out

    def check_all(self, name="<end>", line=""):
        """the guards of every allocation that is still alive"""
        for a in list(self._live):
            self._check_guard(a, name, line, a.what or "allocation")

    def _check_guard(self, a, name, line, what):
        bad = a.damage()
        if bad is not None:
            raise PoisonError(f"{name}: guard band damaged: buffer {what}, bytes {bad[0]:+d} .. {bad[1]:+d} relative to the payload "
                              f"of {a.size} bytes\n  call: {line}")

    # ---------------------------------------------------------------- arguments
    @staticmethod
    def _extent(t):
        """byte range [lo, hi) of the storage that `t` can address"""
        lo = hi = t.storage_offset()
        for s, st in zip(t.shape, t.stride()):
            if st < 0:
                raise PoisonError("negative strides are not re-homed")
            hi += (s - 1) * st
        return lo * t.element_size(), (hi + 1) * t.element_size()

    def _rehome(self, named):
        """named: [(label, tensor, written)] -> ({id(tensor): copy}, clusters); tensors that overlap share one guarded buffer"""
        items = []
        self._seq = getattr(self, "_seq", 0) + 1
        for idx, (label, t, written) in enumerate(named):
            if t.numel() == 0 or not self.guards(t.device) or t.layout != torch.strided or (t.is_cpu and t.is_pinned()):
                continue
            lo, hi = self._extent(t)
            base = t.untyped_storage().data_ptr()
            items.append([base + lo, base + hi, label, t, written, (self._seq, idx)])
        items.sort(key=lambda it: it[0])
        groups = []
        for it in items:
            if groups and it[3].device == groups[-1]["dev"] and it[0] < groups[-1]["hi"]:
                groups[-1]["hi"] = max(groups[-1]["hi"], it[1])
                groups[-1]["items"].append(it)
            else:
                groups.append({"lo": it[0], "hi": it[1], "dev": it[3].device, "items": [it]})
        mapping, clusters = {}, []
        for g in groups:
            t0 = g["items"][0][3]
            st = t0.untyped_storage()
            off = g["lo"] - st.data_ptr()
            size = g["hi"] - g["lo"]
            orig = torch.empty(0, dtype=torch.uint8, device=g["dev"]).set_(st, off, (size,), (1,))
            a = self._buffer(size, g["dev"], phase=g["lo"] % ALIGN)
            a.what = "/".join(dict.fromkeys(it[2] for it in g["items"]))
            a.payload().copy_(orig)
            members = []
            for lo, hi, label, t, written, order in g["items"]:
                start = a.front + (lo - g["lo"])
                assert start % t.element_size() == 0
                c = torch.empty(0, dtype=t.dtype, device=t.device).set_(a.buf.untyped_storage(), start // t.element_size(),
                                                                        t.shape, t.stride())
                mapping[id(t)] = c
                members.append((label, t, c, written, lo, hi, order))
            clusters.append((a, members))
        return mapping, clusters

    def _named_tensors(self, name, bound):
        written = self.inplace.get(name, ())
        out = []
        for k, v in bound.arguments.items():
            if isinstance(v, torch.Tensor):
                out.append((k, v, k in written))
        return out

    # ---------------------------------------------------------------- the hooks
    def _pre(self, name, rec, bound):
        line = spec(rec)
        if not self._stack:
            self._lock.acquire()
        self.launches += 1
        if self._log is not None:
            self._log.write(("  " * len(self._stack)) + line + "\n")
            self._log.flush()
        state = {"name": name, "line": line, "allocs": [], "clusters": [], "mapping": {}, "restore": None, "defer": None}
        self._stack.append(state)
        if len(self._stack) > 1 or bound is None:
            return
        with torch.no_grad():
            for v in bound.arguments.values():
                if all(hasattr(v, f) for f in ("_bufs", "_jobs", "_jobs_d", "_lazy", "flush")):  # a WgradDefer
                    self._defers.add(v)
                    if name.endswith(".flush"):
                        state["flushed"] = v
                    else:
                        state["defer"] = v
            for label, a in self.workspaces():
                if label == "workspace":
                    a.payload().fill_(self.fill)
            if name == "SmallNet.run":
                self._pre_smallnet(state, bound.arguments["self"])
                return
            named = self._named_tensors(name, bound)
            state["rows"] = {k: fn(bound.arguments) for (op, k), fn in INPLACE_ROWS.items() if op == name and k in bound.arguments}
            # an op whose inputs hold a NaN or an infinity (a sort of special values) may return them: no finiteness claim then
            state["finite_in"] = all(bool(torch.isfinite(t).all()) for _, t, _ in named if t.is_floating_point() or t.is_complex())
            # (pushed before re-homing so that the buffers count as made during this call)
            mapping, clusters = self._rehome(named)
            state["mapping"], state["clusters"] = mapping, clusters
            for k, v in list(bound.arguments.items()):
                if isinstance(v, torch.Tensor) and id(v) in mapping:
                    bound.arguments[k] = mapping[id(v)]

    def _pre_smallnet(self, state, net):
        """the tensors of a SmallNet op list were captured as pointers when the list was built: re-home them now, patch the list"""
        ptrs = {}
        for t in net.keep:
            ptrs.setdefault(t.data_ptr(), t)
        written = set()
        for op in net.ops:
            for f in _SN_WRITTEN:
                if getattr(op, f):
                    written.add(getattr(op, f))
        named = [(f"keep[{i}]", t, p in written) for i, (p, t) in enumerate(ptrs.items())]
        mapping, clusters = self._rehome(named)
        state["mapping"], state["clusters"] = mapping, clusters
        new_ptr = {p: mapping[id(t)].data_ptr() for p, t in ptrs.items() if id(t) in mapping}
        saved = []
        for op in net.ops:
            for f in _SN_FIELDS:
                p = getattr(op, f)
                if p in new_ptr:
                    saved.append((op, f, p))
                    setattr(op, f, new_ptr[p])
        state["restore"] = saved

    def _unwind(self, name, rec):
        state = self._stack.pop()
        for op, f, p in state["restore"] or ():
            setattr(op, f, p)
        if not self._stack:
            self._lock.release()

    def _finish_clusters(self, name, line, clusters, outputs, check_finite=True, rows=None):
        """unchanged / copy back / digest of the re-homed arguments of one call"""
        written = []
        for a, members in clusters:
            wr = [(lo, hi) for _, _, _, w, lo, hi, _ in members if w]
            for label, t, c, w, lo, hi, order in members:
                if w:
                    written.append((order, label, c))
                    continue
                if any(lo < h2 and l2 < hi for l2, h2 in wr):
                    continue   # shares memory with a declared output (`out` may alias `mask_aux`)
                d = _bytes_of(c) != _bytes_of(t)
                if bool(d.any()):
                    first, last = _span(d)
                    raise PoisonError(f"{name}: argument {label} was modified and is not declared as written: bytes {first:+d} .. "
                                      f"{last:+d} of it\n  call: {line}")
            for label, t, c, w, lo, hi, order in members:
                if w:
                    t.copy_(c)
        if outputs is not None:   # in the order of the calls and of their arguments, not of the addresses
            rows = rows or {}
            outputs += [self._entry(label, c[slice(*rows[label])] if label in rows else c, check_finite)
                        for _, label, c in sorted(written, key=lambda w: w[0])]

    def _entry(self, label, t, check_finite=True):
        t = t.detach()
        finite = bool(torch.isfinite(t).all()) if (check_finite and (t.is_floating_point() or t.is_complex())) else True
        bits = t.clone() if self.digest == "clone" else hash_bits(t)
        return (label, bits, finite)

    def _post(self, name, rec, result):
        state = self._stack.pop()
        if self._stack:
            return result
        try:
            return self._post_outermost(name, rec, result, state)
        finally:
            self._lock.release()

    def _post_outermost(self, name, rec, result, state):
        line = state["line"]
        for op, f, p in state["restore"] or ():
            setattr(op, f, p)
        with torch.no_grad():
            if torch.cuda.is_available() and torch.cuda.is_initialized():
                torch.cuda.synchronize()
            pending = []
            if state.get("flushed") is not None:
                pending = self._pending.pop(id(state.get("flushed")), [])
            # guards: what this call re-homed or allocated, what waited for this flush, every live workspace
            results = self._flat(result)
            for a, members in state["clusters"] + pending:
                self._check_guard(a, name, line, "argument " + a.what)
            for k, a in enumerate(state["allocs"]):
                if a.what is not None:
                    continue
                pos = [lab for lab, t in results if t.untyped_storage().data_ptr() == a.buf.untyped_storage().data_ptr()]
                ws = [lab for lab, w in self.workspaces() if w is a]
                self._check_guard(a, name, line, pos[0] if pos else (ws[0] if ws else f"allocation {k}"))
            for label, a in self.workspaces():
                self._check_guard(a, name, line, label)
            if self.post is not None:
                result = self.post(name, rec, result)
                results = self._flat(result)
            copies = {id(c): t for _, members in state["clusters"] for _, t, c, *_ in members}
            fin = state.get("finite_in", True)
            outputs = [self._entry(lab, t, fin) for lab, t in results if id(t) not in copies]
            if state["defer"] is not None:
                # gw / gb are complete only after the flush: keep the copies, check and digest them there
                self._pending.setdefault(id(state["defer"]), []).extend(state["clusters"])
                self._finish_clusters(name, line, state["clusters"], None)
            else:
                self._finish_clusters(name, line, state["clusters"], outputs, fin, state.get("rows"))
            if pending:
                self._finish_clusters(name, line, pending, outputs)
            self.calls.append((name, line, outputs))
            return self._map_back(result, copies)

    @staticmethod
    def _flat(result, prefix="return"):
        if isinstance(result, torch.Tensor):
            return [(prefix, result)]
        out = []
        if isinstance(result, (tuple, list)):
            for i, r in enumerate(result):
                out += Poison._flat(r, f"{prefix}[{i}]")
        return out

    @staticmethod
    def _map_back(result, copies):
        if isinstance(result, torch.Tensor):
            return copies.get(id(result), result)
        if isinstance(result, tuple):
            return tuple(Poison._map_back(r, copies) for r in result)
        if isinstance(result, list):
            return [Poison._map_back(r, copies) for r in result]
        return result

    def close(self):
        if self._log is not None:
            self._log.close()
            self._log = None


def compare(a: Poison, b: Poison, exempt=()):
    """the digests of two runs, entry by entry; ops named in `exempt` are left out (the determinism exemption)"""
    if [(n, l) for n, l, _ in a.calls] != [(n, l) for n, l, _ in b.calls]:
        for i, (x, y) in enumerate(zip(a.calls, b.calls)):
            if x[:2] != y[:2]:
                raise PoisonError(f"the two runs made different calls from call {i} on:\n  {x[1]}\n  {y[1]}")
        raise PoisonError(f"the two runs made {len(a.calls)} and {len(b.calls)} calls")
    for i, ((name, line, oa), (_, _, ob)) in enumerate(zip(a.calls, b.calls)):
        if name in exempt:
            continue
        if [o[0] for o in oa] != [o[0] for o in ob]:
            raise PoisonError(f"{name}: call {i} has outputs {[o[0] for o in oa]} under fill {a.fill:#04x} and {[o[0] for o in ob]} "
                              f"under {b.fill:#04x}\n  call: {line}")
        for (label, xa, _), (_, xb, _) in zip(oa, ob):
            if isinstance(xa, torch.Tensor):
                if xa.shape != xb.shape or xa.dtype != xb.dtype:
                    raise PoisonError(f"{name}: output {label} of call {i} differs in shape or type between the fills\n  call: {line}")
                d = _bytes_of(xa) != _bytes_of(xb)
                if bool(d.any()):
                    first, last = _span(d)
                    raise PoisonError(f"{name}: output {label} of call {i} depends on uninitialised or foreign memory: fill "
                                      f"{a.fill:#04x} and fill {b.fill:#04x} differ in bytes {first:+d} .. {last:+d} of it "
                                      f"({int(d.sum())} bytes)\n  call: {line}")
            elif xa != xb:
                raise PoisonError(f"{name}: output {label} of call {i} depends on uninitialised or foreign memory: its digest is "
                                  f"{xa:#018x} under fill {a.fill:#04x} and {xb:#018x} under {b.fill:#04x}\n  call: {line}")


def assert_finite(p: Poison, exempt=()):
    for i, (name, line, outs) in enumerate(p.calls):
        for label, _, finite in outs:
            if not finite and name not in exempt:
                raise PoisonError(f"{name}: output {label} of call {i} holds a NaN or an infinity under fill {p.fill:#04x}\n  call: {line}")


@contextlib.contextmanager
def poisoned(fill=0xFF, *, module=None, inplace=None, guard_cpu=False, digest="clone", classes=None, extra_modules=()):
    """see the module's docstring; yields the `Poison` (`.calls`, `.post`, `.census`).  `module`: the ops module (default
    `musicgan_amd.ops`); `inplace`: its table of written arguments (default INPLACE); `classes`: its (class, method) launches."""
    import pytest
    from routing_census import LAUNCHES_OF_CLASSES
    if module is None:
        from musicgan_amd import ops as module
        import musicgan_amd.optim, musicgan_amd.metrics, musicgan_amd.train_step  # noqa: F401,E401 -- the allocating modules
        import musicgan_amd.networks.engine, musicgan_amd.audio.functions, musicgan_amd.audio.wavio  # noqa: F401,E401
    root = module.__name__.split(".")[0]
    modules = [m for n, m in list(sys.modules.items())
               if m is not None and (n == root or n.startswith(root + ".") or m is module)] + list(extra_modules)
    p = Poison(fill, module, INPLACE if inplace is None else inplace, guard_cpu, digest, modules)
    proxy = _Proxy(torch, p)
    with pytest.MonkeyPatch.context() as mp:
        for m in modules:
            for attr, v in list(vars(m).items()):
                if v is torch:
                    mp.setattr(m, attr, proxy)
        for cache in ("_ws_cache", "_resample_banks", "_venc_tables"):   # built anew inside, so that both runs make the same calls
            for m in modules:
                if hasattr(m, cache):
                    mp.setattr(m, cache, {})
        with census(module, LAUNCHES_OF_CLASSES if classes is None else classes) as c:
            p.census = c

            c.pre, c.post, c.unwind = p._pre, p._post, p._unwind
            try:
                yield p
                p.check_all()
            finally:
                p.close()


def rule(case, *, digest="clone", exempt=(), **kw):
    """R: `case()` under fill 0x00 and again under 0xFF (the zero pass first); no guard damaged, no undeclared argument changed
    (both checked as the case runs), equal digests entry by entry, no NaN / Inf in an output of the 0xFF run.  Returns both runs."""
    runs = []
    for fill in (0x00, 0xFF):
        with poisoned(fill, digest=digest, **kw) as p:
            p.result = case(p)
        runs.append(p)
    compare(runs[0], runs[1], exempt=exempt)
    assert_finite(runs[1])
    return runs
