"""Routing census: which `musicgan_amd.ops` kernels a piece of host code launches, at which shapes and with which flags.

The engine, the layers, the discriminator and the train step all launch kernels as `ops.<name>(...)`, so replacing the module's
attributes sees every call.  `census()` wraps every public function of `musicgan_amd.ops` (and the launches of
`ops.WgradDefer.flush` / `ops.SmallNet.run`) with `monkeypatch.setattr` for the duration of the `with` block and yields a
`Census`; each call is recorded as

    (op name, ((argument, value), ...))

with the arguments as bound to the function's signature (defaults left out): a tensor by its shape -- prefixed with "u8" for the
uint8 tile masks --, a `WgradDefer` as "defer", other objects by their type name, numbers and flags as they are.  Records are
hashable and survive a JSON round trip as lists (`normalise`); `spec` writes one as a line of text and `parse` reads it back, so
a test can commit the records it covers and compare.

`Census.post` (optional) is called as post(name, record, result) after each wrapped call returns and its return value replaces
the call's result: a test may change the values a launch produced (never the addressing) to check that a comparison downstream
notices.

Graph capture replays launches the census does not see: run under it with MG_GRAPHS=0 (or make at most two calls per update
shape -- the stepper captures from the third)."""
from __future__ import annotations

import contextlib
import functools
import inspect

import torch

# the host-side queries (`*_supported`, `packed_floats`, ...) are wrapped and recorded as well: tests simply do not ask for them
LAUNCHES_OF_CLASSES = (("WgradDefer", "flush"), ("SmallNet", "run"))


def describe(v):
    """The census value of one argument."""
    if isinstance(v, torch.Tensor):
        shape = tuple(int(s) for s in v.shape)
        return ("u8",) + shape if v.dtype == torch.uint8 else shape
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return round(v, 6)
    return type(v).__name__


def normalise(rec):
    """A record as read back from JSON (lists) -> the hashable tuple form."""
    def tup(v):
        return tuple(tup(u) for u in v) if isinstance(v, (list, tuple)) else v
    name, args = rec
    return (name, tuple((k, tup(v)) for k, v in args))


def _fmt(v):
    if isinstance(v, tuple):
        if v and v[0] == "u8":
            return "u8[" + ",".join(str(d) for d in v[1:]) + "]"
        return "[" + ",".join(str(d) for d in v) + "]"
    return repr(v)


def _unfmt(s: str):
    if s.startswith("u8["):
        return ("u8",) + tuple(int(d) for d in s[3:-1].split(",") if d)
    if s.startswith("["):
        return tuple(int(d) for d in s[1:-1].split(",") if d)
    if s in ("None", "True", "False"):
        return {"None": None, "True": True, "False": False}[s]
    if s.startswith("'"):
        return s[1:-1]
    return float(s) if ("." in s or "e" in s) else int(s)


def spec(rec) -> str:
    """'conv3x3 x=[192,48,128,128] bias=[64] cout=64 lrelu=True ...': a record as one line (shapes in brackets, u8[...] for masks)."""
    name, args = rec
    return " ".join([name] + [f"{k}={_fmt(v)}" for k, v in args])


def parse(line: str):
    name, *kv = line.split()
    return (name, tuple((k, _unfmt(v)) for k, v in (t.split("=", 1) for t in kv)))


class Census:
    def __init__(self):
        self.calls = []   # every record, in call order
        self.post = None

    def record(self, name, fn, args, kwargs):
        try:
            bound = inspect.signature(fn).bind(*args, **kwargs)
        except TypeError:
            return (name, (("args", tuple(describe(a) for a in args)),) + tuple((k, describe(v)) for k, v in sorted(kwargs.items())))
        rec = []
        for k, v in bound.arguments.items():
            if k == "self":
                continue
            rec.append((k, describe(v)))
        return (name, tuple(rec))

    @property
    def distinct(self):
        """The distinct records, in order of first appearance."""
        return list(dict.fromkeys(self.calls))

    def ops(self):
        return {name for name, _ in self.calls}

    def of(self, *names):
        return [r for r in self.distinct if r[0] in names]


def args_of(rec) -> dict:
    return dict(rec[1])


@contextlib.contextmanager
def census():
    import pytest
    from musicgan_amd import ops
    c = Census()

    def wrap(name, fn):
        @functools.wraps(fn)
        def inner(*args, **kwargs):
            rec = c.record(name, fn, args, kwargs)
            c.calls.append(rec)
            out = fn(*args, **kwargs)
            return c.post(name, rec, out) if c.post is not None else out
        return inner

    with pytest.MonkeyPatch.context() as mp:
        for name, fn in list(vars(ops).items()):
            if not name.startswith("_") and inspect.isfunction(fn) and fn.__module__ == ops.__name__:
                mp.setattr(ops, name, wrap(name, fn))
        for cls, meth in LAUNCHES_OF_CLASSES:
            klass = getattr(ops, cls)
            mp.setattr(klass, meth, wrap(f"{cls}.{meth}", getattr(klass, meth)))
        yield c
