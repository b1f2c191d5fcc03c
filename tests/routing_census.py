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

`Census.pre` (optional) is called as pre(name, record, bound) before the wrapped call, `bound` being the `inspect.BoundArguments`
the record was made from (None where the arguments did not bind): the hook may replace entries of `bound.arguments`, and the call
is made with what it left there.  `Census.unwind` (optional) is called as unwind(name, record) when the wrapped call raises, so a
`pre` hook that keeps state per call can drop it.  tests/poison.py re-homes every tensor argument into a guarded allocation this way.
`census(module)` wraps the public functions of another module in the same manner (the default is `musicgan_amd.ops`).

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
        self.pre = None
        self.unwind = None

    def bind(self, name, fn, args, kwargs):
        """(record, BoundArguments or None) of one call"""
        try:
            bound = inspect.signature(fn).bind(*args, **kwargs)
        except TypeError:
            return (name, (("args", tuple(describe(a) for a in args)),) + tuple((k, describe(v)) for k, v in sorted(kwargs.items()))), None
        rec = []
        for k, v in bound.arguments.items():
            if k == "self":
                continue
            rec.append((k, describe(v)))
        return (name, tuple(rec)), bound

    def record(self, name, fn, args, kwargs):
        return self.bind(name, fn, args, kwargs)[0]

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


def public_functions(module):
    """The functions `census` wraps: the public ones defined in `module` itself."""
    return [(name, fn) for name, fn in list(vars(module).items())
            if not name.startswith("_") and inspect.isfunction(fn) and fn.__module__ == module.__name__]


@contextlib.contextmanager
def census(module=None, classes=LAUNCHES_OF_CLASSES):
    import pytest
    if module is None:
        from musicgan_amd import ops as module
    c = Census()

    def wrap(name, fn):
        @functools.wraps(fn)
        def inner(*args, **kwargs):
            rec, bound = c.bind(name, fn, args, kwargs)
            c.calls.append(rec)
            if c.pre is not None:
                c.pre(name, rec, bound)
            try:
                out = fn(*bound.args, **bound.kwargs) if bound is not None else fn(*args, **kwargs)
            except BaseException:
                if c.unwind is not None:
                    c.unwind(name, rec)
                raise
            return c.post(name, rec, out) if c.post is not None else out
        return inner

    with pytest.MonkeyPatch.context() as mp:
        for name, fn in public_functions(module):
            mp.setattr(module, name, wrap(name, fn))
        for cls, meth in classes:
            klass = getattr(module, cls, None)
            if klass is not None:
                mp.setattr(klass, meth, wrap(f"{cls}.{meth}", getattr(klass, meth)))
        yield c
