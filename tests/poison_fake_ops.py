"""A small ops module of plain torch functions on CPU tensors, for tests/test_poison_cpu.py: correct ops and ops with one planted
defect each.  The defects index, with ordinary torch views of the underlying storage, into the [guard | payload | guard] buffers
that tests/poison.py itself allocated -- a guard band is valid memory, nothing here leaves an allocation.  Outside `poisoned()`
the defective ops must not be called."""
import torch

_ws_cache = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    buf = _ws_cache.get(str(device))
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1024), dtype=torch.uint8, device=device)
        _ws_cache[str(device)] = buf
    return buf


def _at(t: torch.Tensor, index: int) -> torch.Tensor:
    """one element of t's storage, `index` elements from t[0] (negative: in front of it; numel: just past it)"""
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(t.untyped_storage(), t.storage_offset() + index, (1,), (1,))


def _mark(e: torch.Tensor) -> None:
    """four bytes that are neither 0x00 nor 0xFF nor those of the test's inputs"""
    e.view(torch.int32).fill_(0x01020304)


# ------------------------------------------------------------------ correct ops
def scale(x, a: float, out=None):
    """out = a x (`out` optional, written)"""
    out = torch.empty_like(x) if out is None else out
    torch.mul(x, a, out=out)
    return out


def add_(y, x):
    """y += x in place"""
    y.add_(x)
    return y


def pair(x):
    """(2 x, (sum x,)) through a workspace that is written before it is read"""
    ws = workspace(4 * x.numel(), x.device)[:4 * x.numel()].view(torch.float32)
    ws.copy_(x.reshape(-1))
    total = torch.zeros((1,), dtype=torch.float32, device=x.device)
    total += ws.sum()
    return scale(x, 2.0), (total,)


class Deferred:
    """as ops.WgradDefer: `later(x, out, defer=d)` only notes the job, d.flush() runs it"""

    def __init__(self):
        self._bufs, self._jobs, self._jobs_d, self._lazy = [], [], [], []

    def flush(self):
        for x, out in self._lazy:
            torch.mul(x, 3.0, out=out)
        self._lazy = []


def later(x, out, defer):
    """out = 3 x, computed by defer.flush()"""
    defer._lazy.append((x, out))


# ------------------------------------------------------------------ one planted defect each
def write_after_output(x):
    y = scale(x, 2.0)
    _mark(_at(y, y.numel()))
    return y


def write_before_output(x):
    y = scale(x, 2.0)
    _mark(_at(y, -1))
    return y


def write_input_guard(x):
    _mark(_at(x, x.numel()))
    return scale(x, 2.0)


def modify_undeclared(x):
    _mark(_at(x, 1))
    return scale(x, 2.0)


def skip_one(x):
    y = torch.empty_like(x)
    y.reshape(-1)[:-1] = 2.0 * x.reshape(-1)[:-1]
    return y


def add_onto_empty(x):
    y = torch.empty_like(x)
    y += x
    return y


def read_past_input(x):
    out = torch.zeros((1,), dtype=torch.float32, device=x.device)
    out += x.sum() + _at(x, x.numel())[0]
    return out


def read_unwritten_workspace(x):
    ws = workspace(4 * x.numel(), x.device)[:4 * x.numel()].view(torch.float32)
    return x + ws.view(x.shape)
