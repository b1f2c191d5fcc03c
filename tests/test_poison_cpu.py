"""The poison harness (tests/poison.py) has teeth: run on a fake ops module of plain torch functions on CPU tensors
(tests/poison_fake_ops.py), every planted defect is reported with the op, the call, the buffer and the byte offsets, and every
correct counterpart passes.  No project kernel is called; no access leaves a buffer the harness allocated."""
import re

import pytest
import torch

import poison
import poison_fake_ops as fake
import poison_fake_side as side
from poison import PoisonError, assert_finite, compare, poisoned

INPLACE = {"scale": ("out",), "add_": ("y",), "later": ("out",)}
CLASSES = (("Deferred", "flush"),)
N = 6


def _x():
    return torch.arange(1.0, 1.0 + 2 * N).reshape(2, N)


def _ctx(fill, **kw):
    return poisoned(fill, module=fake, inplace=INPLACE, guard_cpu=True, classes=CLASSES, **kw)


def _both(fn):
    runs = []
    for fill in (0x00, 0xFF):
        with _ctx(fill) as p:
            p.result = fn()
        runs.append(p)
    return runs


def _off(v):
    return re.escape(f"{v:+d}")


def _fails(fn, *needles):
    with pytest.raises(PoisonError) as e:
        fn()
    msg = str(e.value)
    for n in needles:
        assert re.search(n, msg), f"{n!r} not in the report:\n{msg}"
    return msg


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("op, buffer, first, last", [
    ("write_after_output", "return", 4 * 2 * N, 4 * 2 * N + 3),
    ("write_before_output", "return", -4, -1),
    ("write_input_guard", "argument x", 4 * 2 * N, 4 * 2 * N + 3),
])
def test_a_write_into_a_guard_is_reported(op, buffer, first, last, fill):
    def run():
        with _ctx(fill):
            getattr(fake, op)(_x())
    _fails(run, rf"^{op}: guard band damaged", rf"buffer {buffer}, bytes {_off(first)} \.\. {_off(last)} relative",
           rf"call: {op} x=\[2,{N}\]")


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_an_undeclared_write_to_an_argument_is_reported(fill):
    x = _x()

    def run():
        with _ctx(fill):
            fake.modify_undeclared(x)
    _fails(run, r"^modify_undeclared: argument x was modified and is not declared as written: bytes \+4 \.\. \+7",
           rf"call: modify_undeclared x=\[2,{N}\]")
    assert torch.equal(x, _x())  # the caller's tensor never saw it


@pytest.mark.parametrize("op, first, last", [
    ("skip_one", 4 * (2 * N - 1), 4 * 2 * N - 1),
    ("add_onto_empty", 0, 4 * 2 * N - 1),
    ("read_past_input", 0, 3),
    ("read_unwritten_workspace", 0, 4 * 2 * N - 1),
])
def test_a_dependence_on_memory_nobody_wrote_is_reported(op, first, last):
    a, b = _both(lambda: getattr(fake, op)(_x()))
    _fails(lambda: compare(a, b), rf"^{op}: output return of call 0 depends on uninitialised or foreign memory",
           rf"bytes {_off(first)} \.\. {_off(last)} of it", rf"call: {op} x=\[2,{N}\]")
    _fails(lambda: assert_finite(b), rf"^{op}: output return of call 0 holds a NaN or an infinity under fill 0xff")
    assert_finite(a)


def test_the_hashed_digest_reports_it_too():
    runs = []
    for fill in (0x00, 0xFF):
        with _ctx(fill, digest="hash") as p:
            fake.skip_one(_x())
        runs.append(p)
    _fails(lambda: compare(*runs), r"^skip_one: output return of call 0 depends on uninitialised or foreign memory: its digest is")


def test_one_changed_bit_changes_the_hash():
    g = torch.Generator().manual_seed(3)
    for n in (1, 7, 8, 1031):
        t = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
        h = poison.hash_bits(t)
        for byte in {0, n // 2, n - 1}:
            for bit in (0, 7):
                u = t.clone()
                u[byte] ^= 1 << bit
                assert poison.hash_bits(u) != h
    x = torch.randn(5, 3)
    assert poison.hash_bits(x) == poison.hash_bits(x.clone()) != poison.hash_bits(-x)


def _correct_case():
    x, o, y = _x(), torch.full((2, N), float("nan")), _x()
    r1 = fake.scale(x, 2.0)
    r2 = fake.scale(x, 3.0, out=o)
    r3 = fake.add_(y, x)
    r4, (tot,) = fake.pair(x)
    return x, o, y, r1, r2, r3, r4, tot


def test_correct_ops_pass_with_equal_digests_and_the_callers_objects():
    a, b = _both(_correct_case)
    compare(a, b)
    assert_finite(b)
    assert [c[0] for c in b.calls] == ["scale", "scale", "add_", "pair"]  # workspace / scale inside pair belong to pair
    assert [[o[0] for o in c[2]] for c in b.calls] == [["return"], ["out"], ["y"], ["return[0]", "return[1][0]"]]
    for run in (a, b):
        x, o, y, r1, r2, r3, r4, tot = run.result
        assert r2 is o and r3 is y                      # the caller's objects, with the values written back
        assert torch.equal(x, _x()) and torch.equal(r1, 2 * _x()) and torch.equal(o, 3 * _x()) and torch.equal(y, 2 * _x())
        assert torch.equal(r4, 2 * _x()) and float(tot) == float(_x().sum())
        assert run.launches == 6                        # 4 outermost + workspace and scale inside pair
    # allocations keep the allocator's alignment and carry a guard of at least 4096 bytes on either side
    al = b.result[3]._poison
    assert al.front == poison.GUARD and al.front % 512 == 0 and al.buf.numel() - al.front - al.size >= poison.GUARD
    assert (al.buf.data_ptr() + al.front) % 64 == al.buf.data_ptr() % 64


def test_overlapping_and_strided_arguments_are_rehomed_together():
    with _ctx(0xFF) as p:
        base = torch.arange(24.0).reshape(4, 6)
        y = base[:, :3]                       # not contiguous
        r = fake.add_(y, base[:, 3:])         # interleaved with its other operand in memory
        assert r is y
        z = torch.arange(6.0)
        assert fake.scale(z, 2.0, out=z) is z  # out aliases x exactly
    want = torch.arange(24.0).reshape(4, 6)
    want[:, :3] += want[:, 3:]
    assert torch.equal(base, want) and torch.equal(z, 2 * torch.arange(6.0))
    assert_finite(p)


def test_deferred_jobs_keep_their_rehomed_tensors_until_the_flush():
    def case():
        d = fake.Deferred()
        x, out = _x(), torch.full((2, N), float("nan"))
        fake.later(x, out, defer=d)
        fake.scale(x, 2.0)                    # a call between add and flush
        assert bool(torch.isnan(out).all())   # not valid before the flush
        d.flush()
        return out
    a, b = _both(case)
    compare(a, b)
    assert torch.equal(b.result, 3 * _x())
    assert [c[0] for c in b.calls] == ["later", "scale", "Deferred.flush"] and [o[0] for o in b.calls[2][2]] == ["out"]


def test_workspace_is_poisoned_again_before_every_call():
    with _ctx(0xFF) as p:
        fake.pair(_x())                                        # leaves finite floats in the workspace
        got = fake.read_unwritten_workspace(_x())              # must not see them
    assert bool(torch.isnan(got).all())
    _fails(lambda: assert_finite(p), r"^read_unwritten_workspace: output return of call 1")


def _side_ctx(fill):
    return poisoned(fill, module=side, inplace={}, guard_cpu=True, classes=(), extra_modules=(fake,))


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_a_workspace_borrowed_from_another_module_is_watched(fill):
    """the wrapped module owns no cache: its scratch memory is the `_ws_cache` buffer of a module that is only patched
    (`extra_modules`), as `pv_ops` and its siblings borrow `ops.workspace`.  That buffer is emptied on entry, filled again before every
    wrapped call, and its guards are checked after every wrapped call."""
    x = torch.arange(1.0, 17.0)
    fake.workspace(64, x.device)                               # a buffer from before: must not be seen inside
    with _side_ctx(fill) as p:
        assert fake._ws_cache == {}
        assert float(side.total(x)) == float(x.sum())          # leaves finite floats in the shared buffer
        (buf,) = fake._ws_cache.values()
        assert [label for label, _ in p.workspaces()] == ["workspace"] and p.workspaces()[0][1] is buf._poison
        assert bool((buf[:64] != fill).any())
        got = side.read_unwritten_workspace(x)                 # must not see them
        assert bool((buf == fill).all()) and next(iter(fake._ws_cache.values())) is buf
    assert bool(torch.isnan(got).all()) if fill == 0xFF else torch.equal(got, x)
    assert len(fake._ws_cache) == 1 and not hasattr(next(iter(fake._ws_cache.values())), "_poison")   # the one from before
    fake._ws_cache.clear()


@pytest.mark.parametrize("reused", [False, True])
def test_a_write_past_a_borrowed_workspace_is_reported(reused):
    x = torch.arange(1.0, 17.0)

    def run():
        with _side_ctx(0xFF):
            if reused:
                side.total(x)                                  # the buffer is then older than the call that damages it
            side.write_past_workspace(x)
    _fails(run, r"^write_past_workspace: guard band damaged", rf"buffer workspace, bytes {_off(1024)} \.\. {_off(1027)} relative",
           r"call: write_past_workspace x=\[16\]")
    assert fake._ws_cache == {}


def test_the_post_hook_changes_values_and_the_comparison_names_the_call():
    def flip(name, rec, result):
        if name == "scale":
            result.view(torch.int32).reshape(-1)[2] ^= 1
        return result
    runs = []
    for fill in (0x00, 0xFF):
        with _ctx(fill) as p:
            p.post = flip if fill == 0xFF else None
            fake.add_(_x(), _x())
            fake.scale(_x(), 2.0)
        runs.append(p)
    _fails(lambda: compare(*runs), r"^scale: output return of call 1 .* bytes \+8 \.\. \+8 of it \(1 bytes\)", r"call: scale x=")


def test_a_raising_op_leaves_the_harness_usable_and_torch_untouched(tmp_path, monkeypatch):
    empty, zeros = torch.empty, torch.zeros
    log = tmp_path / "poison.log"
    monkeypatch.setenv("POISON_LOG", str(log))
    with _ctx(0xFF) as p:
        assert fake.torch is not torch and fake.torch.float32 is torch.float32
        with pytest.raises(RuntimeError):
            fake.scale(_x(), 2.0, out=torch.empty(3, dtype=torch.int64).reshape(3, 1, 1)[:, 0])  # mul into a wrong shape / type
        assert torch.equal(fake.scale(_x(), 2.0), 2 * _x())
        assert fake.torch.empty(3, pin_memory=False).shape == (3,)
    assert fake.torch is torch and torch.empty is empty and torch.zeros is zeros and fake._ws_cache == {}
    assert not hasattr(torch.empty(2), "_poison")
    lines = log.read_text().splitlines()
    assert lines[0].startswith("scale x=[2,6] a=2.0 out=") and lines[-1] == "scale x=[2,6] a=2.0" and len(p.calls) == 1
