"""CPU, world_size 2, gloo: the data-parallel gradient exchange (musicgan_amd/dist.py) sums per-rank gradients into one
flat bucket and -- with the 1/world scale folded into Adam -- reproduces the gradient of the concatenated batch for the
whole WGAN-GP objective (all three losses are batch means; the penalty is a mean of per-sample terms)."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from musicgan_amd.dist import GradBucket, broadcast_parameters, is_distributed
    from oracle import progan as O
    assert is_distributed()

    # identical replicas from the same seed on every rank
    torch.manual_seed(21)
    gs, ds = O.GenState(8), O.DiscState(7)
    gs.next_layer()
    ds.next_layer()
    rng = torch.Generator().manual_seed(99)
    n = 4  # global batch, 2 per rank
    x_real = torch.rand(n, 2, 8, 8, generator=rng) * 2 - 1
    z = torch.randn(n, 8, 2, 2, generator=rng)
    eps = torch.rand(n, 1, 1, 1, generator=rng)
    full = O.d_step(gs, ds, x_real, z, eps, 0.3, dtype=torch.float64, detach_fake=True)
    sl = slice(rank * 2, rank * 2 + 2)
    part = O.d_step(gs, ds, x_real[sl], z[sl], eps[sl], 0.3, dtype=torch.float64, detach_fake=True)

    params = []
    for k in ds.live_keys():
        p = torch.nn.Parameter(ds.params[k].double().clone())
        p.grad = part["d_grads"][k].clone()
        params.append(p)
    bucket = GradBucket()
    assert bucket.world == world and bucket.grad_scale == 0.5
    bucket.launch(params)
    bucket.wait()
    worst = 0.0
    base = params[0].grad.untyped_storage().data_ptr()
    for p, k in zip(params, ds.live_keys()):
        assert p.grad.untyped_storage().data_ptr() == base  # views of ONE flat buffer
        got = p.grad * bucket.grad_scale
        ref = full["d_grads"][k]
        worst = max(worst, float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30)))
    # parameters whose grad is None are skipped
    extra = torch.nn.Parameter(torch.zeros(3))
    bucket.launch([extra])
    assert extra.grad is None
    m = torch.nn.Linear(2, 2)
    with torch.no_grad():
        m.weight.fill_(float(rank))
    broadcast_parameters([m], src=0)
    assert float(m.weight.abs().max()) == 0.0
    # train()'s start-up check: every rank is seen by the data path, a wrong WORLD_SIZE ends the run with a non-zero exit
    from musicgan_amd.dist import check_world
    assert check_world(world) == world
    try:
        check_world(world + 1)
        raise AssertionError("check_world accepted a missing rank")
    except SystemExit as e:
        assert "WORLD_SIZE=3 but 2 rank(s)" in str(e.code)
    torch.save({"worst": worst}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_gloo_world2_bucket_reproduces_concatenated_batch_gradient(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    for r in range(world):
        res = torch.load(os.path.join(str(tmp_path), f"r{r}.pt"))
        assert res["worst"] < 1e-10, res


def test_single_process_bucket_is_identity():
    from musicgan_amd.dist import GradBucket
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    gs = [torch.randn_like(p) for p in ps]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    b = GradBucket()
    assert b.world == 1 and b.grad_scale == 1.0
    b.launch(ps)
    b.wait()
    for p, g in zip(ps, gs):
        assert torch.equal(p.grad, g)


def test_own_flat_buffer_is_recognised_in_any_parameter_order():
    """GradBucket.flat_sink lays the buffer out in the engine's tensor order; launch() walks net.parameters().  The buffer must be
    recognised as "already flat" whenever the gradients are exactly its disjoint slices, whatever order they are listed in."""
    from musicgan_amd.dist import GradBucket
    ps = [torch.nn.Parameter(torch.zeros(3, 4)), torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 2))]
    b = GradBucket()
    flat, layout = b.flat_sink([ps[2], ps[0], ps[1]])  # engine order != registration order
    assert flat.numel() == 21
    for p in ps:
        off, n = layout[id(p)]
        p.grad = flat[off:off + n].view_as(p)
    assert b._as_own_flat(ps) is flat and b._as_own_flat(list(reversed(ps))) is flat
    assert b._as_own_flat(ps[:2]) is None  # a slice missing
    ps[1].grad = torch.zeros(5)
    assert b._as_own_flat(ps) is None      # a gradient living elsewhere


def test_train_sets_the_ipc_mode_itself_when_started_by_torchrun(tmp_path, monkeypatch):
    """`torchrun ... -m musicgan_amd train` never passes through bench.py's launcher: train() and create_dataset() set
    HSA_ENABLE_IPC_MODE_LEGACY=0 in their own process before the first HIP call when WORLD_SIZE > 1 (and leave a single-process
    run's environment alone).  Independent of whether the machine has a GPU: the first thing each does after that point --
    `torch.cuda.set_device` in train(), the side-car glob in create_dataset() (its glob of the audio files comes before) -- raises a
    sentinel here, so neither goes on to initialise HIP or a process group, and the call must end in exactly that sentinel."""
    import glob
    import types
    import pytest
    import musicgan_amd
    train_fn, create_dataset = musicgan_amd.train, musicgan_amd.create_dataset  # (the package's lazily re-exported drivers)

    class ReachedFirstDeviceUse(Exception):
        pass

    def stop(*args, **kwargs):
        raise ReachedFirstDeviceUse

    audio_glob = str(tmp_path / "*.wav")
    monkeypatch.setattr(torch.cuda, "set_device", stop)
    monkeypatch.setattr(sys.modules[create_dataset.__module__], "glob", types.SimpleNamespace(
        escape=glob.escape, glob=lambda pattern: [] if pattern == audio_glob else stop()))
    for fn in (lambda: train_fn("t", str(tmp_path), str(tmp_path / "out")),
               lambda: create_dataset(audio_glob, str(tmp_path / "ds"))):
        monkeypatch.delenv("HSA_ENABLE_IPC_MODE_LEGACY", raising=False)
        monkeypatch.setenv("WORLD_SIZE", "1")
        with pytest.raises(ReachedFirstDeviceUse):
            fn()
        assert "HSA_ENABLE_IPC_MODE_LEGACY" not in os.environ
        monkeypatch.setenv("WORLD_SIZE", "8")
        monkeypatch.setenv("RANK", "0")
        with pytest.raises(ReachedFirstDeviceUse):
            fn()
        assert os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"
