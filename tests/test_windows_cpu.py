"""Host side of training on shifted windows (audio/dataset.py, create_dataset._finish_sidecar, the CLI): the tracks in the side-car,
the successor table, the epoch's offsets, the windowed host gather, the memory rule of the resident array.  No GPU."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

from musicgan_amd.audio import dataset as ds

SHAPE = (2, 4, 16)  # a small sample shape, patched in for (2, 512, 512)
N = 12              # so that magn_phase_10.pt sorts in front of magn_phase_2.pt
TRACKS = [[0, 5], [5, 1], [6, 6]]
NAMES = sorted(f"magn_phase_{i}.pt" for i in range(N))
# string order: 0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9 (position -> idx); successors by hand, as positions in that order:
#   idx 0 -> idx 1 (pos 1); idx 1 -> idx 2 (pos 4); idx 10 -> idx 11 (pos 3); idx 11: last of [6, 12); idx 2 -> 3 (pos 5);
#   idx 3 -> 4 (pos 6); idx 4: last of [0, 5); idx 5: a track of one chunk; idx 6 -> 7 (pos 9); 7 -> 8 (pos 10); 8 -> 9 (pos 11);
#   idx 9 -> idx 10 (pos 2)
SUCC = [1, 4, 3, -1, 5, 6, -1, -1, 9, 10, 11, 2]


def _cd():
    return importlib.import_module("musicgan_amd.create_dataset")  # (the package attribute of that name is the function)


def _write(folder, monkeypatch, tracks="default", n=N):
    """n samples in write order (idx 0, 1, ...) as .pt files and as the streamed shard files, then _finish_sidecar"""
    monkeypatch.setattr(ds, "_SAMPLE_SHAPE", SHAPE)
    rng = torch.Generator().manual_seed(1)
    samples = [torch.rand(*SHAPE, generator=rng) * 2 - 1 for _ in range(n)]
    for i, x in enumerate(samples):
        torch.save(x.double(), os.path.join(folder, f"magn_phase_{i}.pt"))
    fds = [open(os.path.join(folder, ds.shard_name(k, ds.PACKED_SHARDS) + ".tmp"), "wb") for k in range(ds.PACKED_SHARDS)]
    for r, x in enumerate(samples):
        k, local = ds.shard_of_row(r, ds.PACKED_SHARDS, ds.PACKED_BLOCK_ROWS)
        fds[k].seek(local * x.numel() * 4)
        fds[k].write(x.numpy().tobytes())
    for fh in fds:
        fh.close()
    names = [f"magn_phase_{i}.pt" for i in range(n)]
    if tracks == "default":
        _cd()._finish_sidecar(folder, names, tracks=TRACKS)
    elif tracks is None:
        _cd()._finish_sidecar(folder, names)
    else:
        _cd()._finish_sidecar(folder, names, tracks=tracks)
    return samples


def test_sidecar_records_tracks_and_successors_follow_string_order(tmp_path, monkeypatch):
    folder = str(tmp_path)
    _write(folder, monkeypatch)
    assert ds.has_packed(folder)
    meta = json.load(open(os.path.join(folder, ds.PACKED_META)))
    assert meta["tracks"] == TRACKS and meta["files"] == NAMES and NAMES[2] == "magn_phase_10.pt"
    succ = ds.PackedAudioDataset(folder).successors()
    assert succ.dtype == np.int32 and succ.tolist() == SUCC


def test_two_argument_call_writes_no_tracks(tmp_path, monkeypatch):
    folder = str(tmp_path)
    _write(folder, monkeypatch, tracks=None)
    meta = json.load(open(os.path.join(folder, ds.PACKED_META)))
    assert "tracks" not in meta and ds.has_packed(folder)
    assert ds.PackedAudioDataset(folder).successors() is None


@pytest.mark.parametrize("tracks", [[[0, 5], [6, 6]],            # a gap: idx 5 in no track
                                    [[0, 6], [5, 1], [6, 6]],    # an overlap at idx 5
                                    [[0, 5], [5, 1], [6, 7]],    # past the end
                                    [[0, 5], [5, 1], [6, 5]]])   # short of the end
def test_malformed_tracks_count_as_absent(tmp_path, monkeypatch, tracks):
    folder = str(tmp_path)
    _write(folder, monkeypatch, tracks=tracks)
    assert ds.has_packed(folder)
    assert ds.PackedAudioDataset(folder).successors() is None


def test_gather_with_offsets_is_cat_and_slice(tmp_path, monkeypatch):
    folder = str(tmp_path)
    _write(folder, monkeypatch)
    packed = ds.PackedAudioDataset(folder)
    succ, w = packed.successors(), SHAPE[-1]
    with_succ = [i for i in range(N) if succ[i] >= 0]
    assert 2 in with_succ and 11 in with_succ  # idx 10 and idx 9: the successor sorts in front of / far from the item
    for o in (0, 1, 3, w // 2, w - 1):
        out = torch.full((len(with_succ),) + SHAPE, float("nan"))
        packed.gather(with_succ, out, [o] * len(with_succ))
        for k, i in enumerate(with_succ):
            want = torch.cat([packed[i], packed[int(succ[i])]], -1)[..., o:o + w]
            assert torch.equal(out[k], want), (i, o)
    # mixed offsets in one call, numpy offsets, an item without successor at offset 0
    idx, offs = [3, 0, 11, 7], np.array([0, 5, w - 1, 0], dtype=np.int32)
    out = torch.empty((4,) + SHAPE)
    packed.gather(idx, out, offs)
    assert torch.equal(out[0], packed[3]) and torch.equal(out[3], packed[7])
    assert torch.equal(out[1], torch.cat([packed[0], packed[1]], -1)[..., 5:5 + w])
    assert torch.equal(out[2], torch.cat([packed[11], packed[2]], -1)[..., w - 1:2 * w - 1])
    # offsets=None is the old result
    old, new = torch.empty((3,) + SHAPE), torch.empty((3,) + SHAPE)
    packed.gather([2, 0, 11], old)
    packed.gather([2, 0, 11], new, None)
    assert torch.equal(old, new) and all(torch.equal(old[k], packed[i]) for k, i in enumerate([2, 0, 11]))
    # a positive offset on an item without successor
    for i in (3, 6, 7):
        with pytest.raises(ValueError):
            packed.gather([i], torch.empty((1,) + SHAPE), [1])


def test_window_offsets_are_a_function_of_seed_epoch_and_sample():
    succ = np.array(SUCC * 50, dtype=np.int32)
    a, b = ds.window_offsets(succ, 5, 3), ds.window_offsets(succ, 5, 3)
    assert a.dtype == np.int32 and a.shape == succ.shape and np.array_equal(a, b)
    assert not np.array_equal(a, ds.window_offsets(succ, 5, 4)) and not np.array_equal(a, ds.window_offsets(succ, 6, 3))
    assert a.min() >= 0 and a.max() < 512 and a.max() > 256
    assert np.all(a[succ < 0] == 0) and np.any(a[succ >= 0] > 0)
    narrow = ds.window_offsets(succ, 5, 3, width=7)
    assert narrow.max() == 6 and np.all(narrow[succ < 0] == 0)


def test_offsets_do_not_depend_on_rank_world_or_skip():
    from musicgan_amd.train import ShardedShuffle
    succ = np.array(SUCC, dtype=np.int32)
    offs = ds.window_offsets(succ, 5, 1)
    one = ShardedShuffle(N, 5)
    one.set_epoch(1)
    seen = {i: int(offs[i]) for i in one}
    assert sorted(seen) == list(range(N))
    for skip in (0, 2):
        for rank in (0, 1):
            sh = ShardedShuffle(N, 5, rank, 2)
            sh.set_epoch(1, skip=skip)
            mine = list(sh)
            assert len(mine) == N // 2 - skip
            # each rank computes the table from (seed, epoch) alone and looks its own samples up
            table = ds.window_offsets(succ, sh.seed, sh.epoch)
            assert all(int(table[i]) == seen[i] for i in mine)


def test_sharded_shuffle_permutation_is_unchanged():
    """the values of the parent commit: the offsets take nothing from the permutation's generator"""
    from musicgan_amd.train import ShardedShuffle
    s = ShardedShuffle(12, 5)
    assert s._indices() == [11, 0, 9, 6, 10, 3, 4, 5, 8, 7, 1, 2]
    ds.window_offsets(np.array(SUCC, dtype=np.int32), 5, 1)
    s.set_epoch(1)
    assert s._indices() == [2, 9, 5, 0, 6, 3, 11, 8, 7, 1, 4, 10]
    r = ShardedShuffle(12, 5, 1, 2)
    r.set_epoch(1)
    assert r._indices() == [9, 0, 3, 8, 1, 10]


def test_resident_memory_rule():
    assert ds.RESIDENT_STAGE_SAMPLES == _cd().CHUNK_SAMPLES  # one staging buffer of create_dataset's chunk size
    ds.check_resident_fits(75, 100)
    ds.check_resident_fits(20 << 30, 280 << 30)
    with pytest.raises(MemoryError) as e:
        ds.check_resident_fits(76, 100)
    assert "76" in str(e.value) and "100" in str(e.value)
    ds.check_resident_fits(76, 100, max_fraction=0.8)
    with pytest.raises(MemoryError):
        ds.check_resident_fits(51, 100, max_fraction=0.5)


def test_window_index_validation():
    from musicgan_amd import window_ops
    ok = dict(rows=5, width=16)
    window_ops.check_windows(np.array([0, 4], np.int32), np.array([-1, 0], np.int32), np.array([0, 15], np.int32), **ok)
    for a, b, o in (([5], [0], [0]), ([-1], [0], [0]), ([0], [0], [16]), ([0], [0], [-1]), ([0], [-1], [1]), ([0], [5], [1])):
        with pytest.raises(ValueError):
            window_ops.check_windows(np.array(a, np.int32), np.array(b, np.int32), np.array(o, np.int32), **ok)


def test_cli_flags(monkeypatch):
    from musicgan_amd import __main__ as cli
    args = cli.build_parser().parse_args(["train", "R", "-i", "D", "-o", "O", "--resident", "--random-offset"])
    assert args.resident and args.random_offset
    calls = []
    train_mod = importlib.import_module("musicgan_amd.train")  # (the package attribute of that name may be the function)
    monkeypatch.setattr(train_mod, "train", lambda *a, **k: calls.append((a, k)))
    cli.main(["train", "R", "-i", "D", "-o", "O", "--resident", "--random-offset"])
    cli.main(["train", "R", "-i", "D", "-o", "O", "--random-offset"])
    cli.main(["train", "R", "-i", "D", "-o", "O"])
    cli.main(["train", "R", "-i", "D", "-o", "O", "--ema-decay", "0.999"])
    assert calls == [(("R", "D", "O"), {"resident": True, "random_offset": True}), (("R", "D", "O"), {"random_offset": True}),
                     (("R", "D", "O"), {}), (("R", "D", "O"), {"ema_decay": 0.999})]


def test_train_signature_defaults_off():
    import inspect
    from musicgan_amd.train import train
    p = inspect.signature(train).parameters
    assert p["resident"].default is False and p["random_offset"].default is False
    assert p["resident"].kind == p["random_offset"].kind == inspect.Parameter.KEYWORD_ONLY


def test_window_kernels_use_no_scratch_memory():
    """the resource check of tests/test_build.py over the two new kernels"""
    from musicgan_amd import _build
    _build.build()
    usage = {k: v for k, v in _build.resource_usage().items() if "itw_minmax_part" in k or "itw_resize_fused" in k}
    assert len(usage) == 2, sorted(usage)
    for name, u in usage.items():
        assert u.get("ScratchSize [bytes/lane]", 0) == 0 and u.get("VGPRs", 0) > 0, (name, u)


def test_train_refuses_the_flags_before_it_touches_the_device(tmp_path, monkeypatch):
    """no side-car: `resident` / `random_offset` say how to build one; a side-car without tracks (write_packed): `random_offset`
    says the dataset must be rewritten by create_dataset -- both as ValueError on a machine without a GPU"""
    from musicgan_amd.train import train
    monkeypatch.setattr(ds, "_SAMPLE_SHAPE", SHAPE)
    data = tmp_path / "data"
    data.mkdir()
    rng = torch.Generator().manual_seed(2)
    for i in range(2):
        torch.save((torch.rand(*SHAPE, generator=rng) * 2 - 1).double(), str(data / f"magn_phase_{i}.pt"))
    for flags in (dict(resident=True), dict(random_offset=True)):
        with pytest.raises(ValueError, match="write_packed"):
            train("t", str(data), str(tmp_path / "out"), **flags)
    assert ds.write_packed(str(data)) == 2
    with pytest.raises(ValueError, match="rewritten by create_dataset"):
        train("t", str(data), str(tmp_path / "out"), resident=True, random_offset=True)
    assert not (tmp_path / "out").exists()
