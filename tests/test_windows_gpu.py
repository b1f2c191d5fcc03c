"""Training from a dataset in device memory, with random time offsets: the windowed input transform against the existing kernel (bit
for bit) and against the tensor expressions, its 64-bit addressing, its behaviour on poisoned memory, the resident loader against the
packed loader, and the drivers (create_dataset's tracks, train with --resident / --random-offset, resume)."""
import importlib
import json
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _materialise(base, rows_a, rows_b, offs):
    """the windows as a tensor, by cat + slice on base's device"""
    w = base.shape[-1]
    return torch.stack([torch.cat([base[a], base[max(b, 0)]], -1)[..., o:o + w] for a, b, o in zip(rows_a, rows_b, offs)]).contiguous()


def _dev(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _mixed_batch(hw):
    """(rows_a, rows_b, offsets) over 5 rows: offset 0 with row_b = -1 (twice, once on the last row), 1, 3, W/2 with row_b == row_a,
    W - 1 with the last row as row_a and row_b < row_a, W/2 + 1 with row_b < row_a"""
    return [0, 1, 2, 3, 4, 4, 2], [-1, 2, 3, 3, 0, -1, 1], [0, 1, 3, hw // 2, hw - 1, 0, hw // 2 + 1]


# (98: rows of 392 bytes, so the 16-byte phase of a row's start changes from row to row)
@pytest.mark.parametrize("hw,side", [(96, 32), (100, 30), (512, 128), (512, 512), (512, 4), (98, 30)])
def test_windows_equal_the_existing_kernel_bit_for_bit(hw, side):
    """window_ops.input_transform_windows == ops.input_transform on the materialised windows, tolerance ZERO: both run the same tap
    arithmetic in the same order and min / max are exact; (100, 30) also against the tensor expressions on the CPU at the existing
    test's 3e-6, so that this test does not rest on the old kernel alone."""
    from musicgan_amd import audio, ops, window_ops
    g = torch.Generator().manual_seed(71)
    base = torch.rand(5, 2, hw, hw, generator=g) * 7 - 2
    base[0, 1] *= 1e-3  # a channel with a very different range
    ra, rb, of = _mixed_batch(hw)
    window_ops.check_windows(np.array(ra, np.int32), np.array(rb, np.int32), np.array(of, np.int32), 5, hw)
    dbase = base.to(DEV)
    mat = _materialise(dbase, ra, rb, of)
    got = window_ops.input_transform_windows(dbase, _dev(ra), _dev(rb), _dev(of), side)
    want = ops.input_transform(mat, side)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(ra), 2, side, side)
    diff = int((got != want).sum())
    print(f"WINDOWS {hw}->{side}: {diff} of {got.numel()} values differ from ops.input_transform")
    assert torch.equal(got, want)
    if (hw, side) == (100, 30):
        ref = audio.ChangeRange(-1.0, 1.0)(audio.ChannelMinMaxNorm()(_materialise(base, ra, rb, of)))
        ref = F.interpolate(ref, size=(side, side), mode="bilinear", antialias=True, align_corners=False).double()
        err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f"WINDOWS {hw}->{side}: rel err {err:.3e} against the tensor expressions")
        assert err <= 3e-6


def test_addresses_are_64_bit():
    """rows 2 048 and 2 049 of a (2 050, 2, 512, 512) float32 array lie beyond 2^32 bytes; the array is never filled"""
    from musicgan_amd import ops, window_ops
    base = torch.empty((2050, 2, 512, 512), dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(72)
    for r in (0, 2048, 2049):
        base[r] = (torch.rand(2, 512, 512, generator=g) * 7 - 2).to(DEV)
    ra, rb, of = [2048, 0], [2049, -1], [7, 0]
    got = window_ops.input_transform_windows(base, _dev(ra), _dev(rb), _dev(of), 128)
    want = ops.input_transform(_materialise(base, ra, rb, of), 128)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_body_on_poisoned_memory():
    """under poison.rule pointed at window_ops: no guard band damaged, no argument changed, the workspace poisoned before the call,
    equal digests under both fills, nothing non-finite; one sample has off = 0 and row_b = -1"""
    from musicgan_amd import window_ops
    g = torch.Generator().manual_seed(73)
    base = torch.rand(3, 2, 96, 96, generator=g) * 7 - 2
    ra, rb, of = [0, 2, 1, 2], [-1, 0, 2, 2], [0, 95, 5, 48]

    def run(p):
        p.out = window_ops.input_transform_windows(base.to(DEV), _dev(ra), _dev(rb), _dev(of), 32)
        torch.cuda.synchronize()

    r0, r1 = poison.rule(run, module=window_ops, inplace={})
    assert torch.equal(r0.out, r1.out) and bool(torch.isfinite(r1.out).all())
    names = [name for name, _, _ in r1.calls]
    assert "input_transform_windows" in names, names


# ------------------------------------------------------------------------------------------------------------------ the loaders
TRACKS = [[0, 5], [5, 1], [6, 6]]


@pytest.fixture(scope="module")
def sidecar12(tmp_path_factory):
    """12 stored samples (so that magn_phase_10.pt sorts in front of magn_phase_2.pt) with a side-car that records three tracks"""
    from musicgan_amd.audio import dataset as ds
    data = tmp_path_factory.mktemp("windows12")
    rng = torch.Generator().manual_seed(17)
    for i in range(12):
        torch.save((torch.rand(2, 512, 512, generator=rng) * 2 - 1).double(), str(data / f"magn_phase_{i}.pt"))
    assert ds.write_packed(str(data)) == 12
    meta_path = str(data / ds.PACKED_META)
    meta = json.load(open(meta_path))
    meta["tracks"] = TRACKS
    json.dump(meta, open(meta_path, "w"))
    assert ds.has_packed(str(data))
    return str(data)


@pytest.mark.parametrize("random_offset", [False, True])
def test_resident_loader_equals_packed_loader(sidecar12, random_offset):
    from musicgan_amd import audio
    from musicgan_amd.train import ShardedShuffle
    from musicgan_amd.utils import Grower
    packed = audio.PackedAudioDataset(sidecar12)
    succ = packed.successors()
    assert succ is not None and int((succ >= 0).sum()) == 9
    resident = audio.ResidentDataset(packed, DEV)
    assert tuple(resident.data.shape) == (12, 2, 512, 512) and torch.equal(resident.data[2].cpu(), packed[2])
    samplers = [ShardedShuffle(12, 5) for _ in range(2)]
    for s in samplers:
        s.set_epoch(3)
    idx = list(samplers[0])
    offs = audio.window_offsets(succ, 5, 3) if random_offset else np.zeros(12, np.int32)
    assert not random_offset or int((offs > 0).sum()) >= 5
    host = torch.empty((4, 2, 512, 512))
    growers = {}
    for side, downscale in ((4, 7), (128, 2)):
        growers[side] = Grower(7, [1] * 8, [1] * 7)
        growers[side].load_state_dict({"curr_grow": 7 - downscale, "sample_idx": 0, "step_sample_idx": 0, "downscale": downscale})
    a = audio.PackedLoader(packed, 4, samplers[0], DEV, random_offset=random_offset)
    b = audio.ResidentLoader(resident, 4, samplers[1], DEV, random_offset=random_offset)
    assert len(a) == len(b) == 3
    n = 0
    for k, (x, wb) in enumerate(zip(a, b)):
        assert isinstance(wb, audio.WindowBatch) and len(wb) == 4
        mine = idx[4 * k:4 * k + 4]
        assert wb.rows_a.tolist() == mine and wb.offsets.tolist() == [int(offs[i]) for i in mine]
        packed.gather(mine, host, [int(offs[i]) for i in mine])
        assert torch.equal(wb.materialise().cpu(), host) and torch.equal(x.cpu(), host)
        for side, grower in growers.items():
            ya, yb = grower.transform_batch(x), grower.transform_batch(wb)
            assert tuple(yb.shape) == (4, 2, side, side) and torch.equal(ya, yb), (k, side)
        n += 1
    assert n == 3


def test_flags_need_a_sidecar_and_tracks(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.train import ShardedShuffle, train
    data = tmp_path / "data"
    data.mkdir()
    rng = torch.Generator().manual_seed(17)
    for i in range(2):
        torch.save((torch.rand(2, 512, 512, generator=rng) * 2 - 1).double(), str(data / f"magn_phase_{i}.pt"))
    with pytest.raises(ValueError, match="side-car"):
        train("t", str(data), str(tmp_path / "o"), resident=True)
    audio.write_packed(str(data))
    with pytest.raises(ValueError, match="create_dataset"):
        train("t", str(data), str(tmp_path / "o"), random_offset=True)
    with pytest.raises(ValueError):
        audio.PackedLoader(audio.PackedAudioDataset(str(data)), 2, ShardedShuffle(2, 0), DEV, random_offset=True)


# ------------------------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope="module")
def stretched_corpus(tmp_path_factory):
    """create_dataset on two 256 * 1030-sample files with --stretch 9/10: the data directory"""
    from musicgan_amd.audio import wavio
    cd = importlib.import_module("musicgan_amd.create_dataset")  # (the package attribute of that name is the function)
    root = tmp_path_factory.mktemp("windows_corpus")
    wav_dir, data_dir = root / "wav", root / "data"
    wav_dir.mkdir()
    rng = torch.Generator().manual_seed(5)
    for i in range(2):
        wavio.save(str(wav_dir / f"s{i}.wav"), torch.rand(2, 256 * 1030, generator=rng) - 0.5, 44100)
    cd.create_dataset(str(wav_dir / "*.wav"), str(data_dir), stretch=(Fraction(9, 10),))
    return str(data_dir)


def test_create_dataset_writes_tracks(stretched_corpus):
    from musicgan_amd import audio
    from musicgan_amd.audio import dataset as ds
    cd = importlib.import_module("musicgan_amd.create_dataset")
    counts = cd.variant_counts(256 * 1030, audio.N_VEC, rates=(Fraction(9, 10),))
    assert counts == [2, 2]  # 1 031 frames: two chunks; 1 145 frames at rate 9/10: two chunks
    total = 2 * sum(counts)
    assert sorted(os.listdir(stretched_corpus)) == sorted([f"magn_phase_{i}.pt" for i in range(total)] +
                                                          [f"magn_phase_f32.bin.{k}" for k in range(16)] + ["magn_phase_f32.json"])
    meta = json.load(open(os.path.join(stretched_corpus, ds.PACKED_META)))
    assert meta["tracks"] == [[0, 2], [2, 2], [4, 2], [6, 2]]  # per file: its own samples, then the variant as a track of its own
    assert audio.PackedAudioDataset(stretched_corpus).successors().tolist() == [1, -1, 3, -1, 5, -1, 7, -1]


_KW = dict(nb_epoch=10, batch_size=2, num_workers=0, save_every=2, rand_channels=8,
           fadein_lengths=[1, 6, 6, 6, 6, 6, 6, 6], train_lengths=[5, 4, 100, 100, 100, 100, 100])


def _same_checkpoint(a, b, k):
    """every saved tensor of checkpoint k of two runs is bit-equal (the pattern of test_resume_is_bit_identical)"""
    sa, sb = torch.load(os.path.join(a, f"train_state_{k}.pt")), torch.load(os.path.join(b, f"train_state_{k}.pt"))
    assert sa["level"] == sb["level"] and sa["iter_idx"] == sb["iter_idx"] and sa["grower"] == sb["grower"]
    assert (sa["epoch"], sa["epoch_pos"]) == (sb["epoch"], sb["epoch_pos"])
    assert all(torch.equal(x, y) for x, y in zip(sa["noise_rng"], sb["noise_rng"]))
    for net in ("gen", "disc"):
        wa, wb = torch.load(os.path.join(a, f"{net}_{k}.pt")), torch.load(os.path.join(b, f"{net}_{k}.pt"))
        assert list(wa.keys()) == list(wb.keys())
        for key in wa:
            assert torch.equal(wa[key], wb[key]), f"{net} {key} differs"
        oa, ob = torch.load(os.path.join(a, f"optim_{net}_{k}.pt")), torch.load(os.path.join(b, f"optim_{net}_{k}.pt"))
        assert oa["state"].keys() == ob["state"].keys()
        for i in oa["state"]:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(oa["state"][i][key].cpu(), ob["state"][i][key].cpu()), f"optim_{net} state {i} {key}"
    return sa, sb


def test_resident_random_offset_resume_is_bit_identical(stretched_corpus, tmp_path):
    """8 iterations straight == 4 + resume + 4 with resident=True, random_offset=True: the offsets are a function of (seed, epoch,
    sample), so the resumed run draws the windows the straight one drew; a resume with other flags is refused"""
    from musicgan_amd.train import train
    flags = dict(resident=True, random_offset=True)
    torch.manual_seed(123)
    a = str(tmp_path / "straight")
    train("a", stretched_corpus, a, max_iters=8, **flags, **_KW)
    torch.manual_seed(123)
    b = str(tmp_path / "interrupted")
    train("b", stretched_corpus, b, max_iters=4, **flags, **_KW)
    st = torch.load(os.path.join(b, "train_state_1.pt"))
    assert st["iter_idx"] == 4 and st["resident"] is True and st["random_offset"] is True
    for other in (dict(resident=True), dict(random_offset=True), dict()):
        with pytest.raises(ValueError, match="resum"):
            train("b", stretched_corpus, b, max_iters=8, resume_from=b, **other, **_KW)
    torch.manual_seed(999)
    train("b", stretched_corpus, b, max_iters=8, resume_from=b, **flags, **_KW)
    sa, sb = _same_checkpoint(a, b, 3)
    assert sa["iter_idx"] == 8 and sa["level"] == 2


def test_resident_equals_the_default_loader(stretched_corpus, tmp_path):
    """resident=True without offsets trains on the same batches as the packed loader: every saved tensor after 6 iterations"""
    from musicgan_amd.train import train
    torch.manual_seed(123)
    a = str(tmp_path / "packed")
    train("a", stretched_corpus, a, max_iters=6, **_KW)
    torch.manual_seed(123)
    b = str(tmp_path / "resident")
    train("b", stretched_corpus, b, max_iters=6, resident=True, **_KW)
    sa, sb = _same_checkpoint(a, b, 2)
    assert sa["iter_idx"] == 6 and "resident" not in sa and sb["resident"] is True and "random_offset" not in sb
