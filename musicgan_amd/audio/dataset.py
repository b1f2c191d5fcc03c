"""Datasets over what create_dataset writes.

`AudioDataset(dataset_path)` is the reference's interface (/root/reference/music_gan/audio/dataset.py:14-44): items are the float64
(2, 512, 512) tensors of `magn_phase_{idx}.pt`, in file-name order, each read with `th.load` (4 MiB of pickle per sample -- about
300 samples/s per DataLoader worker, i.e. under 2 000 samples/s with the reference's 6 workers against the 3 900 images/s one
MI355X consumes at level 5).

`PackedAudioDataset` / `PackedLoader` read the optional side-car `create_dataset` writes next to those files: ONE memory-mapped
float32 array `magn_phase_f32.bin` of shape (S, 2, 512, 512) (the stored float64 values are float32 numbers widened -- the codec
computes in float32 -- so nothing is lost) plus `magn_phase_f32.json` (count, shape, the .pt file of every row).  A batch is then
one gather from the page cache into a pinned buffer and one asynchronous upload, double-buffered on a background thread: no
pickle, no worker processes, no float64 on the wire.

The side-car written by a single-process `create_dataset` also records the TRACKS: which runs of samples are consecutive chunks of
one spectrum.  Two consecutive chunks share their normalisation and are contiguous in time, so any 512-frame window that straddles
them is as valid a sample as the chunks themselves: `successors` / `window_offsets` / `gather(..., offsets)` serve such windows from
the host, `ResidentDataset` / `ResidentLoader` from a copy of the whole array in device memory, where a batch is three int32 index
vectors and the gather happens inside the input transform (musicgan_amd.window_ops).
"""
from __future__ import annotations

import fnmatch
import json
import os
import queue
import threading
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence

import numpy as np
import torch
from torch.utils.data import Dataset

from ..streams import new_stream

_PATTERN = "magn_phase_*.pt"
PACKED_BIN, PACKED_META = "magn_phase_f32.bin", "magn_phase_f32.json"
_SAMPLE_SHAPE = (2, 512, 512)
# The array may be split over `shards` files (meta "shards" / "block_rows"; 1 = the single file PACKED_BIN): row r lives in shard
# (r // B) % K at local row (r // (B * K)) * B + r % B.  create_dataset's writer threads fill it with concurrent pwrites, and writes
# to ONE file serialise on its inode lock (measured: 0.25 ms per 2 MiB row, i.e. 20 files/s whatever the thread count).
PACKED_SHARDS, PACKED_BLOCK_ROWS = 16, 8


def shard_name(k: int, shards: int) -> str:
    return PACKED_BIN if shards == 1 else f"{PACKED_BIN}.{k}"


def shard_of_row(r: int, shards: int, block_rows: int):
    """(shard, local row) of global row r."""
    b = r // block_rows
    return b % shards, (b // shards) * block_rows + r % block_rows


def shard_rows(count: int, shards: int, block_rows: int):
    """Rows each shard holds for `count` global rows."""
    out = [0] * shards
    full, rest = divmod(count, block_rows)
    for k in range(shards):
        out[k] = (full // shards + (1 if k < full % shards else 0)) * block_rows
    if rest:
        out[full % shards] += rest
    return out


def _sample_files(folder: str):
    with os.scandir(folder) as it:
        names = [e.name for e in it if e.is_file() and fnmatch.fnmatchcase(e.name, _PATTERN)
                 and e.name[len("magn_phase_"):-len(".pt")].isdigit()]
    names.sort()  # plain string order, as the reference sorts them
    return tuple(names)


class AudioDataset(Dataset):
    def __init__(self, dataset_path: str) -> None:
        super().__init__()
        assert os.path.isdir(dataset_path)
        self._root = dataset_path
        self._names = _sample_files(dataset_path)

    def __len__(self) -> int:
        return len(self._names)

    def __getitem__(self, index: int) -> torch.Tensor:
        return torch.load(os.path.join(self._root, self._names[index]))


# ---------------------------------------------------------------------------------------------------------------- packed side-car
def file_probe(path: str) -> int:
    """CRC-32 of 4 KiB from the middle of a sample file (tensor payload).  Every valid sample has the same size, so sizes alone
    cannot tell a regenerated dataset from the one the side-car was built from; this does, at one small read per file."""
    import zlib
    size = os.path.getsize(path)
    with open(path, "rb") as fh:
        fh.seek(max(0, size // 2 - 2048))
        return zlib.crc32(fh.read(4096))


def write_packed(dataset_path: str) -> int:
    """(Re)build the side-car from the `magn_phase_{idx}.pt` files of a dataset directory, rows in AudioDataset order (so index i
    of either dataset is the same sample).  Returns the number of samples."""
    names = _sample_files(dataset_path)
    if not names:
        return 0
    path = os.path.join(dataset_path, PACKED_BIN)
    try:
        os.remove(os.path.join(dataset_path, PACKED_META))  # never leave a meta file describing a half-written array
    except FileNotFoundError:
        pass
    try:
        mm = np.memmap(path + ".tmp", dtype=np.float32, mode="w+", shape=(len(names),) + _SAMPLE_SHAPE)
        for i, n in enumerate(names):
            x = torch.load(os.path.join(dataset_path, n))
            assert tuple(x.shape) == _SAMPLE_SHAPE, f"{n}: shape {tuple(x.shape)}"
            f = x.to(torch.float32)
            assert torch.equal(f.to(x.dtype), x), f"{n}: values are not float32-representable"
            mm[i] = f.numpy()
        mm.flush()
        del mm
    except BaseException:
        try:
            os.remove(path + ".tmp")
        except FileNotFoundError:
            pass
        raise
    os.replace(path + ".tmp", path)
    with open(os.path.join(dataset_path, PACKED_META), "w") as fh:
        json.dump({"count": len(names), "shape": list(_SAMPLE_SHAPE), "dtype": "float32", "files": list(names),
                   "rows": list(range(len(names))), "sizes": [os.path.getsize(os.path.join(dataset_path, n)) for n in names],
                   "probes": [file_probe(os.path.join(dataset_path, n)) for n in names]}, fh)
    return len(names)


def _read_meta(dataset_path: str):
    meta = os.path.join(dataset_path, PACKED_META)
    if not os.path.exists(meta):
        return None
    with open(meta) as fh:
        m = json.load(fh)
    k = int(m.get("shards", 1))
    if not all(os.path.exists(os.path.join(dataset_path, shard_name(i, k))) for i in range(k)):
        return None
    return m


def has_packed(dataset_path: str) -> bool:
    """True when the side-car exists AND still matches the directory's .pt files: same names in the same order, the same file
    sizes, the same CRC of a 4 KiB probe from the middle of every file, and an array file of the recorded length.  (create_dataset
    removes the side-car before it rewrites any .pt file, so a side-car never outlives the files it was built from; every valid
    sample has the same size, so it is the probe that catches files replaced behind its back by another tool.)"""
    m = _read_meta(dataset_path)
    if m is None:
        return False
    names = _sample_files(dataset_path)
    if tuple(m.get("files", ())) != names:
        return False
    if "sizes" in m and list(m["sizes"]) != [os.path.getsize(os.path.join(dataset_path, n)) for n in names]:
        return False
    if "probes" in m and list(m["probes"]) != [file_probe(os.path.join(dataset_path, n)) for n in names]:
        return False
    k, b = int(m.get("shards", 1)), int(m.get("block_rows", PACKED_BLOCK_ROWS))
    row_bytes = int(np.prod(_SAMPLE_SHAPE)) * 4
    sizes_ok = all(os.path.getsize(os.path.join(dataset_path, shard_name(i, k))) == n * row_bytes
                   for i, n in enumerate(shard_rows(int(m["count"]), k, b)))
    return sizes_ok and sorted(m.get("rows", range(len(names)))) == list(range(len(names)))


def _index_of_name(name: str) -> int:
    return int(name[len("magn_phase_"):-len(".pt")])


def _tracks_of(meta) -> Optional[list]:
    """The "tracks" of a side-car's meta data -- [first_idx, count] runs in the numbering of `magn_phase_{idx}.pt` -- when they
    are disjoint runs that cover [0, count) exactly and the files carry exactly those numbers; None otherwise (no key: written by
    `write_packed` or a multi-rank create_dataset; a malformed key counts as absent)."""
    tracks, count = meta.get("tracks"), int(meta["count"])
    if not isinstance(tracks, list) or not tracks:
        return None
    try:
        runs = sorted((int(f), int(c)) for f, c in tracks)
    except (TypeError, ValueError):
        return None
    at = 0
    for first, n in runs:
        if first != at or n < 1:
            return None
        at += n
    if at != count or sorted(_index_of_name(f) for f in meta.get("files", ())) != list(range(count)):
        return None
    return [list(r) for r in runs]


def window_offsets(successors, seed: int, epoch: int, width: int = _SAMPLE_SHAPE[-1]) -> np.ndarray:
    """One time offset per DATASET INDEX for epoch `epoch` of a run seeded `seed` (int32): uniform in [0, width) where the sample has
    a successor, 0 where it has none.  Window (i, o) is columns [o, width) of item i followed by columns [0, o) of item
    successors[i].  The draw comes from a generator of its own, `torch.Generator().manual_seed((seed * 1000003 + epoch +
    0x9E3779B9) mod 2^32)` (the CPU generator keeps 32 bits of a seed) -- one draw of `randint(0, width, (n,))` over all n samples
    -- so it is a function of (seed, epoch, sample) alone: it does not depend on the rank, the world size, the position in the
    epoch or a resume, and it takes nothing from the generator behind the epoch's permutation (ShardedShuffle seeds that one with
    seed + epoch)."""
    succ = np.asarray(successors)
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch) + 0x9E3779B9) % (1 << 32))
    drawn = torch.randint(0, int(width), (succ.shape[0],), generator=g, dtype=torch.int32).numpy()
    return np.where(succ >= 0, drawn, 0).astype(np.int32)


class PackedAudioDataset(Dataset):
    """Same items, same order as AudioDataset, served from the memory-mapped float32 side-car (items are float32).  Item i (file
    names in the reference's plain string order) lives in row `rows[i]` of the array: create_dataset streams the rows out in the
    order it produces them (idx 0, 1, 2, ...), which is not the string order of their names."""

    def __init__(self, dataset_path: str) -> None:
        super().__init__()
        assert has_packed(dataset_path), f"no valid {PACKED_BIN} in \"{dataset_path}\" (musicgan_amd.audio.dataset.write_packed)"
        meta = _read_meta(dataset_path)
        self._count = int(meta["count"])
        self._rows = np.asarray(meta.get("rows", range(self._count)), dtype=np.int64)
        self._k, self._b = int(meta.get("shards", 1)), int(meta.get("block_rows", PACKED_BLOCK_ROWS))
        self._files = tuple(meta["files"])
        self._tracks = _tracks_of(meta)
        self._succ: Optional[np.ndarray] = None
        self._mm = [np.memmap(os.path.join(dataset_path, shard_name(i, self._k)), dtype=np.float32, mode="r", shape=(n,) + _SAMPLE_SHAPE)
                    if n else None for i, n in enumerate(shard_rows(self._count, self._k, self._b))]

    def __len__(self) -> int:
        return self._count

    def _row(self, index: int):
        k, local = shard_of_row(int(self._rows[index]), self._k, self._b)
        return self._mm[k][local]

    def __getitem__(self, index: int) -> torch.Tensor:
        return torch.from_numpy(np.array(self._row(index)))

    def successors(self) -> Optional[np.ndarray]:
        """int32 array in dataset index order (names in plain string order): succ[i] is the index of `magn_phase_{idx + 1}.pt` when
        that file is the next chunk of the track item i (`magn_phase_{idx}.pt`) belongs to, else -1 (the last chunk of a track).  None
        when the side-car records no tracks."""
        if self._tracks is None:
            return None
        if self._succ is None:
            index_of = {_index_of_name(f): i for i, f in enumerate(self._files)}
            succ = np.full(self._count, -1, dtype=np.int32)
            for first, n in self._tracks:
                for idx in range(first, first + n - 1):
                    succ[index_of[idx]] = index_of[idx + 1]
            self._succ = succ
        return self._succ

    def gather(self, indices: Sequence[int], out: torch.Tensor, offsets: Optional[Sequence[int]] = None) -> torch.Tensor:
        """out[k] = sample indices[k]; `out` is a (len(indices), 2, 512, 512) float32 host tensor (pinned for async upload).
        With `offsets` (one per entry of `indices`): out[k] = window (indices[k], offsets[k]), columns [o, W) of the item followed by
        columns [0, o) of its successor -- two strided copies, the same number of bytes."""
        dst = out.numpy()
        if offsets is None:
            for k, i in enumerate(indices):
                dst[k] = self._row(i)
            return out
        succ, width = self.successors(), dst.shape[-1]
        for k, (i, o) in enumerate(zip(indices, offsets)):
            o = int(o)
            if o == 0:
                dst[k] = self._row(i)
                continue
            if not 0 < o < width:
                raise ValueError(f"offset {o} of item {i} outside [0, {width})")
            if succ is None or succ[i] < 0:
                raise ValueError(f"item {i} has no successor in its track: only offset 0 is possible, got {o}")
            dst[k][..., :width - o] = self._row(i)[..., o:]
            dst[k][..., width - o:] = self._row(int(succ[i]))[..., :o]
        return out


class PackedLoader:
    """Batches of a PackedAudioDataset already on the device: a background thread gathers batch b+1 into one of `depth` pinned
    buffers and queues its upload on a side stream while the caller trains on batch b.  Iterating yields float32 device tensors
    (B, 2, 512, 512) in sampler order with the tail dropped (the reference's drop_last=True).

    Buffer life cycle (slot s = pinned[s] + dev[s]):  the consumer frees a slot with STREAM-level ordering only (its kernels on
    dev[s] are queued, not finished), so the upload into dev[s] waits on that event on the loader stream -- and therefore may sit
    in the queue long after the producer got the slot back.  The producer must not gather into pinned[s] while an EARLIER upload
    out of pinned[s] is still pending: it waits on the HOST for that upload's event first (a training loop under graph replay
    has no host synchronisation of its own and runs many steps ahead of the GPU)."""

    def __init__(self, dataset: PackedAudioDataset, batch_size: int, sampler, device, depth: int = 3, random_offset: bool = False):
        self.ds, self.bs, self.sampler, self.device, self.depth = dataset, batch_size, sampler, torch.device(device), depth
        # random_offset: every sample with a successor in its track is served as a window at window_offsets(...)[sample], drawn per
        # epoch from (sampler.seed, sampler.epoch); needs a side-car with tracks
        self.random_offset = random_offset
        if random_offset and dataset.successors() is None:
            raise ValueError("random_offset needs a side-car with tracks (written by a single-process create_dataset)")
        self._pinned = [torch.empty((batch_size,) + _SAMPLE_SHAPE, dtype=torch.float32).pin_memory() for _ in range(depth)]
        self._dev = [torch.empty((batch_size,) + _SAMPLE_SHAPE, dtype=torch.float32, device=self.device) for _ in range(depth)]
        self._uploaded: List[Optional[torch.cuda.Event]] = [None] * depth  # last upload out of pinned[s] (kept across epochs)
        self._stream = new_stream(self.device)

    def __len__(self) -> int:
        return len(self.sampler) // self.bs

    def __iter__(self) -> Iterator[torch.Tensor]:
        idx: List[int] = list(iter(self.sampler))
        nb = len(idx) // self.bs
        offs = window_offsets(self.ds.successors(), self.sampler.seed, self.sampler.epoch) if self.random_offset else None
        ready: "queue.Queue" = queue.Queue(maxsize=self.depth - 1)
        free: "queue.Queue" = queue.Queue()
        for s in range(self.depth):
            free.put(s)
        stop = threading.Event()

        def post(item) -> bool:  # ready.put that gives up when the consumer has left
            while not stop.is_set():
                try:
                    ready.put(item, timeout=0.1)
                    return True
                except queue.Full:
                    continue
            return False

        def producer():
            try:
                torch.cuda.set_device(self.device)
                for b in range(nb):
                    slot = free.get()
                    if stop.is_set() or slot < 0:
                        return
                    if self._uploaded[slot] is not None:
                        self._uploaded[slot].synchronize()  # HOST wait: the previous upload has read pinned[slot]
                    mine = idx[b * self.bs:(b + 1) * self.bs]
                    if offs is None:
                        self.ds.gather(mine, self._pinned[slot])
                    else:
                        self.ds.gather(mine, self._pinned[slot], offs[mine])
                    with torch.cuda.stream(self._stream):
                        self._dev[slot].copy_(self._pinned[slot], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(self._stream)
                    self._uploaded[slot] = ev
                    if not post((slot, ev)):
                        return
                post(None)
            except BaseException as e:  # noqa: BLE001  (I/O error on the memmap, HIP error: re-raised by the consumer)
                post(e)

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        prev: Optional[int] = None
        try:
            while True:
                item = ready.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                slot, ev = item
                torch.cuda.current_stream(self.device).wait_event(ev)
                if prev is not None:  # the consumer moved on: its buffer may be refilled once the work queued on it has run
                    done = torch.cuda.Event()
                    done.record(torch.cuda.current_stream(self.device))
                    self._stream.wait_event(done)
                    free.put(prev)
                prev = slot
                yield self._dev[slot]
        finally:
            stop.set()
            free.put(-1)
            while True:  # a producer blocked in ready.put returns as soon as there is room or it sees `stop`
                try:
                    ready.get_nowait()
                except queue.Empty:
                    break
            th.join(timeout=5)


# ------------------------------------------------------------------------------------------------- the dataset in device memory
RESIDENT_STAGE_SAMPLES = 32  # samples of the pinned staging buffer of the upload: create_dataset's chunk (CHUNK_SAMPLES, 64 MiB)
RESIDENT_FRACTION = 0.75  # of the free device memory the array may take: a POLICY (room for the activations of a level-7 step),
#                           not a measurement


def check_resident_fits(need_bytes: int, free_bytes: int, max_fraction: float = RESIDENT_FRACTION) -> None:
    """MemoryError (naming both numbers) when an array of need_bytes would take more than max_fraction of free_bytes."""
    if need_bytes > max_fraction * free_bytes:
        raise MemoryError(f"the dataset needs {need_bytes} bytes of device memory, more than {max_fraction:g} of the "
                          f"{free_bytes} bytes that are free: train without `resident` (the packed loader streams it from the host)")


class ResidentDataset:
    """The whole side-car in ONE float32 (S, 2, 512, 512) device tensor `data`, row i = item i of the dataset (AudioDataset order),
    uploaded once through one pinned staging buffer of create_dataset's chunk size by the calling thread.  `max_fraction`: see
    RESIDENT_FRACTION.  Under data-parallel training every rank holds the whole array (any rank may draw any index)."""

    def __init__(self, dataset: PackedAudioDataset, device, max_fraction: float = RESIDENT_FRACTION):
        self.packed, self.device = dataset, torch.device(device)
        count = len(dataset)
        need = count * int(np.prod(_SAMPLE_SHAPE)) * 4
        free, _ = torch.cuda.mem_get_info(self.device)
        check_resident_fits(need, free, max_fraction)
        self.data = torch.empty((count,) + _SAMPLE_SHAPE, dtype=torch.float32, device=self.device)
        stage = torch.empty((RESIDENT_STAGE_SAMPLES,) + _SAMPLE_SHAPE, dtype=torch.float32).pin_memory()
        for c0 in range(0, count, RESIDENT_STAGE_SAMPLES):
            n = min(RESIDENT_STAGE_SAMPLES, count - c0)
            dataset.gather(range(c0, c0 + n), stage[:n])
            self.data[c0:c0 + n].copy_(stage[:n], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()  # the one staging buffer is refilled next

    def __len__(self) -> int:
        return self.data.shape[0]

    def successors(self) -> Optional[np.ndarray]:
        return self.packed.successors()


@dataclass
class WindowBatch:
    """A batch that has not been gathered: window k is columns [offsets[k], W) of source[rows_a[k]] followed by columns
    [0, offsets[k]) of source[rows_b[k]] (rows_b[k] = -1 and never read where offsets[k] = 0).  `source` is the resident array, the
    three vectors are int32 views of length B into an epoch's arrays on the same device."""
    source: torch.Tensor
    rows_a: torch.Tensor
    rows_b: torch.Tensor
    offsets: torch.Tensor

    def __len__(self) -> int:
        return self.rows_a.shape[0]

    def materialise(self) -> torch.Tensor:
        """the (B, 2, H, W) float32 tensor of the windows, by tensor expressions on the device (tests, consumers other than the
        training loop's transform)"""
        width = self.source.shape[-1]
        both = torch.cat([self.source[self.rows_a.long()], self.source[self.rows_b.clamp_min(0).long()]], dim=-1)
        cols = self.offsets.long()[:, None] + torch.arange(width, device=self.source.device)[None, :]
        return torch.gather(both, -1, cols[:, None, None, :].expand(-1, both.shape[1], both.shape[2], -1))


class ResidentLoader:
    """Batches of a ResidentDataset as `WindowBatch`es, in sampler order with the tail dropped (as PackedLoader).  Per epoch: the
    sampler's indices, their offsets (`window_offsets` of (sampler.seed, sampler.epoch) with `random_offset`, else all zero) and
    successors are validated on the host and uploaded ONCE as three int32 vectors; a batch is a view into them.  No per-batch
    host-to-device copy, no background thread."""

    def __init__(self, resident: ResidentDataset, batch_size: int, sampler, device, random_offset: bool = False):
        self.resident, self.bs, self.sampler, self.device = resident, batch_size, sampler, torch.device(device)
        self.random_offset = random_offset
        if random_offset and resident.successors() is None:
            raise ValueError("random_offset needs a side-car with tracks (written by a single-process create_dataset)")

    def __len__(self) -> int:
        return len(self.sampler) // self.bs

    def __iter__(self) -> Iterator[WindowBatch]:
        from .. import window_ops
        idx = np.asarray(list(iter(self.sampler)), dtype=np.int32)
        nb = len(idx) // self.bs
        rows_a = idx[:nb * self.bs]
        if self.random_offset:
            succ = self.resident.successors()
            offs = window_offsets(succ, self.sampler.seed, self.sampler.epoch, self.resident.data.shape[-1])[rows_a]
            rows_b = np.where(offs > 0, succ[rows_a], -1).astype(np.int32)
        else:
            offs, rows_b = np.zeros_like(rows_a), np.full_like(rows_a, -1)
        window_ops.check_windows(rows_a, rows_b, offs, len(self.resident), self.resident.data.shape[-1])
        if nb == 0:
            return
        # the epoch's only host-to-device copy, out of pinned memory so that the host does not wait for the queue to drain
        host = torch.from_numpy(np.stack([rows_a, rows_b, offs])).pin_memory()
        epoch = host.to(self.device, non_blocking=True)
        for b in range(nb):
            lo, hi = b * self.bs, (b + 1) * self.bs
            yield WindowBatch(self.resident.data, epoch[0, lo:hi], epoch[1, lo:hi], epoch[2, lo:hi])
