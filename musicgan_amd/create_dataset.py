"""`create_dataset(audio_path_glob, dataset_output_dir)` (/root/reference/music_gan/create_dataset.py:13-64): wav files ->
STFT -> (magnitude, phase-delta) images -> `magn_phase_{idx}.pt` (float64, shape (2,512,512)), STFT and codec on the GPU.
Under torchrun the files are dealt round-robin to the ranks (independent units, no collective); the global sample numbering
stays the reference's (files in glob order) because each file's sample count follows from its length alone.

The GPU side of a 10-minute file is ~0.5 ms; what the loop spends its time on is the 843 MB of float64 `.pt` files it has to
leave behind (201 samples x 4 MiB, create_dataset.py:52-62).  So the loop is a pipeline: the codec writes the stacked
(S, 2, 512, 512) float32 tensor in one pass (`mg_codec_fwd_strided`), it comes back in chunks through a ring of pinned buffers
(float32 on the wire: half the bytes of the reference's `.to(th.float64).cpu()`), a pool of writer threads widens each sample to
float64 and `th.save`s it while the GPU and the copy engine work on the next chunk / file, and the float32 side-car of the fast
loader (audio/dataset.py) is streamed out of the same pinned chunks instead of re-reading every `.pt` afterwards.
`stats` (optional dict) receives where the time went: bench.py's `create_dataset_e2e` record.
`resample=True` accepts files at any sample rate: their PCM is resampled to 44.1 kHz on the device (ops.resample_pcm, the
torchaudio.functional.resample a user of the reference calls first) in the launch that also normalises it; 44.1 kHz files take the
unchanged path.
`stretch` / `pitch` add re-timed and transposed copies of every file behind its own samples (audio.phase_vocoder on the file's STFT;
for a pitch, the mono signal resampled by P / Q first and re-timed by Q / P, which restores the duration): the remedy for a small
corpus.  Without them nothing changes.
`preserve_transients` (with `stretch` / `pitch` only) re-times every variant as audio.time_stretch(..., preserve_transients=True)
does: the harmonic part of the spectrum (audio.hpss) through the phase vocoder, the percussive part by overlap-add, so that drum hits
are not smeared; the variant has the same number of frames either way.  `component` ("harmonic" or "percussive") replaces every
spectrum about to be coded, the original's and each variant's, by that component of it.  Without the two nothing changes.
`phase_lock` (with `stretch` / `pitch` only) sends the variants through the phase-locked vocoder (audio.phase_vocoder(...,
phase_lock=True): the bins of one partial keep their phase differences, so moving pitches do not warble); the frame counts are the
same.  Without it nothing changes.
A single-process run records in the side-car which samples are consecutive chunks of one spectrum ("tracks": a file's own samples
are one, each variant another): what training with random time offsets (`train --random-offset`) cuts its windows from.
"""
import glob
import json
import os
import queue
import threading
import time
from os.path import exists, isdir, join

import torch as th

from . import audio
from .audio import dataset as _ds
from .streams import new_stream

CHUNK_SAMPLES = 32  # samples per pinned chunk (64 MiB of float32)
RING_CHUNKS = 6     # pinned chunks in flight between the copy streams and the writer threads


def host_cpus() -> int:
    """CPUs this process may really use: min(affinity mask, cgroup cpu.max quota)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def _nb_samples(nb_frames_wav: int, nb_vec: int) -> int:
    t = 1 + nb_frames_wav // audio.STFT_STRIDE
    return 0 if t < nb_vec else (t - 1) // nb_vec


def check_variants(stretch=(), pitch=()):
    """-> (stretch rates as Fractions, [(pitch value, P / Q)]); ValueError for a rate outside [1/8, 8], a rate of exactly 1 or a
    pitch of exactly 0 (each would duplicate the original) and duplicate entries -- host arithmetic, no device needed"""
    from . import pv_ops
    rates = [pv_ops.as_rate(r) for r in stretch]
    if any(r == 1 for r in rates):
        raise ValueError("a stretch rate of 1 would duplicate the original")
    if len(set(rates)) != len(rates):
        raise ValueError(f"duplicate stretch rates: {[str(r) for r in rates]}")
    ratios = []
    for v in pitch:
        f = audio.pitch_ratio(v)
        if float(v) == 0 or f == 1:
            raise ValueError(f"a pitch of {v} semitones would duplicate the original")
        pv_ops.as_rate(1 / f)
        ratios.append((v, f))
    if len({float(v) for v, _ in ratios}) != len(ratios) or len({f for _, f in ratios}) != len(ratios):
        raise ValueError(f"duplicate pitch values: {[str(v) for v, _ in ratios]}")
    return tuple(rates), tuple(ratios)


COMPONENTS = ("harmonic", "percussive")


def check_separation(component=None, preserve_transients=False, rates=(), ratios=()) -> None:
    """ValueError for a component other than None / "harmonic" / "percussive" and for preserve_transients without a variant to
    apply it to -- host arithmetic, no device needed"""
    if component is not None and component not in COMPONENTS:
        raise ValueError(f"component must be one of {COMPONENTS} or None, got {component!r}")
    if not isinstance(preserve_transients, bool):
        raise ValueError(f"preserve_transients must be True or False, got {preserve_transients!r}")
    if preserve_transients and not (rates or ratios):
        raise ValueError("preserve_transients applies to the stretch / pitch variants: give at least one")


def check_phase_lock(phase_lock=False, rates=(), ratios=()) -> None:
    """ValueError for a phase_lock that is no bool and for phase_lock without a variant to apply it to -- host arithmetic"""
    if not isinstance(phase_lock, bool):
        raise ValueError(f"phase_lock must be True or False, got {phase_lock!r}")
    if phase_lock and not (rates or ratios):
        raise ValueError("phase_lock applies to the stretch / pitch variants: give at least one")


def variant_counts(nb_frames_wav: int, nb_vec: int, rates=(), ratios=()) -> list:
    """samples of a file of nb_frames_wav frames at 44.1 kHz and of each of its variants, in the order they are written: host
    arithmetic on the length alone (what the global numbering under torchrun rests on)"""
    from . import ops, pv_ops

    def of_frames(t):
        return 0 if t < nb_vec else (t - 1) // nb_vec
    t0 = 1 + nb_frames_wav // audio.STFT_STRIDE
    out = [_nb_samples(nb_frames_wav, nb_vec)]
    out += [of_frames(pv_ops.phase_vocoder_len(t0, r.numerator, r.denominator)) for r in rates]
    for _, f in ratios:
        t1 = 1 + ops.resample_len(nb_frames_wav, f.numerator, f.denominator) // audio.STFT_STRIDE
        out.append(of_frames(pv_ops.phase_vocoder_len(t1, f.denominator, f.numerator)))
    return out


def _remove_sidecar(folder: str) -> None:
    shards = [os.path.basename(p) for p in glob.glob(join(glob.escape(folder), _ds.PACKED_BIN + ".*"))]
    for name in [_ds.PACKED_META, _ds.PACKED_BIN] + shards:  # meta first: a reader never sees meta without data
        try:
            os.remove(join(folder, name))
        except FileNotFoundError:
            pass


class _Writers:
    """`n` threads that widen float32 samples to float64 and write them as `.pt` files (create_dataset.py:52-62); the first failure
    is kept and re-raised by `close()` / the next `submit()`.  A job is a run of consecutive rows of one pinned chunk.  With a
    template (fast_pt.PtTemplate) the per-sample work -- side-car row, widening, container prefix | payload | suffix -- is ONE native
    call per job (`mg_pt_write_samples`, made without the interpreter lock); the Python left per sample is the 600-byte suffix."""

    JOB_ROWS = 8

    def __init__(self, n: int, template=None):
        self.q: "queue.Queue" = queue.Queue(maxsize=4 * n)
        self.template = template  # fast_pt.PtTemplate (byte-identical th.save output from a template + the payload's CRC) or None
        self.err = None
        self.busy_s = 0.0
        self._lock = threading.Lock()
        self.threads = [threading.Thread(target=self._run, daemon=True) for _ in range(n)]
        for t in self.threads:
            t.start()

    def _run(self):
        import ctypes
        from . import _lib
        while True:
            job = self.q.get()
            if job is None:
                return
            chunk, row, paths, side_fd, side_off, check_first = job
            try:
                if self.err is None:
                    chunk.event.synchronize()  # the chunk's device-to-host copy has landed
                    t0 = time.perf_counter()
                    n = len(paths)
                    if self.template is not None:
                        tp = self.template
                        crcs = [int(v) & 0xFFFFFFFF for v in chunk.crc[row:row + n].tolist()]  # from the GPU, came with the samples
                        if check_first:  # spot check (first sample of a file): the GPU's CRC against zlib's on the same bytes
                            import zlib
                            wide = chunk.host[row].numpy().astype("float64")
                            assert zlib.crc32(wide) & 0xFFFFFFFF == crcs[0], f"device CRC-32 of {paths[0]} disagrees with zlib"
                        suffixes = b"".join(tp.suffix(c) for c in crcs)
                        rows = chunk.host[row:row + n]
                        _lib.check(_lib.load().mg_pt_write_samples(
                            ctypes.c_void_p(rows.data_ptr()), n, rows[0].numel(), b"\0".join(os.fsencode(p) for p in paths) + b"\0",
                            tp.prefix, len(tp.prefix), suffixes, len(suffixes) // n, -1 if side_fd is None else side_fd, side_off),
                            "mg_pt_write_samples")
                    else:
                        for i, path in enumerate(paths):
                            arr = chunk.host[row + i].numpy()
                            if side_fd is not None:  # the float32 side-car row of this sample, at its place in the array file
                                view, done = memoryview(arr).cast("B"), 0
                                while done < len(view):
                                    done += os.pwrite(side_fd, view[done:], side_off + i * arr.nbytes + done)
                            # (numpy, not torch: its intra-op pool under 16 writer threads made `.to(float64)` cost 20-50 ms a sample)
                            th.save(th.from_numpy(arr.astype("float64")), path)
                    with self._lock:
                        self.busy_s += time.perf_counter() - t0
            except BaseException as e:  # noqa: BLE001  (kept for the submitting thread)
                self.err = self.err or e
            finally:
                chunk.release()

    def submit(self, chunk, row, paths, side_fd=None, side_off=0, check_first=False):
        """`paths`: the files of rows row .. row + len(paths) - 1 of `chunk` (side-car rows consecutive from byte `side_off`)."""
        if self.err is not None:
            raise self.err
        chunk.acquire()
        self.q.put((chunk, row, list(paths), side_fd, side_off, check_first))

    def close(self):
        for _ in self.threads:
            self.q.put(None)
        for t in self.threads:
            t.join()
        if self.err is not None:
            raise self.err


class _Loader:
    """Reads, page-locks and uploads the wav files ahead of the loop that transforms them (create_dataset.py:34-38 does
    `wav_to_stft(path)` in line): WORKERS threads, worker i taking files i, i + WORKERS, ...; each maps its file, copies the PCM
    frames AS STORED (int16 stays int16: half of float32's bytes; de-interleaving, scaling and the mono mean happen inside the STFT
    kernel) through two pinned staging buffers of its own and queues the host-to-device copies on its own stream, while the main
    thread is busy with the device-to-host copies and writers of earlier files.  (One thread moved a 106 MB float32 file in ~27 ms
    -- page cache -> pinned memory is a single-core copy -- and was the loop's slowest stage once the writers were fixed, r05.)
    Items come out in file order: (path, device PCM tensor (frames, channels) or None, sample rate, ready event)."""

    STAGE_BYTES = 32 << 20  # two pinned staging buffers of this size per worker, page-locked by the worker while the ring is set up
    WORKERS = 3

    def __init__(self, paths, device, workers: int = 0):
        paths = list(paths)
        self.device = device
        self.busy_s = 0.0  # summed over the workers
        self._stop = False
        self._lock = threading.Lock()
        n = max(1, min(workers or self.WORKERS, len(paths)))
        self.workers = n
        self._n_files = len(paths)
        self._qs = [queue.Queue(maxsize=1) for _ in range(n)]
        self._threads = [threading.Thread(target=self._run, args=(paths[i::n], self._qs[i]), daemon=True) for i in range(n)]
        for t in self._threads:
            t.start()

    def _run(self, paths, out_q):
        import numpy as np
        try:
            th.cuda.set_device(self.device)
            pins = [th.empty(self.STAGE_BYTES, dtype=th.uint8).pin_memory() for _ in range(2)]
            stream = new_stream(self.device)
            events = [None, None]
            tdt = {np.dtype(np.int16): th.int16, np.dtype(np.int32): th.int32, np.dtype(np.uint8): th.uint8,
                   np.dtype(np.float32): th.float32}
            slot = 0
            for path in paths:
                if self._stop:
                    return
                t0 = time.perf_counter()
                fl = vs = None
                ext = os.path.splitext(path)[1].lower()
                if ext in audio.wavio.OGG_EXTS:
                    # the whole file travels (through the same staging buffers) and is decoded on this worker's stream; the
                    # pages are walked and the headers parsed here, on the host
                    from . import ops
                    raw = np.fromfile(path, dtype=np.uint8)
                    vs = audio.wavio.vorbis.parse(raw, path)
                    nbytes = raw.size
                    pcm, sr, offset = raw, vs.setup.rate, None
                    with th.cuda.stream(stream):
                        dev = th.empty(nbytes, dtype=th.uint8, device=self.device)
                elif ext == ".flac":
                    # the compressed frames travel as they are (through the same staging buffers) and are decoded on this
                    # worker's stream; the decoder's one status read-back is this file's only host synchronisation
                    from . import ops
                    fl = audio.wavio.flac.read_header(path)
                    nbytes = fl.audio_end - fl.audio_offset
                    pcm, sr, offset = None, fl.sample_rate, fl.audio_offset
                    with th.cuda.stream(stream):
                        dev = th.empty(ops.flac_padded_bytes(nbytes), dtype=th.uint8, device=self.device)
                        dev[nbytes:].zero_()
                else:
                    pcm, sr = audio.wavio.load_pcm(path)  # a memory map where the format allows: header parsed, no sample read yet
                    nbytes = pcm.size * pcm.dtype.itemsize
                    with th.cuda.stream(stream):
                        dev = th.empty(nbytes, dtype=th.uint8, device=self.device)
                    offset = getattr(pcm, "offset", None)
                fh = open(path, "rb") if offset is not None else None
                flat = None if fh is not None else np.ascontiguousarray(pcm).reshape(-1).view(np.uint8)
                try:
                    if fh is not None:
                        fh.seek(offset)
                    for o in range(0, nbytes, self.STAGE_BYTES):
                        n = min(self.STAGE_BYTES, nbytes - o)
                        if events[slot] is not None:
                            events[slot].synchronize()  # the upload that last read this staging buffer has finished (HOST wait)
                        host = pins[slot][:n]
                        if fh is not None:  # file (page cache) -> pinned memory in one pass, no intermediate array
                            got = fh.readinto(memoryview(host.numpy()))
                            assert got == n, f"short read from {path}"
                        else:
                            host.numpy()[...] = flat[o:o + n]
                        with th.cuda.stream(stream):
                            dev[o:o + n].copy_(host, non_blocking=True)
                            ev = th.cuda.Event()
                            ev.record(stream)
                        events[slot] = ev
                        slot ^= 1
                finally:
                    if fh is not None:
                        fh.close()
                if vs is not None:
                    with th.cuda.stream(stream):
                        item = ops.vorbis_decode(dev, vs, name=path)
                        ready = th.cuda.Event()
                        ready.record(stream)
                    del pcm
                elif fl is not None:
                    with th.cuda.stream(stream):
                        item = ops.flac_decode(dev, fl, nbytes=nbytes, name=path)
                        ready = th.cuda.Event()
                        ready.record(stream)
                else:
                    with th.cuda.stream(stream):
                        ready = th.cuda.Event()
                        ready.record(stream)
                    shape, dt = (pcm.shape[0], pcm.shape[1]), tdt[pcm.dtype]
                    del pcm
                    item = dev.view(dt).view(*shape)
                with self._lock:
                    self.busy_s += time.perf_counter() - t0
                out_q.put((path, item, sr, ready))
        except BaseException as e:  # noqa: BLE001  (re-raised by the consumer)
            out_q.put(e)

    def __iter__(self):
        for k in range(self._n_files):  # file k comes from worker k % workers
            item = self._qs[k % self.workers].get()
            if isinstance(item, BaseException):
                raise item
            yield item

    def close(self):
        self._stop = True
        for t, q in zip(self._threads, self._qs):
            while t.is_alive():  # a producer blocked on a full queue needs room to see the flag
                try:
                    q.get_nowait()
                except queue.Empty:
                    pass
                t.join(timeout=0.05)


class _Chunk:
    """One pinned (CHUNK_SAMPLES, 2, 512, nb_vec) float32 buffer of the ring; reusable once every consumer released it."""

    def __init__(self, nb_vec: int, ring: "queue.Queue"):
        self.host = th.empty((CHUNK_SAMPLES, 2, audio.N_FFT // 2, nb_vec), dtype=th.float32).pin_memory()
        self.crc = th.empty((CHUNK_SAMPLES,), dtype=th.int64).pin_memory()  # CRC-32 of each sample's float64 bytes (mg_crc32_f64)
        self.event = th.cuda.Event()
        self._ring, self._refs, self._lock = ring, 0, threading.Lock()

    def acquire(self):
        with self._lock:
            self._refs += 1

    def release(self):
        with self._lock:
            self._refs -= 1
            done = self._refs == 0
        if done:
            self._ring.put(self)


def create_dataset(audio_path: str, dataset_output_dir: str, *, packed: bool = True, writer_threads: int = 0,
                   stats: dict = None, resample: bool = False, stretch=(), pitch=(), component=None,
                   preserve_transients: bool = False, phase_lock: bool = False) -> None:
    """`packed` (extension, single-process runs): also write the float32 memory-mapped side-car the fast loader reads
    (audio/dataset.py); the reference-format `magn_phase_{idx}.pt` files are written either way.  `writer_threads`: 0 = one per
    available CPU (at most 16).  `resample`: files not at 44.1 kHz are resampled to it (else they raise, as in the reference).
    `stretch`: rates (int, Fraction or float, as audio.phase_vocoder takes them; above 1: faster); `pitch`: semitones.  Behind its own
    samples every file also yields, in the order given, those of its STFT re-timed by each rate, then those of its mono 44.1 kHz
    signal resampled by P / Q = audio.pitch_ratio(value) and re-timed by Q / P.  `preserve_transients`: the variants are re-timed
    with their percussive part overlap-added instead of going through the phase vocoder (a file of fewer than 4 frames raises
    audio.istft's ValueError).  `component`: "harmonic" or "percussive", what audio.hpss leaves of every spectrum is coded.
    `phase_lock` (with `stretch` / `pitch` only): the variants go through the phase-locked vocoder (audio.phase_vocoder(...,
    phase_lock=True)); with `preserve_transients` their harmonic part does."""
    rates, ratios = check_variants(stretch, pitch)
    check_separation(component, preserve_transients, rates, ratios)
    check_phase_lock(phase_lock, rates, ratios)
    w_p = glob.glob(audio_path)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # (dmabuf IPC, before the first HIP call: train.py)
    if not exists(dataset_output_dir):
        os.makedirs(dataset_output_dir, exist_ok=True)
    elif not isdir(dataset_output_dir):
        raise NotADirectoryError(f"\"{dataset_output_dir}\" is not a directory")
    # whatever side-car an earlier run left describes OTHER .pt files than the ones about to be written (same names!)
    _remove_sidecar(dataset_output_dir)
    nb_vec = audio.N_VEC
    if world > 1:
        th.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
        counts = []
        for p in w_p:
            frames, _, sr, _ = audio.wavio.info(p)  # headers only: no audio is read
            if resample and sr != audio.SAMPLE_RATE:  # the samples come from the resampled signal: ceil(44100 L / sr) frames
                from . import ops
                frames = ops.resample_len(frames, sr, audio.SAMPLE_RATE)
            counts.append(sum(variant_counts(frames, nb_vec, rates, ratios)) if rates or ratios else _nb_samples(frames, nb_vec))
    t_setup = time.perf_counter()
    mine = [f_i for f_i in range(len(w_p)) if world == 1 or f_i % world == rank]
    first_idx = {}
    if world > 1:  # global sample numbering: files of other ranks in front of each of mine
        run = 0
        for f_i in range(len(w_p)):
            first_idx[f_i] = run
            run += counts[f_i]
    dev = th.device("cuda", th.cuda.current_device())
    # started first: it reads and uploads the first files while the chunk ring below is being page-locked
    loader = _Loader([w_p[f_i] for f_i in mine], dev, workers=int(os.environ.get("MG_LOADER_THREADS", "0")) or max(1, min(
        _Loader.WORKERS, host_cpus() // max(1, int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))) // 4)))
    # writer threads: one per CPU this process may use (at most 16) -- divided by the ranks sharing the host: 8 ranks x 16 threads
    # on the cores of one node only take turns (the widen + write path is memory-bandwidth-bound)
    cpus = host_cpus()
    local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
    n_thr = writer_threads or max(1, min(16, cpus // local_world))
    ring: "queue.Queue" = queue.Queue()
    for _ in range(RING_CHUNKS):
        ring.put(_Chunk(nb_vec, ring))
    # device-to-host copies go out on two streams of their own, alternating by chunk: the loop's stream never waits for a copy
    # (it used to carry them, and the per-file `.cpu()` of the CRCs then waited for 421 MB of copies each time)
    copy_streams = [new_stream(dev) for _ in range(2)]
    n_chunks = 0
    # th.save's output for a (2, 512, nb_vec) float64 tensor as a template (checked against th.save at construction; None: keep
    # calling th.save): the container's CRC-32 then comes from the GPU (mg_crc32_f64) instead of one host core per sample
    template = None
    if os.environ.get("MG_FAST_PT", "1") != "0":
        from .fast_pt import PtTemplate
        template = PtTemplate((2, audio.N_FFT // 2, nb_vec))
        if not template.ok:
            template = None
    writers = _Writers(n_thr, template)
    side = None
    names = []
    tracks = []  # [first idx, count] of every spectrum written (a file's own samples; each of its variants): consecutive chunks
    if packed and world == 1:
        # written row by row by the writer threads (os.pwrite at row idx): one thread streaming 421 MB per file was the
        # slowest stage of the loop
        # into PACKED_SHARDS files, blocks of PACKED_BLOCK_ROWS rows dealt round-robin: concurrent writes to ONE file take turns on
        # its inode lock (0.25 ms per 2 MiB row = 20 files/s however many threads write)
        side = [os.open(join(dataset_output_dir, _ds.shard_name(k, _ds.PACKED_SHARDS) + ".tmp"), os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                for k in range(_ds.PACKED_SHARDS)]
    t_start = time.perf_counter()
    t_setup = t_start - t_setup  # pinned ring (RING_CHUNKS x 64 MiB page-locked) + writer threads: paid once per call
    t_gpu = t_load = t_wait = t_drain = t_loader = 0.0
    row_bytes = 2 * (audio.N_FFT // 2) * nb_vec * 4
    idx = n_files = 0
    ok = False
    try:
        for f_i, (wav_p, pcm, sr, ready) in zip(mine, loader):
            if world > 1:
                idx = first_idx[f_i]
            t0 = time.perf_counter()
            assert resample or sr == audio.SAMPLE_RATE, \
                f"Audio sample rate must be {audio.SAMPLE_RATE}Hz, " \
                f"file \"{wav_p}\" is {sr}Hz"
            th.cuda.current_stream().wait_event(ready)  # the upload (loader's stream) is ordered in front of the STFT
            pcm.record_stream(th.cuda.current_stream())
            complex_values = audio.functions.stft_from_pcm(pcm, nperseg=audio.N_FFT, stride=audio.STFT_STRIDE, sample_rate=sr)
            if not ratios:
                del pcm
            t1 = time.perf_counter()
            t_load += t1 - t0
            spectra = [complex_values]
            if rates or ratios:  # the variants of this file, from the spectrum and the PCM that are on the device already
                from . import ops, pv_ops

                def retime(spectrum, r):
                    if not preserve_transients:
                        if phase_lock:
                            return pv_ops.phase_vocoder(spectrum, r.numerator, r.denominator, lock=True)
                        return pv_ops.phase_vocoder(spectrum, r.numerator, r.denominator)
                    if spectrum.size()[1] < 4:
                        audio.istft(spectrum)  # raises: nothing that short can be separated and overlap-added
                    if pv_ops.phase_vocoder_len(spectrum.size()[1], r.numerator, r.denominator) - 1 < nb_vec:
                        return None  # too short for one image: left out below, as the plain variant would be
                    if phase_lock:
                        return audio.functions.retime_preserving_transients(spectrum, r, phase_lock=True)
                    return audio.functions.retime_preserving_transients(spectrum, r)
                spectra += [retime(complex_values, r) for r in rates]
                if ratios:
                    mono = ops.pcm_to_mono(pcm) if sr == audio.SAMPLE_RATE else ops.resample_pcm(pcm, sr, audio.SAMPLE_RATE)
                    del pcm
                    for _, f in ratios:
                        shifted = ops.stft_1024(ops.resample_rows(mono[None, :], f.numerator, f.denominator)[0].contiguous())
                        spectra.append(retime(shifted, 1 / f))
                    del mono
            del complex_values
            for v_i, complex_values in enumerate(spectra):
                # create_dataset.py:41-42 skips files of fewer than nb_vec frames; a file of EXACTLY nb_vec frames has nb_vec - 1 phase
                # differences, i.e. no complete image either (the reference would write one degenerate (2, 512, 0) tensor for it)
                if complex_values is None or complex_values.size()[1] - 1 < nb_vec:
                    continue  # (a variant that is too short is left out in the same way)
                if component is not None:  # the last step in front of the codec, in the spectral domain
                    complex_values = audio.hpss(complex_values)[COMPONENTS.index(component)]
                both = audio.stft_to_stacked_phase_magn(complex_values, nb_vec=nb_vec)  # (S, 2, 512, nb_vec) float32, on the device
                n_files += v_i == 0
                tracks.append([idx, int(both.size()[0])])
                crcs = None
                if template is not None:
                    from . import ops
                    crcs = ops.crc32_of_float64(both)  # int64 [S] on the device; it travels with the samples, no host sync here
                produced = th.cuda.Event()
                produced.record()  # codec (+ CRC) of this file queued: the copy streams start behind it
                for c0 in range(0, both.size()[0], CHUNK_SAMPLES):
                    t2 = time.perf_counter()
                    chunk = ring.get()
                    t_wait += time.perf_counter() - t2
                    n = min(CHUNK_SAMPLES, both.size()[0] - c0)
                    chunk.acquire()  # held by this loop until everything that reads the chunk has been queued
                    cs = copy_streams[n_chunks % 2]
                    n_chunks += 1
                    with th.cuda.stream(cs):
                        cs.wait_event(produced)
                        chunk.host[:n].copy_(both[c0:c0 + n], non_blocking=True)
                        if crcs is not None:
                            chunk.crc[:n].copy_(crcs[c0:c0 + n], non_blocking=True)
                            crcs.record_stream(cs)
                        both.record_stream(cs)
                        chunk.event.record(cs)
                    r0 = 0
                    while r0 < n:
                        # a job = consecutive rows of this chunk inside ONE block of side-car rows (global row = len(names); rows in idx
                        # order == AudioDataset order only after the sort in _finish_sidecar)
                        g_row = len(names)
                        m = min(n - r0, _ds.PACKED_BLOCK_ROWS - g_row % _ds.PACKED_BLOCK_ROWS)
                        batch = [f"magn_phase_{idx + k}.pt" for k in range(m)]
                        fd, off = None, 0
                        if side is not None:
                            k_sh, local = _ds.shard_of_row(g_row, _ds.PACKED_SHARDS, _ds.PACKED_BLOCK_ROWS)
                            fd, off = side[k_sh], local * row_bytes
                        writers.submit(chunk, r0, [join(dataset_output_dir, b) for b in batch], fd, off,
                                       check_first=crcs is not None and c0 + r0 == 0)
                        names.extend(batch)
                        idx += m
                        r0 += m
                    chunk.release()
            t_gpu += time.perf_counter() - t1
        t_loader = loader.busy_s
        t_drain = time.perf_counter()
        writers.close()  # the writers finish what is queued
        t_drain = time.perf_counter() - t_drain
        ok = True
    finally:
        loader.close()
        if not ok:
            try:
                writers.close()
            except BaseException:  # noqa: BLE001  (the original error is the one to report)
                pass
        if side is not None:
            for fd in side:
                os.close(fd)
            if not ok:
                _remove_sidecar(dataset_output_dir)
    if side is not None:
        _finish_sidecar(dataset_output_dir, names, tracks)
    if stats is not None:
        wall = time.perf_counter() - t_start
        stats.update({"files": n_files, "samples": len(names), "wall_s": wall, "setup_s": t_setup, "drain_s": t_drain,
                      "load_stft_s": t_load, "loader_thread_busy_s": t_loader, "loader_threads": loader.workers,
                      "codec_copy_submit_s": t_gpu, "ring_wait_s": t_wait, "writer_threads": n_thr,
                      "writer_busy_s": writers.busy_s, "pt_bytes": len(names) * 2 * (audio.N_FFT // 2) * nb_vec * 8})


def _finish_sidecar(folder: str, names_in_write_order, tracks=None) -> None:
    """The rows were streamed in write order (idx 0, 1, 2, ...); AudioDataset / the loader index samples in file-NAME order
    (plain string sort, as the reference does: magn_phase_10.pt < magn_phase_2.pt).  The meta file carries the row of every
    sorted name, so the stream never has to be permuted on disk.  `tracks` (optional): [first_idx, count] per spectrum written, in
    the numbering of the file names -- runs of consecutive chunks of one spectrum, which the loaders cut shifted windows from
    (audio/dataset.py); recorded under "tracks" in the same meta file."""
    k = _ds.PACKED_SHARDS
    tmps = [join(folder, _ds.shard_name(i, k) + ".tmp") for i in range(k)]

    def drop():
        for t in tmps:
            try:
                os.remove(t)
            except FileNotFoundError:
                pass
    if not names_in_write_order:
        drop()
        return
    order = sorted(range(len(names_in_write_order)), key=lambda i: names_in_write_order[i])
    files = [names_in_write_order[i] for i in order]
    if tuple(files) != _ds._sample_files(folder):
        # the directory also holds magn_phase_*.pt files of an earlier, longer run: AudioDataset would serve them too (as the
        # reference's does), so no side-car describes this directory -- the loader then takes the reference path
        drop()
        return
    for i, t in enumerate(tmps):
        os.replace(t, join(folder, _ds.shard_name(i, k)))
    with open(join(folder, _ds.PACKED_META), "w") as fh:
        json.dump({"count": len(files), "shape": list(_ds._SAMPLE_SHAPE), "dtype": "float32", "files": files, "rows": order,
                   "shards": k, "block_rows": _ds.PACKED_BLOCK_ROWS,
                   "sizes": [os.path.getsize(join(folder, f)) for f in files],
                   "probes": [_ds.file_probe(join(folder, f)) for f in files],
                   **({"tracks": [[int(f), int(c)] for f, c in tracks]} if tracks is not None else {})}, fh)
