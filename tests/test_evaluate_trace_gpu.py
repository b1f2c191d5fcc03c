"""GPU: which dataset entries and which latent rows `evaluate` turns into images, in which batches and in which order.  The
generator's kernels are chosen by N * H * W, so a sample's bits may depend on the batch it was generated in: the sequence of
batches is part of what evaluate computes, and it is written out here as plain loops, metric by metric."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from eval_corpus import tiny_corpus  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB, SEED, CHANNELS = 8, 1, 8


def _expected(metrics, nb, bs, seed):
    """[("real", dataset indices) | ("fake", latent rows)], one entry per batch, in the order evaluate makes them"""
    nn_queries = sys.modules["musicgan_amd.evaluate"]._NN_QUERIES
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).tolist()
    half, nq = nb // 2, min(nb, nn_queries)
    calls = []

    def real(idx):
        calls.append(("real", list(idx)))

    def fake(rows):
        calls.append(("fake", list(rows)))

    if "swd" in metrics:
        for lo in range(0, nb, bs):
            real(range(lo, min(lo + bs, nb)))
            fake(range(lo, min(lo + bs, nb)))
    if "msssim" in metrics:
        first, second = perm[:half], perm[half:2 * half]
        for lo in range(0, half, bs):
            real(first[lo:lo + bs])
            real(second[lo:lo + bs])
            fake(first[lo:lo + bs])
            fake(second[lo:lo + bs])
    if "nn" in metrics:
        for lo in range(0, nq, bs):
            fake(range(lo, min(lo + bs, nb)))       # not clipped to nq: the concatenation is cut afterwards
        for lo in range(0, nq, bs):
            real(perm[lo:min(lo + bs, nq)])
        for lo in range(0, nb, bs):
            real(range(lo, min(lo + bs, nb)))       # one batch, fed to both searches
    if "prdc" in metrics:
        for lo in range(0, nb, bs):
            real(range(lo, min(lo + bs, nb)))
            fake(range(lo, min(lo + bs, nb)))
        for lo in range(0, half, bs):
            real(perm[lo:min(lo + bs, half)])
            real(perm[half + lo:min(half + lo + bs, 2 * half)])
    if "ndb" in metrics:
        for lo in range(0, half, bs):
            real(perm[lo:min(lo + bs, half)])
        for lo in range(0, half, bs):
            n = min(bs, half - lo)
            fake(range(lo, lo + n))
            real(perm[half + lo:half + lo + n])
    return calls


def test_evaluate_reads_and_generates_the_same_batches_in_the_same_order(tmp_path, capsys, monkeypatch):
    import musicgan_amd
    from musicgan_amd import audio, ops
    from musicgan_amd.networks import Generator
    evaluate = musicgan_amd.evaluate                                 # the function: the package binds it over the sub-module
    METRICS_EVERY = sys.modules["musicgan_amd.evaluate"].METRICS_EVERY
    data_dir, ck = tiny_corpus(tmp_path, 4, 6)
    cls = audio.PackedAudioDataset if audio.has_packed(data_dir) else audio.AudioDataset
    assert len(cls(data_dir)) == NB
    latents = torch.randn(NB, CHANNELS, 2, 2, device=DEV, generator=torch.Generator(device=DEV).manual_seed(SEED))
    calls, read = [], []
    getitem, transform, forward = cls.__getitem__, ops.input_transform, Generator.forward

    def traced_getitem(self, index):
        read.append(int(index))
        return getitem(self, index)

    def traced_transform(x, side):
        assert x.shape[0] == len(read), (tuple(x.shape), read)      # every entry read since the last real batch is in this one
        calls.append(("real", list(read)))
        read.clear()
        return transform(x, side)

    def traced_forward(self, z, alpha):
        same = (z[:, None] == latents[None]).flatten(2).all(2)       # (n, NB): which latent row is each row of the batch
        assert same.sum(1).tolist() == [1] * z.shape[0], same
        calls.append(("fake", same.int().argmax(1).tolist()))
        return forward(self, z, alpha)

    monkeypatch.setattr(cls, "__getitem__", traced_getitem)
    monkeypatch.setattr(ops, "input_transform", traced_transform)
    monkeypatch.setattr(Generator, "forward", traced_forward)

    def run(metrics, bs):
        """evaluate, held against the written-out sequence; (result, printed text)"""
        del calls[:], read[:]
        capsys.readouterr()
        result = evaluate(ck, CHANNELS, data_dir, metrics=metrics, level=2, nb_images=NB, batch_size=bs, seed=SEED)
        text = capsys.readouterr().out
        want = _expected(metrics, NB, bs, SEED)
        assert not read and len(calls) == len(want), (metrics, bs, len(calls), len(want))
        for i, (got, exp) in enumerate(zip(calls, want)):
            assert got == exp, (metrics, bs, i, got, exp)
        return result, text

    full, text_full = run(METRICS_EVERY, 3)
    run(METRICS_EVERY, 16)                                           # one batch per loop
    mixed, text_mixed = run(("ndb", "swd"), 3)                       # the order run is METRICS_EVERY's, not the order asked for
    single = {m: run((m,), 3) for m in METRICS_EVERY}

    header = "".join(text_full.splitlines(True)[:2])                 # "Load model...", "Evaluate 8 real and 8 generated ..."
    assert header.count("\n") == 2 and "Evaluate 8 real and 8 generated images of 16 x 16" in header
    assert all(text.startswith(header) for _, text in single.values())
    assert text_full == header + "".join(single[m][1][len(header):] for m in METRICS_EVERY)
    assert list(full) == [name for m in METRICS_EVERY for name in single[m][0]]
    assert full == {name: value for m in METRICS_EVERY for name, value in single[m][0].items()}
    assert text_mixed == header + single["swd"][1][len(header):] + single["ndb"][1][len(header):]
    assert list(mixed) == list(single["swd"][0]) + list(single["ndb"][0])
    assert mixed == {**single["swd"][0], **single["ndb"][0]}
