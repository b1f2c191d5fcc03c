"""CPU: Ogg Vorbis encoding's host side (audio/vorbis_encode.py) -- argument checks, no file without a GPU, the headers read back by
audio/vorbis.py, complete codebooks that cover the floor values and the residue range, a setup independent of quality, and the
test-side float64 forward MDCT (the oracle of tests/test_vorbis_encode_gpu.py) inverted by tests/vorbis_reader.py exactly."""
import os

import numpy as np
import pytest
import torch

import vorbis_reader as R
from musicgan_amd.audio import vorbis as V
from musicgan_amd.audio import vorbis_encode as VE

N2 = 1024


def mdct_blocks(x):
    """(frames, channels) float64 -> (packets, channels, 1024): the forward MDCT of every block the encoder writes (block k covers
    samples 1024 k - 1024 .. 1024 k + 1023, zero outside), X_k = 4 / n sum_i w_i x_i cos(2 pi / n (i + 1/2 + n/4)(k + 1/2))"""
    x = np.asarray(x, dtype=np.float64)
    n, ch = x.shape
    P = -(-n // N2) + 1
    pad = np.zeros(((P + 1) * N2, ch))
    pad[N2:N2 + n] = x
    w = R.window(2 * N2, VE.BLOCKSIZES, 1, 1, 1)
    i = np.arange(2 * N2)[None, :]
    k = np.arange(N2)[:, None]
    C = np.cos(2 * np.pi / (2 * N2) * (i + 0.5 + N2 / 2) * (k + 0.5)) * (4.0 / (2 * N2))
    blocks = np.stack([pad[N2 * p:N2 * p + 2 * N2] for p in range(P)])  # (P, 2048, ch)
    return np.einsum("ki,pic->pck", C, blocks * w[None, :, None])


def _no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


@pytest.mark.parametrize("ext", [".ogg", ".oga", ".OGG"])
def test_save_ogg_without_gpu_raises_and_writes_nothing(tmp_path, monkeypatch, ext):
    from musicgan_amd._lib import MusicGanHipError
    from musicgan_amd.audio import wavio
    _no_gpu(monkeypatch)
    path = str(tmp_path / f"x{ext}")
    with pytest.raises(MusicGanHipError, match="GPU"):
        wavio.save(path, torch.zeros(1, 1000), 44100)
    assert not os.path.exists(path)


@pytest.mark.parametrize("kwargs, match", [
    (dict(compression=-1.5), "compression|quality"), (dict(compression=10.5), "compression|quality"),
    (dict(compression="high"), "compression|quality"), (dict(bits_per_sample=16), "bits_per_sample"),
])
def test_argument_errors(tmp_path, kwargs, match):
    from musicgan_amd.audio import wavio
    path = str(tmp_path / "x.ogg")
    with pytest.raises(ValueError, match=match):
        wavio.save(path, torch.zeros(2, 100), 44100, **kwargs)
    assert not os.path.exists(path)


def test_compression_only_for_ogg(tmp_path):
    from musicgan_amd.audio import wavio
    for name in ("x.wav", "x.flac"):
        with pytest.raises(ValueError, match="compression"):
            wavio.save(str(tmp_path / name), torch.zeros(1, 100), 44100, compression=3)
        assert not os.path.exists(tmp_path / name)


@pytest.mark.parametrize("wav, match", [
    (torch.zeros(9, 100), "channels"), (torch.zeros(2, 3, 100), "shape"), (torch.zeros(2, 100, dtype=torch.int32), "int16"),
    (torch.zeros(2, 0), "no samples"), ([0.0] * 10, "tensor"),
])
def test_bad_input_raises(tmp_path, wav, match):
    from musicgan_amd import ops
    from musicgan_amd.audio import wavio
    with pytest.raises(ValueError, match=match):
        ops.vorbis_encode_args(wav, 44100)
    with pytest.raises(ValueError, match=match):
        wavio.save(str(tmp_path / "x.ogg"), wav, 44100)
    assert not os.path.exists(tmp_path / "x.ogg")


def test_good_arguments_pass():
    from musicgan_amd import ops
    x, q = ops.vorbis_encode_args(torch.zeros(1000), 48000, None)
    assert tuple(x.shape) == (1, 1000) and q == 3.0
    assert ops.vorbis_encode_args(torch.zeros(8, 5, dtype=torch.int16), 8000, -1)[1] == -1.0
    assert ops.vorbis_encode_args(torch.zeros(2, 5, dtype=torch.float64), 96000, 10)[1] == 10.0


def _stream(ch, rate=44100):
    """the header pages and one 1-byte audio packet (a silent long block), so the product parser reads a whole stream"""
    head, n = VE.header_pages(ch, rate)
    return head + VE.ogg_page(bytes([0x0E]), [1], 0, n, 4), n


@pytest.mark.parametrize("ch", [1, 2, 3, 6, 8])
def test_headers_parse_and_pack(ch):
    data, nhead = _stream(ch, 48000)
    vs = V.parse(data, "x.ogg")
    s = vs.setup
    assert (s.channels, s.rate, s.blocksize) == (ch, 48000, (256, 2048))
    assert s.vendor == VE.VENDOR.decode() and s.comments == []
    assert s.modes == [(0, 0), (1, 0)] and len(s.mappings) == 1
    assert s.mappings[0].magnitude == ([0] if ch == 2 else []) and s.mappings[0].angle == ([1] if ch == 2 else [])
    f = s.floors[0]
    assert len(f.X) == VE.NPOSTS <= V.MAX_POSTS and f.multiplier == 2 and f.rangebits == 10
    r = s.residues[0]
    assert (r.type, r.begin, r.end, r.partition_size, r.classifications) == (2, 0, 1024 * ch, 16, 6)
    pages = vs.pages
    assert pages.flags[0] == 2 and pages.body_len[0] == 30 and all(int(g) == 0 for g in pages.granule[:nhead])
    assert all(V.page_crc_ok(np.frombuffer(data, np.uint8), pages, i) for i in range(len(pages.offset)))
    ints, floats = V.pack_setup(s)
    assert ints.dtype == np.int32 and len(floats) > 0


def test_codebooks_are_complete_and_cover_the_ranges():
    s = V.parse(_stream(2)[0], "x.ogg").setup
    for i, b in enumerate(s.books):
        assert sum(2.0 ** -ln for ln in b.lengths) == 1.0, i
        assert min(b.lengths) >= 1 and max(b.lengths) <= VE.MAXLEN, i
    # every floor `val` (0 .. range - 1) has a codeword, in every partition class and subclass
    f = s.floors[0]
    for c in set(f.partition_class):
        for book in f.subclass_books[c]:
            assert s.books[book].entries >= VE.RANGE and all(s.books[book].lengths[:VE.RANGE])
    # the residue books: class c codes every vector of values within its bound; class 5 (two passes) every value to QMAX_CODED
    r = s.residues[0]
    bounds = [0, 1, 2, 4, 8]
    for c in range(1, 5):
        book = s.books[r.books[c][0]]
        vals = {tuple(v) for v in book.values.astype(int)}
        grid = np.array(np.meshgrid(*[np.arange(-bounds[c], bounds[c] + 1)] * book.dims)).reshape(book.dims, -1).T
        assert all(tuple(v) in vals for v in grid), c
        assert all(x < 0 for x in r.books[c][1:]), c
    coarse, fine = s.books[r.books[5][0]], s.books[r.books[5][1]]
    sums = {int(a + b) for a in coarse.values[:, 0] for b in fine.values[:, 0]}
    assert set(range(-VE.QMAX_CODED, VE.QMAX_CODED + 1)) <= sums
    assert VE.QMAX_CODED >= 2 * VE.QMAX  # a coupled angle reaches twice a channel's bound
    assert r.books[0] == [-1] * 8


def test_setup_is_independent_of_quality_and_calls():
    a = VE._Setup(2).setup_packet
    VE._SETUPS.clear()
    VE._HEADERS.clear()
    b = VE.setup_for(2).setup_packet
    assert a == b and VE.header_pages(2, 44100) == VE.header_pages(2, 44100)
    assert VE.setup_for(1).setup_packet != b  # the residue's end and the coupling differ with the channel count
    # quality enters through S(q) alone, monotone
    qs = np.linspace(-1, 10, 23)
    assert np.all(np.diff([VE.s_db(q) for q in qs]) > 0)


def test_float_pack_and_book_values():
    s = V.parse(_stream(1)[0], "x.ogg").setup
    coarse = s.books[s.residues[0].books[5][0]]
    assert np.array_equal(coarse.values[:, 0], 17.0 * np.arange(-15, 16))
    assert V.float32_unpack(VE._f32pack(-255)) == -255.0 and V.float32_unpack(VE._f32pack(17)) == 17.0


@pytest.mark.parametrize("n", [1, 700, 1024, 1025, 5000])
def test_forward_mdct_oracle_inverts_through_the_reader(n):
    """the test's float64 MDCT, then the reader's IMDCT, window and overlap-add, returns the input (TDAC): pins the oracle"""
    rng = np.random.default_rng(n)
    x = rng.standard_normal((n, 2))
    X = mdct_blocks(x)
    P = X.shape[0]
    assert P == -(-n // N2) + 1
    w = R.window(2 * N2, VE.BLOCKSIZES, 1, 1, 1)
    full = np.zeros(((P + 1) * N2, 2))
    for p in range(P):
        for c in range(2):
            full[N2 * p:N2 * p + 2 * N2, c] += R.imdct(X[p, c]) * w
    np.testing.assert_allclose(full[N2:N2 + n], x, rtol=0, atol=1e-12 * np.abs(x).max())


def test_generate_parser_takes_format_ogg():
    from musicgan_amd.__main__ import build_parser
    a = build_parser().parse_args(["generate", "gen.pt", "32", "-o", "o", "--format", "ogg"])
    assert a.audio_format == "ogg"


def test_encoder_kernels_use_no_scratch():
    from musicgan_amd import _build
    _build.build()
    usage = {k: v for k, v in _build.resource_usage().items() if "venc_" in k}
    assert len(usage) == 7, sorted(usage)
    for name, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, name
