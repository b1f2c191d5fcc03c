"""GPU: Ogg Vorbis encoding (csrc/vorbis_encode.hip) -- exact frame counts through wavio.save / load, the product decoder and the
float64 reader (tests/vorbis_reader.py) agreeing on the encoder's bytes, Ogg framing, the per-bin quantisation bound against the
test's float64 MDCT, silence, quality, determinism, errors, and the public paths: magn_phase_to_wav, generate, create_dataset."""
import os
import sys

import numpy as np
import pytest
import torch

import vorbis_reader as R
from musicgan_amd.audio import vorbis as V
from musicgan_amd.audio import vorbis_encode as VE
from test_vorbis_encode_cpu import mdct_blocks

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_flac import music  # noqa: E402  (the benchmark's music-like signal)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SNR_MARGIN_DB = 3.0  # SNR of the music-like signal at quality 3 is at least S(3) minus this


def encode(x, rate=44100, quality=3.0):
    """(frames, channels) -> file bytes"""
    from musicgan_amd import ops
    return ops.vorbis_encode(torch.from_numpy(np.ascontiguousarray(np.asarray(x).T)), rate, quality).numpy().tobytes()


def decode(data):
    from musicgan_amd import ops
    vs = V.parse(data, "<enc>")
    return ops.vorbis_decode(torch.frombuffer(bytearray(data), dtype=torch.uint8).to(DEV), vs).cpu().numpy().astype(np.float64)


def snr_db(x, y):
    return 10 * np.log10(np.sum(x ** 2) / max(np.sum((x - y) ** 2), 1e-300))


def tones(n, ch, seed=0, amp=0.5):
    """harmonic tones plus noise 30 dB down, channels correlated"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    base = sum(np.sin(2 * np.pi * 220 * h * t + h) / h for h in range(1, 8))
    x = np.stack([base * (0.6 + 0.1 * c) + 0.3 * np.sin(2 * np.pi * (330 + 40 * c) * t) for c in range(ch)], 1)
    x = amp * x / np.abs(x).max()
    return x + rng.standard_normal((n, ch)) * amp * 10 ** (-30 / 20) / 3


def signals(n=8 * 1024 + 300):
    t = np.arange(n)
    xs = V.parse(VE.header_pages(1, 44100)[0] + VE.ogg_page(b"\x0e", [1], 0, 2, 4), "x").setup.floors[0].X
    s = sorted(xs)
    mid = (s[20] + s[21]) / 2  # a bin midway between two neighbouring posts
    rng = np.random.default_rng(5)
    return {
        "tones": tones(n, 2),
        "between_posts": np.stack([np.sin(np.pi * (mid + 0.5) / 1024 * t), np.cos(np.pi * (mid + 0.5) / 1024 * t)], 1),
        "impulse": np.stack([(t == 3000).astype(float), (t == 5000).astype(float) * 0.7], 1),
        "noise": rng.uniform(-1, 1, (n, 2)),
        "square": np.stack([np.sign(np.sin(2 * np.pi * 441 * t / 44100))] * 2, 1) * 0.999,
        "loud": tones(n, 2, seed=2, amp=4.0),
    }


@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("n", [1, 1000, 1024, 1025, 3 * 44100, 60 * 44100])
def test_round_trip_frame_count(tmp_path, ch, rate, n):
    from musicgan_amd.audio import wavio
    if n == 60 * 44100 and (ch, rate) != (2, 44100):
        n = 60 * rate if ch == 1 else 20 * rate
    x = tones(n, ch, seed=n % 97)
    for ext in (".ogg", ".oga"):
        path = str(tmp_path / f"x{ext}")
        wavio.save(path, torch.from_numpy(x.T.copy()).float(), rate)
        y, sr = wavio.load(path)
        assert sr == rate and tuple(y.shape) == (ch, n), (ext, tuple(y.shape))
        assert wavio.info(path)[:3] == (n, ch, rate)
        if n >= 4096:
            assert snr_db(x, y.numpy().T.astype(np.float64)) > VE.s_db(3) - SNR_MARGIN_DB


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_two_decoders_agree_and_pages_are_valid(ch):
    n = 6 * 1024 + 77
    x = tones(n, ch, seed=ch)
    data = encode(x)
    a = decode(data)
    b = R.decode_file(data)
    assert a.shape == b.shape == (n, ch)
    assert np.abs(a - b).max() <= 1e-5 * max(np.abs(b).max(), 1e-3)
    vs = V.parse(data, "<enc>")
    raw = np.frombuffer(data, np.uint8)
    pages = vs.pages
    assert all(V.page_crc_ok(raw, pages, i) for i in range(len(pages.offset)))
    bos, eos = pages.flags & 2, pages.flags & 4
    assert bos[0] and not bos[1:].any() and eos[-1] and not eos[:-1].any()
    g = pages.granule[vs.header_pages:]
    g = g[g >= 0]
    assert np.all(np.diff(g) >= 0) and int(pages.granule[-1]) == n
    assert len(vs.pkt_len) == -(-n // 1024) + 1 and np.all(vs.pkt_blockflag == 1)
    assert np.all(pages.serial == VE.SERIAL) and list(pages.offset[:1]) == [0]


def _floor_curves(pkt, setup, maps):
    """per channel the floor F = dB[curve] the packet's floors give (None: unused)"""
    br = R.Bits(pkt)
    br.read(1)
    br.read(V.ilog(len(setup.modes) - 1))
    br.read(2)
    db = V.inverse_db_table()
    out = []
    for _ in range(setup.channels):
        Y = R._decode_floor(br, setup.floors[0], maps)
        out.append(None if Y is None else db[R.floor1_curve(setup.floors[0], Y, 1024)])
    return out


@pytest.mark.parametrize("name", ["tones", "between_posts", "impulse", "noise", "square", "loud"])
def test_quantisation_bound(name):
    x = signals()[name]
    data = encode(x)
    vs = V.parse(data, "<enc>")
    setup = vs.setup
    maps = R._code_maps(setup)
    X = mdct_blocks(x)
    bound_energy, used_bins = 0.0, 0
    for k in range(len(vs.pkt_len)):
        pkt = V.packet_bytes(data, vs, k)
        spec = R.decode_packet(pkt, setup, maps, want_spectrum=True)[3]
        for c, F in enumerate(_floor_curves(pkt, setup, maps)):
            if F is None:
                assert np.all(spec[c] == 0)
                continue
            slack = 1e-5 * np.abs(X[k, c]).max() + 1e-6 * F
            err = np.abs(X[k, c] - spec[c])
            assert np.all(err <= F / 2 + slack), (name, k, c, int(np.argmax(err - F / 2)))
            bound_energy += np.sum((F / 2) ** 2)
            used_bins += 1
    assert used_bins > 0
    # time domain: the error energy is within what the per-bin bound allows (Parseval for the TDAC frame: |x|^2 ~ n/4 |X|^2 / ...)
    y = decode(data)
    e = np.sum((x - y) ** 2)
    assert e <= 1024 / 2 * bound_energy * 1.01 + 1e-9, (name, e, bound_energy)


def test_silence_is_exact_and_small():
    n = 44100
    data = encode(np.zeros((n, 2)))
    head = len(VE.header_pages(2, 44100)[0])
    assert len(data) - head < 400, len(data) - head
    assert np.array_equal(decode(data), np.zeros((n, 2)))
    x = tones(n, 2)
    x[:, 1] = 0
    y = decode(encode(x))
    assert np.array_equal(y[:, 1], np.zeros(n)) and snr_db(x[:, 0], y[:, 0]) > VE.s_db(3) - SNR_MARGIN_DB
    x = tones(n, 2)
    x[:, 0] = 0
    y = decode(encode(x))
    assert np.array_equal(y[:, 0], np.zeros(n)) and snr_db(x[:, 1], y[:, 1]) > VE.s_db(3) - SNR_MARGIN_DB


def test_quality_orders_size_and_snr():
    from musicgan_amd import ops
    pcm = music(10 * 44100)
    x = pcm / 32768.0
    sizes, snrs = [], []
    for q in (-1, 0, 3, 6, 10):
        data = encode(x, quality=q)
        sizes.append(len(data))
        snrs.append(snr_db(x, decode(data)))
    print("sizes", sizes, "snr", [round(s, 2) for s in snrs])
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(a < b for a, b in zip(snrs, snrs[1:]))
    flac = ops.flac_encode(torch.from_numpy(pcm.T.astype(np.int16).copy()), 44100).numel()
    assert sizes[2] < flac, (sizes[2], flac)
    assert snrs[2] >= VE.s_db(3) - SNR_MARGIN_DB


def test_deterministic_and_layouts():
    from musicgan_amd import ops
    x = tones(20000, 2)
    a = encode(x)
    assert encode(x) == a
    t = torch.from_numpy(x.T.copy())
    assert ops.vorbis_encode(t.to(DEV), 44100).numpy().tobytes() == a  # float64 on the device
    assert ops.vorbis_encode(torch.from_numpy(x.copy()).T, 44100).numpy().tobytes() == a  # a transposed view
    i16 = torch.from_numpy(np.round(x.T * 20000).astype(np.int16))
    y = decode(ops.vorbis_encode(i16, 44100).numpy().tobytes())
    assert snr_db(i16.numpy().T / 32768.0, y) > VE.s_db(3) - SNR_MARGIN_DB


def test_non_finite_and_too_loud_raise_and_write_nothing(tmp_path):
    from musicgan_amd.audio import wavio
    x = torch.zeros(2, 5000)
    x[1, 1234] = float("nan")
    x[0, 4000] = float("inf")
    path = str(tmp_path / "x.ogg")
    with pytest.raises(ValueError, match="sample 4000 of channel 0"):  # the first in channel-major order
        wavio.save(path, x, 44100)
    assert not os.path.exists(path)
    with pytest.raises(ValueError, match="too loud"):
        wavio.save(path, torch.full((1, 5000), 1000.0), 44100)
    assert not os.path.exists(path)


def test_magn_phase_to_wav_writes_ogg(tmp_path):
    from musicgan_amd import audio
    from musicgan_amd.audio import wavio
    from golden_util import load
    mp = torch.from_numpy(load("audio_codec.npz")["inv_in"]).to(DEV)
    audio.magn_phase_to_wav(mp, str(tmp_path / "x.wav"), 44100)
    audio.magn_phase_to_wav(mp, str(tmp_path / "x.ogg"), 44100)
    assert (tmp_path / "x.ogg").read_bytes()[:4] == b"OggS"
    w, _ = wavio.load(str(tmp_path / "x.wav"))
    o, sr = wavio.load(str(tmp_path / "x.ogg"))
    assert sr == 44100 and o.shape == w.shape
    assert snr_db(w.numpy().astype(np.float64), o.numpy().astype(np.float64)) > VE.s_db(3) - SNR_MARGIN_DB - 6


def test_generate_ogg_matches_the_wav_run(tmp_path):
    import musicgan_amd
    from musicgan_amd.audio import wavio
    from musicgan_amd.networks import Generator
    torch.manual_seed(0)
    g7 = Generator(8, end_layer=7)
    ck = str(tmp_path / "gen7.pt")
    torch.save(g7.state_dict(), ck)
    torch.manual_seed(21)
    musicgan_amd.generate(str(tmp_path / "w"), 8, ck, 1, 2)
    torch.manual_seed(21)
    musicgan_amd.generate(str(tmp_path / "o"), 8, ck, 1, 2, audio_format="ogg")
    assert sorted(os.listdir(tmp_path / "o")) == ["sound_0.ogg", "sound_1.ogg"]
    for i in range(2):
        w, sr = wavio.load(str(tmp_path / "w" / f"sound_{i}.wav"))
        o, sr2 = wavio.load(str(tmp_path / "o" / f"sound_{i}.ogg"))
        assert sr == sr2 == 44100 and o.shape == w.shape
        assert snr_db(w.numpy().astype(np.float64), o.numpy().astype(np.float64)) > VE.s_db(3) - SNR_MARGIN_DB - 6, i


def test_create_dataset_reads_encoded_ogg(tmp_path, monkeypatch):
    import glob
    import musicgan_amd
    from musicgan_amd.audio import wavio
    (tmp_path / "ogg").mkdir()
    for i, n in enumerate((256 * 1100, 256 * 530)):
        wavio.save(str(tmp_path / "ogg" / f"f{i}.ogg"), torch.from_numpy(music(n, seed=i).T / 32768.0).float(), 44100)
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    musicgan_amd.create_dataset(str(tmp_path / "ogg" / "*.ogg"), str(tmp_path / "out"))
    assert len(glob.glob(str(tmp_path / "out" / "*"))) >= 2
