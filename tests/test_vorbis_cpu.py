"""CPU: Ogg Vorbis headers, codebooks and refusals (audio/vorbis.py), and the float64 reference reader against the fixture
(tests/golden/invalid_keypress.ogg, from MathJax 2.x, Apache-2.0: see tests/golden/NOTICE)."""
import hashlib
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vorbis_reader  # noqa: E402
import vorbis_writer as W  # noqa: E402
from musicgan_amd.audio import vorbis as V  # noqa: E402
from musicgan_amd.audio import wavio  # noqa: E402


def test_fixture_header_facts():
    data = W.fixture_bytes()
    assert len(data) == 5353 and hashlib.md5(data).hexdigest() == "32a420467788f3f7a4bb277cc3404f1a"
    vs = V.parse(data, W.FIXTURE)
    s = vs.setup
    assert (s.channels, s.rate, s.bitrate_nominal, s.bitrate_max, s.bitrate_min) == (2, 44100, 112000, 0, 0)
    assert s.vendor == "Xiph.Org libVorbis I 20070622" and s.blocksize == (256, 2048)
    assert len(vs.pages.offset) == 3 and len(vs.pkt_len) == 26
    assert vs.pages.flags[-1] & 4 and vs.pages.granule[-1] == 22050
    assert len(s.books) == 38
    assert sorted({b.lookup_type for b in s.books}) == [0, 1] and sorted({b.dims for b in s.books}) == [1, 2, 4, 8]
    assert s.floor_types == [1, 1] and [r.type for r in s.residues] == [2, 2]
    assert [(len(m.submap_floor), m.magnitude, m.angle) for m in s.mappings] == [(1, [0], [1])] * 2
    assert s.modes == [(0, 0), (1, 1)]
    heads, audio, _ = W.fixture_packets()
    assert s.setup_bits == 30650 and 8 * len(heads[2]) == 30656  # the 30 651st of 30 656 bits
    assert list(vs.pkt_blockflag) == [0] * 4 + [1] * 22
    flags = [(p[0] >> 2) & 3 for p in audio[4:]]  # after the packet type and 1 mode bit: previous, next window flags
    assert flags[0] == 0b10 and all(f == 0b11 for f in flags[1:])
    assert sum(len(p) == 1 for p in audio) == 12
    assert vs.returned == 22464 and vs.frames == 22050 and vs.trim_start == 0


def test_info_without_a_gpu():
    assert wavio.info(W.FIXTURE) == (22050, 2, 44100, 0)


def test_codeword_assignment_example():
    codes = V.make_codewords([2, 4, 4, 4, 4, 2, 3, 3])
    assert [format(c, f"0{ln}b") for c, ln in zip(codes, [2, 4, 4, 4, 4, 2, 3, 3])] == \
        ["00", "0100", "0101", "0110", "0111", "10", "110", "111"]
    assert V.make_codewords([0, 1, 0, 1]) == [None, 0, None, 1]
    with pytest.raises(ValueError):
        V.make_codewords([1, 1, 1])


def test_float32_unpack_and_lookup1_values():
    assert V.lookup1_values(81, 4) == 3 and V.lookup1_values(80, 4) == 2 and V.lookup1_values(625, 4) == 5
    assert V.lookup1_values(624, 4) == 4 and V.lookup1_values(1, 1) == 1 and V.lookup1_values(256, 8) == 2
    # mantissa 1, exponent 788: 1.0; sign bit; exponent 788 - 20 with mantissa 2^20: 1.0 again
    assert V.float32_unpack(1 | (788 << 21)) == 1.0
    assert V.float32_unpack(0x80000000 | 3 | (788 << 21)) == -3.0
    assert V.float32_unpack((1 << 20) | (768 << 21)) == 1.0
    assert V.float32_unpack(0) == 0.0


def test_header_page_crcs_match():
    data = np.frombuffer(W.fixture_bytes(), np.uint8)
    pages = V.walk_pages(data, "f")
    for i in range(len(pages.offset)):
        assert V.page_crc_ok(data, pages, i)
    assert V.ogg_crc(b"") == 0 and V.ogg_crc(b"\x01") == 0x04C11DB7


def test_reader_ends_every_packet_in_its_last_byte():
    pcm, ends = vorbis_reader.decode_file(W.fixture_bytes(), return_ends=True)
    assert pcm.shape == (22050, 2)
    for k, (bits, nbytes) in enumerate(ends):
        assert 8 * (nbytes - 1) < bits <= 8 * nbytes, (k, bits, nbytes)


def _ogg_page(body, flags=2, granule=0, serial=1):
    hdr = b"OggS" + bytes([0, flags]) + struct.pack("<qII", granule, serial, 0) + b"\0\0\0\0" + bytes([1]) + bytes([len(body)])
    crc = V.ogg_crc(hdr + body)
    return hdr[:22] + struct.pack("<I", crc) + hdr[26:] + body


def test_refusals_name_the_file(tmp_path):
    def refuse(data, match, name="x.ogg"):
        p = tmp_path / name
        p.write_bytes(data)
        with pytest.raises(ValueError, match=match) as e:
            wavio.load_pcm(str(p))
        assert str(p) in str(e.value)

    refuse(b"RIFF" + bytes(60), "not an Ogg")
    refuse(_ogg_page(b"OpusHead" + bytes(11)), "Opus")
    refuse(_ogg_page(b"\x7fFLAC" + bytes(40)), "FLAC")
    refuse(_ogg_page(b"Speex   " + bytes(72)), "Speex")
    refuse(_ogg_page(b"\x80theora" + bytes(40)), "Theora")
    data = W.fixture_bytes()
    # chained: the stream twice, the second with another serial number
    heads, audio, _ = W.fixture_packets()
    second = W.paginate(heads + audio[:4], [0, 0, 0, 0, 128, 256, 384], serial=99)
    refuse(data + second, "logical streams")
    # a header page CRC mismatch
    bad = bytearray(data)
    bad[40] ^= 1
    refuse(bytes(bad), "CRC")
    # a bad setup header: its sync pattern broken (the CRC recomputed so the header parse sees it)
    vs = V.parse(data, "f")
    body = bytearray(data[int(vs.pages.body[1]):int(vs.pages.body[1] + vs.pages.body_len[1])])
    i = body.find(b"\x05vorbis")
    body[i + 8] ^= 0xFF
    hdr = bytearray(data[int(vs.pages.offset[1]):int(vs.pages.body[1])])
    hdr[22:26] = b"\0\0\0\0"
    hdr[22:26] = struct.pack("<I", V.ogg_crc(bytes(hdr) + bytes(body)))
    refuse(data[:int(vs.pages.offset[1])] + bytes(hdr) + bytes(body) + data[int(vs.pages.offset[2]):], "setup header")
    # more than 8 channels; a missing setup header
    ident = bytearray(heads[0])
    ident[11] = 9
    refuse(W.paginate([bytes(ident)] + heads[1:] + audio, [0, 0, 0] + [0] * len(audio)), "9 channels")
    refuse(W.paginate(heads[:2], [0, 0]), "missing Vorbis header")
    # floor type 0: a setup header whose first floor says type 0 (written by hand: one codebook, one floor)
    refuse(W.paginate(heads[:2] + [_setup_with_floor0()], [0, 0, 0]), "floor type 0")
    # a truncated last page
    refuse(data[:-10], "truncated")


def _setup_with_floor0():
    bits = []

    def put(v, n):
        bits.extend((v >> i) & 1 for i in range(n))

    put(0, 8)                 # one codebook
    put(0x564342, 24)
    put(1, 16)                # dims
    put(2, 24)                # entries
    put(0, 1)                 # not ordered
    put(0, 1)                 # not sparse
    put(0, 5)                 # length 1
    put(0, 5)
    put(0, 4)                 # lookup 0
    put(0, 6)                 # one time-domain value
    put(0, 16)
    put(0, 6)                 # one floor
    put(0, 16)                # type 0
    put(0, 64)
    bits.extend([0] * (-len(bits) % 8))
    body = bytes(sum(b << i for i, b in enumerate(bits[k:k + 8])) for k in range(0, len(bits), 8))
    return b"\x05vorbis" + body


def test_existing_refusals_unchanged(tmp_path):
    ogg_flac = tmp_path / "ogg.flac"
    ogg_flac.write_bytes(b"OggS" + bytes(60))
    with pytest.raises(ValueError, match="Ogg"):
        wavio.load_pcm(str(ogg_flac))
    mp3 = tmp_path / "x.mp3"
    mp3.write_bytes(b"ID3" + bytes(60))
    with pytest.raises(ValueError, match="mp3"):
        wavio.load(str(mp3))


def test_valid_vorbis_without_a_gpu_raises_hip_error(monkeypatch):
    import torch
    from musicgan_amd._lib import MusicGanHipError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(MusicGanHipError):
        wavio.load(W.FIXTURE)
