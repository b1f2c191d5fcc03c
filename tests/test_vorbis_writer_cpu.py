"""CPU: the header parser (audio/vorbis.py) against streams tests/vorbis_writer.py writes from chosen parameters -- codewords,
VQ values (lookups 1 and 2, sequence_p), ordered and sparse lengths, floor posts and neighbours, residues, mappings, the packet
table and the granule trims all equal what the writer put in -- and the reader ending every written packet in its last byte."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vorbis_reader as R  # noqa: E402
import vorbis_writer as W  # noqa: E402
from musicgan_amd.audio import vorbis as V  # noqa: E402


def test_writer_codewords_follow_the_specification_example():
    lengths = [2, 4, 4, 4, 4, 2, 3, 3]
    assert [format(c, f"0{n}b") for c, n in zip(W.Book(lengths).codes, lengths)] == \
        ["00", "0100", "0101", "0110", "0111", "10", "110", "111"]


@pytest.mark.parametrize("ch,bs,rtype,submaps,coupling", [(1, (64, 512), 0, 1, []), (2, (256, 2048), 1, 1, [(0, 1)]),
                                                          (6, (512, 4096), 2, 2, [(0, 1), (2, 3), (4, 5), (0, 2)])])
def test_parser_reads_back_what_the_writer_wrote(ch, bs, rtype, submaps, coupling):
    rng = np.random.default_rng(ch)
    spec = W.random_spec(rng, ch, bs, rtype, submaps=submaps, coupling=coupling, sparse=True)
    pk = W.random_packets(spec, rng, 6)
    data = spec.stream([p for p, _ in pk], max_segments=3, start_trim=0, end_trim=5)
    vs = V.parse(data, "w")
    s = vs.setup
    assert (s.channels, s.blocksize) == (ch, bs)
    for got, want in zip(s.books, spec.books):
        assert (got.dims, got.entries, got.lengths, got.codes, got.lookup_type) == \
            (want.dims, want.entries, want.lengths, want.codes, want.lookup)
        assert (got.values is None) == (want.values is None)
        if want.values is not None:
            assert np.array_equal(got.values, want.values)
    assert any(b.lookup == 2 and b.seq for b in spec.books) and any(0 in b.lengths for b in spec.books)
    assert any(b.ordered for b in spec.books)
    for got, want in zip(s.floors, spec.floors):
        assert (got.X, got.order, got.low, got.high, got.multiplier) == (want.X, want.order, want.low, want.high, want.mult)
    for got, want in zip(s.residues, spec.residues):
        assert (got.type, got.begin, got.end, got.partition_size, got.books) == \
            (want.type, want.begin, want.end, want.partition_size, want.books)
    for got, want in zip(s.mappings, spec.mappings):
        assert (got.mux, got.magnitude, got.angle, got.submap_floor) == (want.mux, want.magnitude, want.angle, want.submap_floor)
    assert list(vs.pkt_len) == [len(p) for p, _ in pk]
    ns = [bs[b] for b in vs.pkt_blockflag]
    assert vs.frames == sum(ns[i - 1] // 4 + ns[i] // 4 for i in range(1, len(ns))) - 5
    _, ends = R.decode_file(data, return_ends=True, setup=spec.setup())
    for (bits, nbytes), (p, floor_end) in zip(ends, pk):
        assert 8 * (nbytes - 1) < bits <= 8 * nbytes and bits >= floor_end


def test_info_counts_what_the_decoder_returns(tmp_path):
    rng = np.random.default_rng(5)
    spec = W.random_spec(rng, 2, (256, 2048), 2)
    pk = [p for p, _ in W.random_packets(spec, rng, 8)]
    from musicgan_amd.audio import wavio
    for kw, eos in (({"end_trim": 100}, True), ({"start_trim": 0}, False)):
        data = spec.stream(pk, max_segments=4, **kw)
        if not eos:  # no EOS flag on the last page: every decoded frame is returned
            last = data.rfind(b"OggS")
            page = bytearray(data[last:])
            page[5] &= ~4
            page[22:26] = b"\0\0\0\0"
            page[22:26] = V.ogg_crc(bytes(page)).to_bytes(4, "little")
            data = data[:last] + bytes(page)
        p = tmp_path / "i.ogg"
        p.write_bytes(data)
        assert wavio.info(str(p))[0] == V.parse(data, "i").frames == R.decode_file(data, setup=spec.setup()).shape[0]
