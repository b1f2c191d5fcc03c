"""No GPU: csrc/ogg_crc.h compiled for the host.  The page kernels of vorbis.hip and vorbis_encode.hip cut a page into one chunk per
lane, shift every chunk's CRC past the bytes behind it with a GF(2) multiply and xor the parts; here that arithmetic runs lane by
lane on the host against audio.vorbis.ogg_crc, the byte-serial definition."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from musicgan_amd.audio import vorbis as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 26, 27, 28, 255, 256, 257, 4096, 65307]     # 65307: the largest Ogg page; 1 .. 257 leave trailing lanes empty


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ogg_crc")
    shim = tmp / "shim.cpp"
    shim.write_text('#define OGG_HD static inline\n#include "ogg_crc.h"\n'
                    'extern "C" uint32_t lanes_xor(const uint8_t* p, long long len, int nlanes) { uint32_t T[256], x = 0;'
                    ' for (uint32_t i = 0; i < 256; ++i) T[i] = ogg::crc_table_entry(i);'
                    ' for (int l = 0; l < nlanes; ++l) x ^= ogg::page_crc_part(p, len, l, nlanes, T); return x; }\n'
                    'extern "C" uint32_t mulmod(uint32_t a, uint32_t b) { return ogg::gf2_mulmod(a, b); }\n'
                    'extern "C" uint32_t xpow8(long long k) { return ogg::xpow8(k); }\n')
    so = str(tmp / "shim.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "musicgan_amd", "csrc"), str(shim), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.lanes_xor.restype = lib.mulmod.restype = lib.xpow8.restype = ctypes.c_uint32
    lib.lanes_xor.argtypes = [ctypes.c_char_p, ctypes.c_longlong, ctypes.c_int]
    lib.mulmod.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.xpow8.argtypes = [ctypes.c_longlong]
    return lib


def test_lane_parts_xor_to_the_page_crc(lib):
    rng = np.random.default_rng(22)
    for length in LENGTHS:
        data = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        zeroed = bytearray(data)
        zeroed[22:26] = bytes(len(zeroed[22:26]))            # the page's own CRC field reads as zero
        want = V.ogg_crc(zeroed)
        for nlanes in (64, 256):
            assert lib.lanes_xor(data, length, nlanes) == want, (length, nlanes)


def test_multiplying_by_a_power_of_x_appends_zero_bytes(lib):
    data = np.random.default_rng(23).integers(0, 256, 257, dtype=np.uint8).tobytes()
    crc = V.ogg_crc(data)
    for k in (0, 1, 2, 255, 65307):
        assert lib.mulmod(crc, lib.xpow8(k)) == V.ogg_crc(data + bytes(k)), k
