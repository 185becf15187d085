"""Support for the lzip write tests: the named inputs of the device tests (shared with the recorded digests of
tests/golden/lzip_write_digests.json), the checks every written image has to pass, and the CPU stand-in of
tests/mock_gpu/la_gpu_lzip_comp_mock.c, which compiles the kernels' own rules header and therefore writes the device's bytes."""
import ctypes as C
import functools
import hashlib
import json
import os
import struct
import zlib

import lzip_support as LS
import mock_build
import xz_write_support as XW

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "lzip_write_digests.json")
M, BIG = 1 << 16, 1 << 18
LEVELS = (6, 9)         # one of each group: levels 0..6 write the same bytes, and so do 7..9
EVENTS = XW.EVENTS + ["marker"]
big_text, noise, filler, marker, planted = XW.big_text, XW.noise, XW.filler, XW.marker, XW.planted


def member_bytes(level):
    """the table of la_lzip_enc_dev.h"""
    return M if level <= 6 else BIG


def dict_byte(level):
    return 0x10 if level <= 6 else 0x12


def bound(n, level):
    """the header's arithmetic: 7 m + 64 stream bytes and 26 of framing per member of m input bytes"""
    m = member_bytes(level)
    full, rest = divmod(n, m)
    return full * (7 * m + 64 + 26) + ((7 * rest + 64 + 26) if rest or n == 0 else 0)


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes, at most 2 MiB"""
    t = big_text()
    far = bytearray(filler(51, BIG))
    far[1000:1040] = marker(6)
    far[201000:201040] = marker(6)
    return {
        "empty": b"", "one_byte": b"x", "m_minus_1": t[:M - 1], "m": t[:M], "m_plus_1": t[:M + 1],
        "three_m_plus_5": t[:3 * M + 5],
        "noise_2m5": noise(21, 2 * M + 5),
        "text_noise_text": t[:M] + noise(22, M) + t[M:2 * M],
        "run_3m": b"\x07" * (3 * M),
        "planted": planted()[0],
        "big_m_plus_1": t[:BIG + 1],
        "far_pair": bytes(far),
        "text_2mib": t[:2 << 20],
    }


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def digest(blob):
    return {"size": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}


def walk(img):
    """the members of an image, from the trailers: the last eight bytes of a member are its size, so the sizes have to
    chain from the image's end exactly to its start"""
    out, end = [], len(img)
    assert end >= 26
    while end > 0:
        assert end >= 26, end
        crc, data_size, member_size = struct.unpack_from("<IQQ", img, end - 20)
        start = end - member_size
        assert member_size >= 26 and start >= 0 and img[start:start + 4] == b"LZIP", (end, member_size)
        out.append({"off": start, "version": img[start + 4], "dict_byte": img[start + 5], "stream": img[start + 6:end - 20], "crc": crc,
                    "data_size": data_size, "member_size": member_size})
        end = start
    return out[::-1]


def accept(img, data, level):
    """what every written image has to pass: the reference's read loop over liblzma returns the input, whole and 4 096
    bytes at a time; the members are version 1 with the level's dictionary byte, cut the data every member_bytes(level),
    chain exactly to the image's end and carry the CRC32 of their piece; each raw stream alone decodes to its piece,
    ends at the marker and has no byte behind it; the image is within the bound."""
    for read_size in (None, 4096):
        assert LS.reference_read(img, read_size) == (data, 0, "")
    ms, m = walk(img), member_bytes(level)
    assert [x["version"] for x in ms] == [1] * len(ms) and [x["dict_byte"] for x in ms] == [dict_byte(level)] * len(ms)
    pieces = [data[o:o + m] for o in range(0, len(data), m)] or [b""]
    assert [x["data_size"] for x in ms] == [len(p) for p in pieces]
    assert sum(x["member_size"] for x in ms) == len(img)
    for x, piece in zip(ms, pieces):
        assert x["crc"] == zlib.crc32(piece)
        assert LS.liblzma_raw(x["stream"], dict_byte(level), len(piece) + 64) == (piece, True, len(x["stream"]))
    assert len(img) <= bound(len(data), level)
    return ms


# ---- the CPU stand-in -------------------------------------------------------------------------------------------

class _Batch(C.Structure):      # la_lzc_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("level", C.c_uint32), ("flags", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p)]


class StandIn:
    """la_gpu_lzip_compress of tests/mock_gpu through its ABI entry ("device" pointers are host pointers)"""

    def __init__(self):
        lib = mock_build.gpu_lib()
        lib.la_gpu_lzip_compress.argtypes = [C.c_void_p, C.POINTER(_Batch)]
        lib.la_gpu_lzip_compress_bound.restype = C.c_uint64
        lib.la_gpu_lzip_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_gpu_lzip_compress_member_bytes.restype = C.c_uint64
        lib.la_gpu_lzip_compress_member_bytes.argtypes = [C.c_uint32]
        lib.la_lzc_mock_events.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        lib.la_lzc_mock_events.restype = C.c_uint32
        self.lib = lib

    def bound(self, n, level=6):
        return int(self.lib.la_gpu_lzip_compress_bound(n, level))

    def member_bytes(self, level=6):
        return int(self.lib.la_gpu_lzip_compress_member_bytes(level))

    def call(self, data, level=6, flags=0, cap=None):
        """(return code, needed size, the out_cap bytes of room)"""
        cap = self.bound(len(data), level) if cap is None else cap
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        out = C.create_string_buffer(max(cap, 1))
        n = C.c_uint64(0)
        b = _Batch(C.addressof(src) if data else None, len(data), level, flags, C.addressof(out), cap, C.addressof(n))
        rc = self.lib.la_gpu_lzip_compress(1, C.byref(b))       # (the stand-in only asks for a context that is not NULL)
        return rc, n.value, out.raw[:cap]

    def compress(self, data, level=6):
        rc, n, out = self.call(data, level)
        assert rc == 0 and n <= len(out)
        return out[:n]

    def events(self, reset=False):
        v = (C.c_uint64 * 32)()
        n = self.lib.la_lzc_mock_events(v, 1 if reset else 0)
        assert n == len(EVENTS)
        return dict(zip(EVENTS, (int(x) for x in v[:n])))
