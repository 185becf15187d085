"""Support for the xz write tests: the named inputs of the device tests (shared with the recorded digests of
tests/golden/xz_write_digests.json), the checks every written image has to pass, and the CPU stand-in of
tests/mock_gpu/la_gpu_xz_comp_mock.c, which compiles the kernels' own rules header and therefore writes the device's bytes."""
import ctypes as C
import functools
import hashlib
import json
import lzma
import os
import random

import mock_build
import xz_parse as XP
import xz_support as XS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "xz_write_digests.json")
CHUNK, BLOCK = 1 << 16, 1 << 20
FIRST = 1
EVENTS = ["carry_long", "stored", "rep0", "rep1", "rep2", "rep3", "short_rep", "len_low", "len_mid", "len_high", "split", "dist_slot",
          "dist_special", "dist_align", "matched_literal", "across_chunks"]


def noise(seed, n):
    return random.Random(seed).randbytes(n)


def filler(seed, n):
    """sixteen letters, no structure: codes to about half its size as literals, matches of four bytes are rare"""
    return noise(seed, n).translate(bytes(b"abcdefghijklmnop"[i & 15] for i in range(256)))


@functools.lru_cache(maxsize=None)
def big_text():
    """2 MiB + 1 of text-like bytes; the shorter text inputs are its prefixes"""
    r = random.Random(77)
    words = [XS.letters(7700 + i, 2 + i % 7, 8) for i in range(60)]
    out = bytearray()
    while len(out) < 2 * BLOCK + 1:
        out += b" ".join(r.choice(words) for _ in range(4096)) + b" "
    return bytes(out[:2 * BLOCK + 1])


def marker(seed, n=40):
    """bytes no filler holds: they match each other only"""
    return bytes(0x80 | b for b in noise(seed, n))


PLANT_DISTANCES = (1, 2, 3, 5, 100, 127, 128, 129, 4096, 60000)


@functools.lru_cache(maxsize=None)
def planted():
    """one chunk of filler with a 24-byte pattern repeated at each of PLANT_DISTANCES, each pair starting at all four
    residues of the position mod 4.  Returns (bytes, [(first start, distance)])."""
    buf = bytearray(filler(31, CHUNK))
    spots, p = [], 64
    for d in sorted(PLANT_DISTANCES, reverse=True):     # the widest pairs first: both copies must lie in the chunk
        for r in range(4):
            p += (r - p) % 4
            unit = marker(1000 * d + r, min(d, 24))
            if d < 24:          # a period: the pattern overlaps its own repeat
                seg = (unit * (48 // d + 2))[:24 + d]
                buf[p:p + len(seg)] = seg
            else:
                buf[p:p + 24] = unit
                buf[p + d:p + d + 24] = unit
            spots.append((p, d))
            p += 64 if d == 60000 else d + 24 + 40
    assert p < 60000
    return bytes(buf), spots


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes: every input of tests/test_gpu_xz_compress.py whose bytes are recorded, at most 2 MiB + 1"""
    t = big_text()
    m = marker(5)
    border = bytearray(filler(41, 2 * CHUNK))
    border[CHUNK - 50:CHUNK - 10] = m
    border[CHUNK + 10:CHUNK + 50] = m
    blocks = bytearray(filler(42, BLOCK + CHUNK))
    blocks[BLOCK - 45:BLOCK - 5] = m
    blocks[BLOCK + 5:BLOCK + 45] = m
    return {
        "empty": b"", "one_byte": b"x", "chunk_minus_1": t[:CHUNK - 1], "chunk": t[:CHUNK], "chunk_plus_1": t[:CHUNK + 1],
        "block": t[:BLOCK], "block_plus_1": t[:BLOCK + 1], "two_blocks_plus_1": t,
        "noise_2c5": noise(21, 2 * CHUNK + 5),
        "text_noise_text": t[:CHUNK] + noise(22, CHUNK) + t[CHUNK:2 * CHUNK],
        "run_3c": b"\x07" * (3 * CHUNK),
        "planted": planted()[0],
        "border_marker": bytes(border),
        "block_marker": bytes(blocks),
        "text_2mib": t[:2 * BLOCK],
    }


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def digest(blob):
    return {"size": len(blob), "sha256": hashlib.sha256(blob).hexdigest()}


def stored_size(n):
    """bytes la_gpu_xz_compress writes for ONE block of n input bytes when every chunk is stored, stream header included"""
    body = n + 3 * -(-n // CHUNK) + 1
    return 12 + 16 + body + (-body % 4) + 8


def accept(img, data):
    """what every written image has to pass: liblzma returns the input; the reference's read loop does, whole and 4 096
    bytes at a time; ONE stream; every block header carries both sizes; every block is at most 1 MiB; index records equal
    the blocks; backward size and footer are right; no byte follows the footer (the last four are XP.walk's)."""
    dec = lzma.LZMADecompressor(format=lzma.FORMAT_XZ)
    assert dec.decompress(img) == data and dec.eof and dec.unused_data == b"" and dec.check == lzma.CHECK_CRC64
    for read_size in (None, 4096):
        assert XS.reference_read(img, read_size) == (data, 0, "")
    w = XP.walk(img)
    assert w["check"] == 4
    assert all(b["comp"] is not None and b["uncomp"] is not None and b["header_size"] == 16 and b["dict_byte"] == 16 for b in w["blocks"])
    assert [b["uncomp"] for b in w["blocks"]] == [min(BLOCK, len(data) - o) for o in range(0, len(data), BLOCK)]
    assert w["records"] == [(b["unpadded"], b["uncomp"]) for b in w["blocks"]]
    for b in w["blocks"]:
        sizes = [c[1] for c in b["chunks"]]
        assert sizes == [min(CHUNK, b["uncomp"] - o) for o in range(0, b["uncomp"], CHUNK)]
        for k, (control, usize, csize, _) in enumerate(b["chunks"]):
            assert control == ((0xE0 if k == 0 else 0xC0) if csize is not None else (1 if k == 0 else 2))
            assert (6 + csize if csize is not None else 3 + usize) <= usize + 5
    return w


# ---- the CPU stand-in -------------------------------------------------------------------------------------------

class _Batch(C.Structure):      # la_xzc_batch
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("level", C.c_uint32), ("flags", C.c_uint32),
                ("d_out", C.c_void_p), ("out_cap", C.c_uint64), ("d_out_bytes", C.c_void_p)]


class StandIn:
    """la_gpu_xz_compress of tests/mock_gpu through its ABI entry ("device" pointers are host pointers)"""

    def __init__(self):
        lib = mock_build.gpu_lib()
        lib.la_gpu_xz_compress.argtypes = [C.c_void_p, C.POINTER(_Batch)]
        lib.la_gpu_xz_compress_bound.restype = C.c_uint64
        lib.la_gpu_xz_compress_bound.argtypes = [C.c_uint64, C.c_uint32]
        lib.la_xzc_mock_events.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        lib.la_xzc_mock_events.restype = C.c_uint32
        self.lib = lib

    def bound(self, n, level=6):
        return int(self.lib.la_gpu_xz_compress_bound(n, level))

    def compress(self, data, level=6, flags=FIRST):
        cap = self.bound(len(data), level)
        src = C.create_string_buffer(bytes(data), max(len(data), 1))
        out = C.create_string_buffer(max(cap, 1))
        n = C.c_uint64(0)
        b = _Batch(C.addressof(src) if data else None, len(data), level, flags, C.addressof(out), cap, C.addressof(n))
        assert self.lib.la_gpu_xz_compress(1, C.byref(b)) == 0      # (the stand-in only asks for a context that is not NULL)
        assert n.value <= cap
        return out.raw[:n.value]

    def events(self, reset=False):
        v = (C.c_uint64 * 32)()
        n = self.lib.la_xzc_mock_events(v, 1 if reset else 0)
        assert n == len(EVENTS)
        return dict(zip(EVENTS, (int(x) for x in v[:n])))
