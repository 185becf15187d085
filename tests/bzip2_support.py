"""Support for the bzip2 tests: the reference's read loop restated over the image's real libbz2, and the generators.

reference_read() is bzip2_filter_read (libarchive/archive_read_support_filter_bzip2.c:214-332) in Python, statement
for statement: the bid before every stream (bzip2.c:112-148), BZ2_bzDecompressInit / BZ2_bzDecompress /
BZ2_bzDecompressEnd through ctypes, one 64 KiB output block per read, "truncated bzip2 input" when upstream has no
byte left inside a stream, "bzip decompression failed" for everything libbz2 refuses.  Upstream is a memory reader
that hands out `read_size` bytes at a time (default: everything).  It returns what la_api.as_reference_tuple returns:
(bytes, 0, "") for a clean end, (bytes in front of the error, -30, message) otherwise."""
import bz2
import ctypes as C
import random

ARCHIVE_FATAL = -30
OUT_BLOCK = 64 * 1024
BZ_OK, BZ_STREAM_END = 0, 4
BLOCK_MAGIC, END_MAGIC = 0x314159265359, 0x177245385090


class _BzStream(C.Structure):
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_uint), ("total_in_lo32", C.c_uint), ("total_in_hi32", C.c_uint),
                ("next_out", C.c_void_p), ("avail_out", C.c_uint), ("total_out_lo32", C.c_uint), ("total_out_hi32", C.c_uint),
                ("state", C.c_void_p), ("bzalloc", C.c_void_p), ("bzfree", C.c_void_p), ("opaque", C.c_void_p)]


_LIB = None


def libbz2():
    global _LIB
    if _LIB is None:
        lib = C.CDLL("libbz2.so.1.0")
        lib.BZ2_bzDecompressInit.argtypes = [C.POINTER(_BzStream), C.c_int, C.c_int]
        lib.BZ2_bzDecompress.argtypes = [C.POINTER(_BzStream)]
        lib.BZ2_bzDecompressEnd.argtypes = [C.POINTER(_BzStream)]
        lib.BZ2_bzlibVersion.restype = C.c_char_p
        _LIB = lib
    return _LIB


def bid(buf):
    """bzip2_reader_bid over the 14 bytes ahead (fewer: 0)."""
    if len(buf) < 14 or buf[:3] != b"BZh" or not (0x31 <= buf[3] <= 0x39):
        return 0
    if buf[4:10] not in (BLOCK_MAGIC.to_bytes(6, "big"), END_MAGIC.to_bytes(6, "big")):
        return 0
    return 24 + 5 + 48


def reference_read(image, read_size=None):
    lib = libbz2()
    image = bytes(image)
    if not bid(image[:14]):
        raise ValueError("the bidder would not take this image: no bzip2 filter is created")
    src = C.create_string_buffer(image, len(image))
    base = C.addressof(src)
    pos = 0                                     # what upstream has consumed
    chunk = read_size or max(len(image), 1)
    out_block = C.create_string_buffer(OUT_BLOCK)
    out = bytearray()
    strm = _BzStream()
    valid = eof = False
    try:
        while not eof:                          # one bzip2_filter_read per turn
            strm.next_out = C.addressof(out_block)
            strm.avail_out = OUT_BLOCK
            while True:
                if not valid:
                    if bid(image[pos:pos + 14]) == 0:
                        eof = True
                        break
                    if lib.BZ2_bzDecompressInit(C.byref(strm), 0, 0) != BZ_OK:
                        return bytes(out), ARCHIVE_FATAL, "Internal error initializing decompressor"
                    valid = True
                # __archive_read_filter_ahead(upstream, 1, &ret): what is buffered of the current chunk, NULL at the end
                avail = min(len(image) - pos, chunk - (pos % chunk))
                if avail <= 0:
                    return bytes(out), ARCHIVE_FATAL, "truncated bzip2 input"
                strm.next_in = base + pos
                strm.avail_in = avail
                ret = lib.BZ2_bzDecompress(C.byref(strm))
                pos += avail - strm.avail_in
                if ret == BZ_STREAM_END:
                    lib.BZ2_bzDecompressEnd(C.byref(strm))
                    valid = False
                elif ret != BZ_OK:
                    return bytes(out), ARCHIVE_FATAL, "bzip decompression failed"
                if strm.avail_out == 0:
                    break
            out += out_block.raw[:OUT_BLOCK - strm.avail_out]
        return bytes(out), 0, ""
    finally:
        if valid:
            lib.BZ2_bzDecompressEnd(C.byref(strm))


def reference_cat(image, read_size=None):
    """What the whole read stack gives: libarchive puts a filter on a filter's output as long as a bidder takes it
    (cat/test/test_expand.bz2 is a bzip2 stream of a bzip2 stream), so the loop is applied until the bid fails."""
    data, rc, msg = reference_read(image, read_size)
    while rc == 0 and bid(data[:14]):
        data, rc, msg = reference_read(data)
    return data, rc, msg


# ---- generators -------------------------------------------------------------------------------------------------

def letters(seed, n, k=10):
    r = random.Random(seed)
    return bytes(r.choice(b"abcdefghij"[:k]) for _ in range(n))


def noise(seed, n, k=256):
    r = random.Random(seed)
    return bytes(r.randrange(k) for _ in range(n))


def stream350k(level=1):
    """350 000 bytes over four values: four blocks at level 1, none of them byte-aligned but the first."""
    return bz2.compress(noise(350, 350000, 4), level)


def find_magics(image):
    """[(bit offset, kind)] of every block (0) and end-of-stream (1) magic at any bit position, ascending."""
    import numpy as np
    n = len(image)
    if n < 6:
        return []
    b = np.frombuffer(bytes(image) + bytes(8), dtype=np.uint8).astype(np.uint64)
    w = np.zeros(n, dtype=np.uint64)            # the 7 bytes from byte i on, big-endian
    for k in range(7):
        w = (w << np.uint64(8)) | b[k:k + n]
    hits = []
    for ph in range(8):
        v = (w >> np.uint64(8 - ph)) & np.uint64(0xFFFFFFFFFFFF)
        for magic, kind in ((BLOCK_MAGIC, 0), (END_MAGIC, 1)):
            for i in np.nonzero(v == np.uint64(magic))[0]:
                bit = int(i) * 8 + ph
                if bit + 48 <= n * 8:
                    hits.append((bit, kind))
    return sorted(hits)


def flip(image, bit):
    b = bytearray(image)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def abi_cases():
    """name -> plain bytes: the shapes of the device ABI test (all level 1)."""
    return {
        "empty": b"", "one_byte": b"x",
        "letters_50": letters(1, 50), "letters_300": letters(2, 300), "letters_800": letters(3, 800),
        "letters_2000": letters(4, 2000), "letters_10000": letters(5, 10000), "letters_120000": letters(6, 120000),
        "one_symbol": b"zzz", "all_256": bytes(range(256)) * 3,
        "periodic_ab": b"ab" * 50000, "periodic_abc": b"abc" * 30000, "periodic_1000": noise(7, 1000) * 100,
        "run_4": b"q" + b"a" * 4 + b"z", "run_5": b"q" + b"a" * 5 + b"z", "run_255": b"a" * 255 + b"c",
        "run_259": b"a" * 259 + b"c", "run_260": b"a" * 260 + b"c", "bbbbaaaaa": b"bbbbaaaaa",
        "run_at_block_end": letters(8, 500) + b"k" * 7, "run_4_at_block_end": letters(9, 500) + b"k" * 4,
        "count_equals_byte": b"\x04" * 8 + b"x" + b"\x01" * 5 + b"\x01y",
        "unaligned_350k": noise(350, 350000, 4),
    }


def stream3000():
    """11 000 bytes over four values: one block, a stream of about 3 000 bytes."""
    return bz2.compress(noise(31, 11000, 4), 1)


def filter_shapes():
    """name -> image: the stream shapes of the filter tests."""
    big, small = stream350k(), stream3000()
    empty = bz2.compress(b"")
    return {
        "one_stream": big,
        "small_stream": small,
        "empty_stream": empty,
        "concatenated_mixed_levels": small + empty + bz2.compress(letters(3, 5000), 9) + big + bz2.compress(b"", 3) +
        bz2.compress(letters(4, 40000), 5) + empty,
        "trailing_junk": big + b"junk" * 9,
        "trailing_junk_short": small + b"xyz",
        "trailing_junk_that_starts_like_a_stream": small + b"BZh9" + bytes(20),
        "higher_level_behind_a_lower": small + bz2.compress(noise(5, 250000, 7), 3),
    }


def randomised_bits(image):
    """Bit positions of the randomised bit of every block of a VALID single-window image: 80 bits behind a block magic
    (48 of magic, 32 of CRC).  find_magics may list a false match inside compressed data; the caller passes streams
    that have none (checked against the block count)."""
    return [b + 80 for b, k in find_magics(image) if k == 0]


FIXTURE_DIR = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "ref_fixtures", "bzip2")


def fixtures():
    """[(manifest entry, image bytes)]"""
    import json
    import os
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        man = json.load(f)
    return [(m, open(os.path.join(FIXTURE_DIR, m["file"]), "rb").read()) for m in man]
