"""Support for the xz tests: the reference's read loop restated over the image's real liblzma, and the stream shapes.

reference_read() is xz_filter_read (libarchive/archive_read_support_filter_xz.c:651-735) in Python, statement for
statement, for the xz case: lzma_stream_decoder(memlimit UINT64_MAX, LZMA_CONCATENATED) (xz.c:512-515), one 64 KiB
output block per read, lzma_code with LZMA_FINISH once upstream has no byte left, set_error's strings (xz.c:420-458).
Upstream is a memory reader that hands out `read_size` bytes at a time (default: everything).  It returns what
la_api.as_reference_tuple returns: (bytes, 0, "") for a clean end, (bytes in front of the error, -30, message) otherwise.
liblzma is on the image, lzma.h is not: the lzma_stream layout is declared here."""
import ctypes as C
import functools
import json
import lzma
import os
import random

import xz_build as XB

ARCHIVE_FATAL = -30
OUT_BLOCK = 64 * 1024
LZMA_OK, LZMA_STREAM_END = 0, 1
LZMA_RUN, LZMA_FINISH = 0, 3
LZMA_CONCATENATED = 0x08
MAGIC = b"\xFD7zXZ\x00"
MESSAGES = {5: "Lzma library error: Cannot allocate memory", 6: "Lzma library error: Out of memory",
            7: "Lzma library error: format not recognized", 8: "Lzma library error: Invalid options",
            9: "Lzma library error: Corrupted input data", 10: "Lzma library error:  No progress is possible"}
DATA_ERROR, BUF_ERROR, OPTIONS_ERROR = MESSAGES[9], MESSAGES[10], MESSAGES[8]


class _LzmaStream(C.Structure):     # lzma/base.h: lzma_stream
    _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_size_t), ("total_in", C.c_uint64),
                ("next_out", C.c_void_p), ("avail_out", C.c_size_t), ("total_out", C.c_uint64),
                ("allocator", C.c_void_p), ("internal", C.c_void_p),
                ("reserved_ptr1", C.c_void_p), ("reserved_ptr2", C.c_void_p), ("reserved_ptr3", C.c_void_p), ("reserved_ptr4", C.c_void_p),
                ("reserved_int1", C.c_uint64), ("reserved_int2", C.c_uint64), ("reserved_int3", C.c_size_t), ("reserved_int4", C.c_size_t),
                ("reserved_enum1", C.c_int), ("reserved_enum2", C.c_int)]


_LIB = None


def liblzma():
    global _LIB
    if _LIB is None:
        lib = C.CDLL("liblzma.so.5")
        lib.lzma_stream_decoder.argtypes = [C.POINTER(_LzmaStream), C.c_uint64, C.c_uint32]
        lib.lzma_code.argtypes = [C.POINTER(_LzmaStream), C.c_int]
        lib.lzma_end.argtypes = [C.POINTER(_LzmaStream)]
        lib.lzma_end.restype = None
        lib.lzma_version_string.restype = C.c_char_p
        _LIB = lib
    return _LIB


def bid(buf):
    """xz_bidder_bid over the 6 bytes ahead (fewer: 0)."""
    return 48 if bytes(buf[:6]) == MAGIC else 0


def reference_read(image, read_size=None):
    lib = liblzma()
    image = bytes(image)
    if not bid(image):
        raise ValueError("the bidder would not take this image: no xz filter is created")
    src = C.create_string_buffer(image, len(image))
    base = C.addressof(src)
    pos = 0                                     # what upstream has consumed
    chunk = read_size or max(len(image), 1)
    out_block = C.create_string_buffer(OUT_BLOCK)
    out = bytearray()
    strm = _LzmaStream()
    ret = lib.lzma_stream_decoder(C.byref(strm), 2 ** 64 - 1, LZMA_CONCATENATED)
    if ret != LZMA_OK:
        return b"", ARCHIVE_FATAL, MESSAGES.get(ret, "Lzma decompression failed:  Unknown error")
    eof = False
    try:
        while True:                             # one xz_filter_read per turn
            strm.next_out = C.addressof(out_block)
            strm.avail_out = OUT_BLOCK
            while strm.avail_out > 0 and not eof:
                # __archive_read_filter_ahead(upstream, 1, &avail_in): what is buffered of the current chunk, NULL at the end
                avail = min(len(image) - pos, chunk - (pos % chunk))
                strm.next_in = base + pos if avail > 0 else None
                strm.avail_in = avail
                ret = lib.lzma_code(C.byref(strm), LZMA_FINISH if avail == 0 else LZMA_RUN)
                if ret == LZMA_STREAM_END:
                    eof = True
                if ret in (LZMA_OK, LZMA_STREAM_END):
                    pos += avail - strm.avail_in
                else:
                    return bytes(out), ARCHIVE_FATAL, MESSAGES.get(ret, "Lzma decompression failed:  Unknown error")
            n = OUT_BLOCK - strm.avail_out
            if n == 0:
                return bytes(out), 0, ""
            out += out_block.raw[:n]
    finally:
        lib.lzma_end(C.byref(strm))


def reference_cat(image, read_size=None):
    """What the whole read stack gives: a filter is put on a filter's output as long as a bidder takes it."""
    data, rc, msg = reference_read(image, read_size)
    while rc == 0 and bid(data):
        data, rc, msg = reference_read(data)
    return data, rc, msg


# ---- generators -------------------------------------------------------------------------------------------------

def letters(seed, n, k=10):
    r = random.Random(seed)
    return bytes(r.choice(b"abcdefghij"[:k]) for _ in range(n))


def noise(seed, n, k=256):
    r = random.Random(seed)
    return bytes(r.randrange(k) for _ in range(n))


def text(seed, n):
    """text-like: words of a small vocabulary"""
    r = random.Random(seed)
    words = [letters(seed * 100 + i, 2 + i % 7, 8) for i in range(60)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + b" "
    return bytes(out[:n])


def flip(image, bit):
    b = bytearray(image)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def stream3000():
    """three blocks with both sizes in their headers, CRC64, about 3 KB: the stream of the cut and flip tests"""
    parts = [text(1, 5000), noise(2, 700, 16), text(3, 4000)]
    return XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC64) for p in parts], XB.CHECK_CRC64)


def stream3000_layout():
    """[(first byte, end, kind)] of stream3000(): 'header', 'block_header', 'data', 'check', 'index', 'footer'"""
    parts = [text(1, 5000), noise(2, 700, 16), text(3, 4000)]
    pos, spans = 12, [(0, 12, "header")]
    for p in parts:
        b = XB.block(XB.lzma2(p), p, XB.CHECK_CRC64)
        hs = (b.image[0] + 1) * 4
        spans += [(pos, pos + hs, "block_header"), (pos + hs, pos + len(b.image) - 8, "data"), (pos + len(b.image) - 8, pos + len(b.image), "check")]
        pos += len(b.image)
    n = len(stream3000())
    spans += [(pos, n - 12, "index"), (n - 12, n, "footer")]
    return spans


def flip_cases():
    """bit positions: every bit of the headers, checks, index and footer, every 7th bit of block data"""
    bits = []
    for a, b, kind in stream3000_layout():
        bits += list(range(a * 8, b * 8, 7 if kind == "data" else 1))
    return [b for b in bits if b >= 48]      # (the first 48 bits are the bidder's)


def filter_shapes():
    """name -> image: the container shapes of the filter tests"""
    t = text(5, 20000)
    sized = lambda p, c=XB.CHECK_CRC64: XB.block(XB.lzma2(p), p, c)             # noqa: E731
    bare = lambda p, c=XB.CHECK_CRC64: XB.block(XB.lzma2(p), p, c, comp=False, uncomp=False)   # noqa: E731
    one = XB.stream([sized(t)], XB.CHECK_CRC64)
    shapes = {
        "one_block_sized": one,
        "one_block_bare": XB.stream([bare(t)], XB.CHECK_CRC64),
        "python_lzma": lzma.compress(t),
        "two_blocks_sized": XB.stream([sized(t[:9000]), sized(t[9000:])], XB.CHECK_CRC64),
        "two_blocks_bare": XB.stream([bare(t[:9000]), bare(t[9000:])], XB.CHECK_CRC64),
        "mixed_sized_and_bare": XB.stream([sized(t[:100]), bare(t[100:300]), sized(t[300:301]), bare(t[301:302]), sized(t[302:])], XB.CHECK_CRC64),
        "only_comp_size": XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, uncomp=False)], XB.CHECK_CRC32),
        "only_uncomp_size": XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, comp=False)], XB.CHECK_CRC32),
        "seventy_blocks_sized": XB.stream([sized(t[i * 97:(i + 1) * 97 + (i % 3)]) for i in range(70)], XB.CHECK_CRC64),
        "seventy_blocks_bare": XB.stream([bare(t[i * 97:(i + 1) * 97 + (i % 3)], XB.CHECK_CRC32) for i in range(70)], XB.CHECK_CRC32),
        "one_byte_blocks": XB.stream([sized(b"a"), bare(b"b"), sized(b"c")], XB.CHECK_CRC64),
        "empty_stream": XB.stream([], XB.CHECK_CRC64),
        "empty_stream_python": lzma.compress(b""),
        "three_streams_padded": one + XB.stream([], 0) + bytes(4) + lzma.compress(t[:500]) + bytes(8) + one,
        "padding_of_three": one + bytes(3) + one,
        "padding_of_three_at_the_end": one + bytes(3),
        "padding_of_eight_at_the_end": one + bytes(8),
        "trailing_garbage": one + b"garbage behind the stream",
        "trailing_garbage_short": one + b"xyz",
        "trailing_garbage_behind_padding": one + bytes(4) + b"0123456789abcdef",
        "second_stream_bad_magic": one + MAGIC[:5] + b"\x01" + one[6:],
        "noise_64k_blocks": XB.stream([sized(noise(9, 65536)), sized(noise(10, 65536)), sized(noise(11, 5))], XB.CHECK_CRC64),
        "across_the_64k_boundary": XB.stream([sized(text(6, 65536)), sized(text(7, 65530)), bare(text(8, 70000))], XB.CHECK_CRC64),
    }
    for name, cid in (("none", 0), ("crc32", 1), ("crc64", 4), ("sha256", 10), ("unknown_id_2", 2), ("unknown_id_15", 15)):
        shapes["check_" + name] = XB.stream([sized(t[:3000], cid), bare(t[3000:7000], cid)], cid)
    for lc, lp, pb in ((0, 0, 0), (3, 0, 2), (4, 0, 0), (0, 4, 0), (0, 0, 4), (1, 3, 2)):      # 1 .. 3000 bytes under every corner of lc / lp / pb
        parts = [text(n, n) if n % 2 else noise(n, n, 6) for n in (1, 2, 65, 1000, 3000)]
        shapes["props_lc%d_lp%d_pb%d" % (lc, lp, pb)] = XB.stream(
            [XB.block(XB.lzma2(p, lc, lp, pb), p, XB.CHECK_CRC32, comp=i % 2 == 0, uncomp=i % 2 == 0) for i, p in enumerate(parts)], XB.CHECK_CRC32)
    # sizes and records that disagree
    good = sized(t[:3000])
    shapes["header_comp_size_too_small"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:3000], XB.CHECK_CRC64, comp_value=len(XB.lzma2(t[:3000])) - 4)], XB.CHECK_CRC64)
    shapes["header_comp_size_too_large"] = XB.stream([XB.block(XB.lzma2(t[:3000]) + bytes(4), t[:3000], XB.CHECK_CRC64, comp_value=len(XB.lzma2(t[:3000])) + 4)], XB.CHECK_CRC64)
    shapes["header_uncomp_size_too_small"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:3000], XB.CHECK_CRC64, uncomp_value=2999)], XB.CHECK_CRC64)
    shapes["header_uncomp_size_too_large"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:3000], XB.CHECK_CRC64, uncomp_value=3001)], XB.CHECK_CRC64)
    shapes["header_uncomp_only_too_small"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:3000], XB.CHECK_CRC64, comp=False, uncomp_value=2000)], XB.CHECK_CRC64)
    shapes["index_one_record_short"] = XB.stream([good, good], XB.CHECK_CRC64, records=[(good.unpadded, 3000)])
    shapes["index_one_record_more"] = XB.stream([good], XB.CHECK_CRC64, records=[(good.unpadded, 3000)] * 2)
    shapes["index_uncomp_differs"] = XB.stream([good, good], XB.CHECK_CRC64, records=[(good.unpadded, 3000), (good.unpadded, 3001)])
    shapes["index_unpadded_differs"] = XB.stream([good, good], XB.CHECK_CRC64, records=[(good.unpadded + 1, 3000), (good.unpadded, 3000)])
    shapes["index_records_swapped_sums_equal"] = XB.stream([sized(t[:3000]), sized(t[:3001])], XB.CHECK_CRC64,
                                                         records=[(sized(t[:3001]).unpadded, 3001), (sized(t[:3000]).unpadded, 3000)])
    shapes["index_padding_not_zero"] = XB.stream([good], XB.CHECK_CRC64, index_pad=b"\x01")
    shapes["footer_backward_size"] = XB.stream([good], XB.CHECK_CRC64, backward_delta=1)
    shapes["footer_check_differs"] = XB.stream([good], XB.CHECK_CRC64, footer_check=XB.CHECK_CRC32)
    shapes["block_padding_not_zero"] = XB.stream([XB.block(XB.lzma2(t[:3001]), t[:3001], XB.CHECK_CRC64, pad_byte=1)], XB.CHECK_CRC64)
    shapes["wrong_check_value"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:2999] + b"!", XB.CHECK_CRC64, uncomp_value=3000)], XB.CHECK_CRC64)
    shapes["wrong_sha256"] = XB.stream([XB.block(XB.lzma2(t[:3000]), t[:2999] + b"!", XB.CHECK_SHA256, uncomp_value=3000)], XB.CHECK_SHA256)
    shapes["header_reserved_flag"] = XB.stream([XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, flags_or=0x04)], XB.CHECK_CRC64)
    shapes["header_padding_not_zero"] = XB.stream([XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, header_pad=b"\x00\x00\x00\x01")], XB.CHECK_CRC64)
    shapes["header_dict_byte_41"] = XB.stream([XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, dict_byte=41)], XB.CHECK_CRC64)
    shapes["header_unknown_filter"] = XB.stream([XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, filter_id=0x30)], XB.CHECK_CRC64)
    shapes["header_comp_size_zero"] = XB.stream([XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, comp_value=0)], XB.CHECK_CRC64)
    shapes["stream_flags_reserved"] = XB.stream([good], XB.CHECK_CRC64, header_flags=b"\x00\x14")
    shapes["error_behind_64k_boundary"] = XB.stream([sized(text(6, 65536)), XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, flags_or=0x04)], XB.CHECK_CRC64)
    shapes["error_behind_64k_and_one"] = XB.stream([sized(text(6, 65537)), XB.block(XB.lzma2(t[:300]), t[:300], XB.CHECK_CRC64, flags_or=0x04)], XB.CHECK_CRC64)
    shapes["bad_check_behind_64k"] = XB.stream([sized(text(6, 65536)), XB.block(XB.lzma2(t[:3000]), t[:2999] + b"!", XB.CHECK_CRC64, uncomp_value=3000)], XB.CHECK_CRC64)
    return shapes


@functools.lru_cache(maxsize=None)
def padded_streams():
    """name -> image, about 8.4 MB each: eight streams of one 20 000-byte block, 1 MiB of stream padding behind each.
    Read with LA_GPU_BATCH_MIB=1 every window decodes one stream, so the filter's held-back tail grows over three
    windows (20 000, 40 000, 60 000 bytes) before the fourth crosses 64 KiB.  PADDED_STREAMS_BYTES: what the reference
    delivers of each."""
    pad = bytes(1 << 20)
    parts = [text(100 + i, 20000) for i in range(8)]
    streams = [XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC32)], XB.CHECK_CRC32) for p in parts]
    start = lambda i: sum(len(s) + len(pad) for s in streams[:i])      # noqa: E731
    clean = b"".join(s + pad for s in streams)
    return {
        "clean": clean,
        "cut_in_the_seventh_stream": clean[:start(6) + 100],
        "cut_in_the_fifth_padding": clean[:start(5) - 1000],
        "padding_of_three_more_behind_five": clean[:start(5)] + bytes(3) + streams[5],
        "sixth_stream_header_flip": flip(clean, (start(5) + 7) * 8 + 7),
        "sixth_stream_data_flip": flip(clean, (start(5) + 200) * 8 + 4),
        "fourth_stream_data_flip": flip(clean, (start(3) + 200) * 8 + 4),      # 60 000 held-back bytes of three windows are dropped
    }


PADDED_STREAMS_RESULT = {       # name -> (bytes delivered, message)
    "clean": (160000, ""), "cut_in_the_seventh_stream": (65536, BUF_ERROR), "cut_in_the_fifth_padding": (100000, ""),
    "padding_of_three_more_behind_five": (65536, DATA_ERROR), "sixth_stream_header_flip": (65536, DATA_ERROR),
    "sixth_stream_data_flip": (65536, DATA_ERROR), "fourth_stream_data_flip": (0, DATA_ERROR)}


FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "xz")


def fixtures():
    """[(manifest entry, image bytes)]"""
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        man = json.load(f)
    return [(m, open(os.path.join(FIXTURE_DIR, m["file"]), "rb").read()) for m in man]


# ---- hand-built LZMA2 data (xz_build.Lzma2Writer) ---------------------------------------------------------------

def wrap(raw, plain=b"", cid=XB.CHECK_NONE, dict_byte=18):
    """raw LZMA2 data as a stream of one block without sizes (what the emulator and the filter are given)"""
    return XB.stream([XB.block(raw, plain, cid, comp=False, uncomp=False, dict_byte=dict_byte)], cid)


PACKET_LOG = {}     # name -> [(packet, bytes written before it)] of the three cases named after what they hit


@functools.lru_cache(maxsize=None)
def packet_cases():
    """name -> (raw LZMA2 data, the bytes it stands for): every rep kind and short rep; lengths 2, 9, 10, 17, 18, 273;
    distances 1, 4, 127, 128, slot 14 and above with align bits, and one equal to the bytes produced so far"""
    L, M, R, S = XB.literals, XB.Match, XB.Rep, XB.ShortRep
    out = {}
    w = XB.Lzma2Writer()
    w.lzma_chunk(0xE0, L(b"abcdefgh") + [M(8, 4), XB.Lit(0x78), R(0, 3), M(3, 5), R(1, 4), M(11, 2), M(2, 6), R(2, 2), R(3, 3), S(), XB.Lit(0x79), S(), S(),
                                        R(3, 9), R(1, 17), XB.Lit(0x7A), R(0, 273), R(2, 10), R(3, 18)])
    out["reps"] = (w.image(), w.plain())
    PACKET_LOG["reps"] = w.log
    w = XB.Lzma2Writer()
    w.lzma_chunk(0xE0, L(noise(4, 300, 7)) + [M(300, 2), M(7, 9), XB.Lit(1), M(250, 10), M(1, 17), XB.Lit(2), M(299, 18), M(5, 273), M(273, 273), XB.Lit(3)])
    out["lengths"] = (w.image(), w.plain())
    PACKET_LOG["lengths"] = w.log
    w = XB.Lzma2Writer()
    pk = L(noise(5, 200, 5)) + [M(1, 3), M(4, 5), M(127, 2), M(128, 6), M(134, 4), M(192, 3), M(200, 40)]
    w.lzma_chunk(0xE0, pk)
    n = len(w.plain())
    w.lzma_chunk(0x80, [M(n, 30), XB.Lit(9), M(n + 31, 2)])        # the distance equal to the bytes produced so far, twice
    w.raw_chunk(2, noise(6, 65536))
    w.raw_chunk(2, noise(7, 5000))
    w.lzma_chunk(0x80, [M(70001, 20), M(65552, 3), M(len(w.plain()) + 23, 273), XB.Lit(4), M((1 << 16) + 0x0F + 1, 5)])   # slots 32 and 33: direct bits, align 0 and 15
    out["distances"] = (w.image(), w.plain())
    PACKET_LOG["distances"] = w.log
    for lc, lp, pb in ((0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4), (1, 3, 2)):
        w = XB.Lzma2Writer()
        w.lzma_chunk(0xE0, L(text(7, 70)) + [M(9, 12), XB.Lit(0x41), S(), R(0, 5), M(3, 8)] + L(text(8, 40)) + [R(1, 2), M(60, 20)], props=(lc, lp, pb))
        out["props_%d_%d_%d" % (lc, lp, pb)] = (w.image(), w.plain())
    return out


@functools.lru_cache(maxsize=None)
def beyond_cases():
    """name -> (raw, the bytes in front of the refusal or all of them, accepted, dictionary byte of the block header): a
    distance one beyond the data as a match, a rep and a short rep; one beyond a dictionary reset; one beyond the
    dictionary size; and next to each refusal the distance just inside, which is accepted"""
    L, M = XB.literals, XB.Match
    out = {}
    w = XB.Lzma2Writer().lzma_chunk(0xE0, L(b"0123456789") + [M(11, 4)] + L(b"zz"))
    out["match_one_beyond"] = (w.image(), b"0123456789", False, 18)
    w = XB.Lzma2Writer().lzma_chunk(0xE0, L(b"0123456789") + [M(10, 4)] + L(b"zz"))
    out["match_just_inside"] = (w.image(), w.plain(), True, 18)
    w = XB.Lzma2Writer().lzma_chunk(0xE0, [XB.ShortRep()] + L(b"zz"))
    out["short_rep_first"] = (w.image(), b"", False, 18)
    w = XB.Lzma2Writer().lzma_chunk(0xE0, [XB.Rep(0, 5)] + L(b"zz"))
    out["rep_first"] = (w.image(), b"", False, 18)
    w = XB.Lzma2Writer().raw_chunk(1, b"abcdefgh").lzma_chunk(0xE0, L(b"xy") + [M(3, 2)])   # the reset cuts the raw chunk off
    out["match_over_a_dictionary_reset"] = (w.image(), b"abcdefghxy", False, 18)
    w = XB.Lzma2Writer().raw_chunk(1, b"abcdefgh").lzma_chunk(0xC0, L(b"xy") + [M(3, 2)])
    out["match_over_a_raw_chunk"] = (w.image(), w.plain(), True, 18)
    w = XB.Lzma2Writer().lzma_chunk(0xE0, L(noise(8, 5000, 3)) + [M(4097, 3)])
    out["one_beyond_a_4096_dictionary"] = (w.image(), w.plain()[:5000], False, 0)
    w = XB.Lzma2Writer().lzma_chunk(0xE0, L(noise(8, 5000, 3)) + [M(4096, 3)])
    out["just_inside_a_4096_dictionary"] = (w.image(), w.plain(), True, 0)
    return out


@functools.lru_cache(maxsize=None)
def chunk_plans():
    """name -> (raw, plain): every chunk kind, an uncompressed chunk between two LZMA chunks, a chunk of 2 MiB, a chunk
    of 65 536 compressed bytes"""
    L, M, R, S = XB.literals, XB.Match, XB.Rep, XB.ShortRep
    out = {}
    w = XB.Lzma2Writer()
    w.raw_chunk(1, b"first, uncompressed with a reset ")
    w.lzma_chunk(0xC0, L(b"new props ") + [M(10, 6), S()], props=(2, 1, 1))
    w.lzma_chunk(0x80, [M(4, 9), XB.Lit(0x2E), R(0, 3)])
    w.lzma_chunk(0xA0, L(b"state reset ") + [M(12, 12)])
    w.raw_chunk(2, b"raw without a reset ")
    w.lzma_chunk(0x80, [M(20, 20), R(0, 2), XB.Lit(0x21)])
    w.lzma_chunk(0xE0, L(b"everything reset ") + [M(17, 5)], props=(0, 2, 0))
    w.raw_chunk(1, b"raw with a reset")
    w.lzma_chunk(0xC0, L(b"and on") + [M(6, 3)])
    out["every_kind"] = (w.image(), w.plain())
    w = XB.Lzma2Writer()
    w.lzma_chunk(0xE0, L(text(9, 100)) + [M(50, 30)])
    w.raw_chunk(2, noise(10, 777))
    w.lzma_chunk(0x80, [M(777 + 130, 100), M(700, 50), XB.Lit(0x0A), S(), R(1, 7)])
    out["raw_between_lzma"] = (w.image(), w.plain())
    w = XB.Lzma2Writer()
    n = (1 << 21) - 8
    w.lzma_chunk(0xE0, L(b"2 MiB.. ") + [M(8, 273)] * (n // 273) + [M(8, n % 273)])
    w.lzma_chunk(0x80, [M(1 << 20, 100), XB.Lit(0x21)])
    assert len(w.plain()) == (1 << 21) + 101
    out["chunk_2mib"] = (w.image(), w.plain())
    w = XB.Lzma2Writer()
    w.lzma_chunk_until(0xE0, (XB.Lit(b) for b in noise(11, 70000)), 65536)
    w.lzma_chunk(0x80, [M(60000, 8)])
    assert len(w.chunks[0]) == 6 + 65536
    out["chunk_65536_compressed"] = (w.image(), w.plain())
    return out


def _patch(raw, off, value):
    b = bytearray(raw)
    b[off] = value
    return bytes(b)


@functools.lru_cache(maxsize=None)
def refusals():
    """name -> (raw LZMA2 data that liblzma refuses with LZMA_DATA_ERROR, the bytes it was built from: what a decoder
    has written when it refuses is a prefix of them): the list of the LZMA2 layer"""
    L, M = XB.literals, XB.Match
    w = XB.Lzma2Writer().lzma_chunk(0xE0, L(b"some literals and ") + [M(4, 6)] + L(b" a tail"))
    good, plain = w.image(), w.plain()      # control, 2 + 2 size bytes, props, data, 0x00
    out = {"control_03": (b"\x03\x00\x00x\x00", b""), "control_7f": (b"\x7f\x00\x00x\x00", b"")}
    out["control_03_behind_a_chunk"] = (XB.Lzma2Writer().raw_chunk(1, b"abc").image()[:-1] + b"\x03\x00\x00x\x00", b"abc")
    out["first_chunk_raw_without_reset"] = (XB.Lzma2Writer().raw_chunk(2, b"abc").image(), b"")
    out["first_chunk_lzma_c0"] = (_patch(good, 0, 0xC0), b"")
    out["first_chunk_lzma_a0"] = (_patch(good, 0, 0xA0), b"")
    out["first_chunk_lzma_80"] = (_patch(good, 0, 0x80), b"")
    for control in (0x80, 0xA0):
        w2 = XB.Lzma2Writer().raw_chunk(1, b"abc").lzma_chunk(control, L(b"no properties yet"))
        out["lzma_%02x_behind_raw_reset" % control] = (w2.image(), b"abc")
    out["props_225"] = (_patch(good, 5, 225), b"")
    out["props_lc3_lp2"] = (_patch(good, 5, (2 * 5 + 2) * 9 + 3), b"")
    out["first_range_coder_byte_not_zero"] = (_patch(good, 6, 1), b"")
    out["compressed_size_one_more"] = (_patch(good, 4, good[4] + 1)[:-1] + b"\x00\x00", plain)
    out["compressed_size_one_less"] = (_patch(good, 4, good[4] - 1), plain)
    out["uncompressed_size_one_less"] = (_patch(good, 2, good[2] - 1), plain)
    out["uncompressed_size_one_more"] = (_patch(good, 2, good[2] + 1), plain + b"?")
    w3 = XB.Lzma2Writer().lzma_chunk(0xE0, L(b"abcdefgh") + [M(8, 20)])
    out["match_over_the_chunk_end"] = (_patch(w3.image(), 2, 20), w3.plain())
    return out
