"""Support for the lzip tests: a member builder, hand-built LZMA streams, and the reference's read loop restated over
the image's real liblzma.

member() writes header, raw LZMA1 stream (Python's lzma: FORMAT_RAW, FILTER_LZMA1, lc 3, lp 0, pb 2, end marker
included) and trailer, with a knob for every field.  StreamWriter turns an explicit packet list (xz_build's packets,
plus Marker) into one raw LZMA1 stream through xz_build's range encoder, used unchanged.

reference_read() is xz_filter_read + lzip_init + lzip_tail (libarchive/archive_read_support_filter_xz.c:533-735) in
Python, statement for statement, for the lzip case: lzma_properties_decode + lzma_raw_decoder per member, one 64 KiB
output block per read, lzma_code with LZMA_FINISH once upstream has no byte left, set_error's strings and lzip_tail's.
Upstream is a memory reader that hands out `read_size` bytes at a time (default: everything).  It returns (bytes in front
of the error or all of them, the filter's return code: 0, -25 ARCHIVE_FAILED or -30 ARCHIVE_FATAL, message)."""
import collections
import ctypes as C
import functools
import json
import lzma
import os
import struct
import zlib

import xz_build as XB
import xz_support as XS

ARCHIVE_FAILED, ARCHIVE_FATAL = -25, -30
OUT_BLOCK = 64 * 1024
LZMA_OK, LZMA_STREAM_END = 0, 1
LZMA_RUN, LZMA_FINISH = 0, 3
LZMA_FILTER_LZMA1 = 0x4000000000000001
LZMA_VLI_UNKNOWN = 2 ** 64 - 1
DATA_ERROR, BUF_ERROR = XS.DATA_ERROR, XS.BUF_ERROR
E_REMAINING, E_CRC, E_SIZE, E_MEMBER = ("Lzip: Remaining data is less bytes", "Lzip: CRC32 error", "Lzip: Uncompressed size error",
                                        "Lzip: Member size error")
ARCHIVE_FILTER_LZIP = 9

text, noise, letters, flip = XS.text, XS.noise, XS.letters, XS.flip


class _LzmaFilter(C.Structure):     # lzma/filter.h: lzma_filter
    _fields_ = [("id", C.c_uint64), ("options", C.c_void_p)]


def _liblzma():
    lib = XS.liblzma()
    lib.lzma_properties_decode.argtypes = [C.POINTER(_LzmaFilter), C.c_void_p, C.c_char_p, C.c_size_t]
    lib.lzma_raw_decoder.argtypes = [C.POINTER(XS._LzmaStream), C.POINTER(_LzmaFilter)]
    lib.lzma_crc32.restype = C.c_uint32
    lib.lzma_crc32.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32]
    return lib


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def has_member(buf):
    """lzip_has_member over the 6 bytes ahead (fewer: 0): the bits checked"""
    b = bytes(buf[:6])
    if len(b) < 6 or b[:4] != b"LZIP" or b[4] not in (0, 1) or not 12 <= (b[5] & 0x1F) <= 29:
        return 0
    return 48


def dict_size(b):
    size = 1 << (b & 0x1F)
    if (b & 0x1F) > 12:
        size -= (size // 16) * (b >> 5)
    return size


def reference_read(image, read_size=None):
    lib = _liblzma()
    image = bytes(image)
    if not has_member(image):
        raise ValueError("the bidder would not take this image: no lzip filter is created")
    src = C.create_string_buffer(image, len(image))
    base = C.addressof(src)
    chunk = read_size or max(len(image), 1)
    out_block = C.create_string_buffer(OUT_BLOCK)
    out = bytearray()
    strm = XS._LzmaStream()
    S = {"pos": 0, "in_stream": False, "eof": False, "crc32": 0, "member_in": 0, "member_out": 0, "ver": 0}

    def ahead(n):
        """__archive_read_filter_ahead(upstream, n): the offset, or None when fewer than n bytes are left (a memory
        reader's buffer is refilled until it holds n)"""
        return S["pos"] if len(image) - S["pos"] >= n else None

    def lzip_init():
        h = ahead(6)
        if h is None:
            return ARCHIVE_FATAL, ""
        S["ver"] = image[h + 4]
        log2dic = image[h + 5] & 0x1F
        if log2dic < 12 or log2dic > 29:
            return ARCHIVE_FATAL, ""
        props = bytes([0x5D]) + struct.pack("<I", dict_size(image[h + 5]))
        S["pos"] += 6
        S["member_in"] = 6
        filters = (_LzmaFilter * 2)()
        filters[0].id, filters[0].options = LZMA_FILTER_LZMA1, None
        filters[1].id, filters[1].options = LZMA_VLI_UNKNOWN, None
        ret = lib.lzma_properties_decode(C.byref(filters[0]), None, props, len(props))
        if ret != LZMA_OK:
            return ARCHIVE_FATAL, XS.MESSAGES.get(ret, "Lzma decompression failed:  Unknown error")
        ret = lib.lzma_raw_decoder(C.byref(strm), filters)
        _libc.free(filters[0].options)
        if ret != LZMA_OK:
            return ARCHIVE_FATAL, XS.MESSAGES.get(ret, "Lzma decompression failed:  Unknown error")
        return 0, ""

    def lzip_tail():
        tail = 12 if S["ver"] == 0 else 20
        f = ahead(tail)
        if f is None:
            return ARCHIVE_FAILED, E_REMAINING
        if S["crc32"] != struct.unpack_from("<I", image, f)[0]:
            return ARCHIVE_FAILED, E_CRC
        if S["member_out"] != struct.unpack_from("<Q", image, f + 4)[0]:
            return ARCHIVE_FAILED, E_SIZE
        if S["ver"] == 1 and S["member_in"] + tail != struct.unpack_from("<Q", image, f + 12)[0]:
            return ARCHIVE_FAILED, E_MEMBER
        S["pos"] += tail
        if has_member(image[S["pos"]:S["pos"] + 6]):
            S.update(in_stream=False, crc32=0, member_out=0, member_in=0, eof=False)
        return 0, ""

    try:
        while True:                             # one xz_filter_read per turn
            redo = True
            while redo:
                redo = False
                strm.next_out = C.addressof(out_block)
                strm.avail_out = OUT_BLOCK
                member_in = S["member_in"]
                while strm.avail_out > 0 and not S["eof"]:
                    if not S["in_stream"]:
                        rc, msg = lzip_init()
                        if rc != 0:
                            return bytes(out), rc, msg
                        S["in_stream"] = True
                    avail = min(len(image) - S["pos"], chunk - (S["pos"] % chunk))
                    strm.next_in = base + S["pos"] if avail > 0 else None
                    strm.avail_in = avail
                    ret = lib.lzma_code(C.byref(strm), LZMA_FINISH if avail == 0 else LZMA_RUN)
                    if ret == LZMA_STREAM_END:
                        S["eof"] = True
                    if ret in (LZMA_OK, LZMA_STREAM_END):
                        S["pos"] += avail - strm.avail_in
                        S["member_in"] += avail - strm.avail_in
                    else:
                        return bytes(out), ARCHIVE_FATAL, XS.MESSAGES.get(ret, "Lzma decompression failed:  Unknown error")
                n = OUT_BLOCK - strm.avail_out
                S["member_out"] += n
                if n == 0:
                    if member_in != S["member_in"] and S["eof"]:
                        rc, msg = lzip_tail()
                        if rc != 0:
                            return bytes(out), rc, msg
                        if not S["eof"]:
                            redo = True
                            continue
                    return bytes(out), 0, ""
                S["crc32"] = lib.lzma_crc32(C.addressof(out_block), n, S["crc32"])
                if S["eof"]:
                    rc, msg = lzip_tail()
                    if rc != 0:
                        return bytes(out), rc, msg
                out += out_block.raw[:n]
    finally:
        lib.lzma_end(C.byref(strm))


def reference_cat(image, read_size=None):
    """What the whole read stack gives: a filter is put on a filter's output as long as a bidder takes it; the filter's
    code is what the read core turns every failed read into (archive_read.c: __archive_read_filter_ahead)"""
    data, rc, msg = reference_read(image, read_size)
    while rc == 0 and has_member(data):
        data, rc, msg = reference_read(data)
    return data, (ARCHIVE_FATAL if rc else 0), msg


# ---- members ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def raw_lzma1(plain, dict_bits=20, preset=6):
    return lzma.compress(plain, format=lzma.FORMAT_RAW,
                         filters=[{"id": lzma.FILTER_LZMA1, "preset": preset, "lc": 3, "lp": 0, "pb": 2, "dict_size": 1 << dict_bits}])


def wrap(raw, plain, version=1, dict_byte=20, crc=None, data_size=None, member_size=None, magic=b"LZIP"):
    """header + a raw LZMA1 stream + trailer over `plain`; every trailer field can be written wrong"""
    out = magic + bytes([version, dict_byte]) + raw
    out += struct.pack("<IQ", zlib.crc32(plain) if crc is None else crc, len(plain) if data_size is None else data_size)
    if version != 0:
        out += struct.pack("<Q", len(out) + 8 if member_size is None else member_size)
    return out


def member(plain, preset=6, **kw):
    return wrap(raw_lzma1(bytes(plain), kw.get("dict_byte", 20) & 0x1F, preset), plain, **kw)


# ---- hand-built streams ---------------------------------------------------------------------------------------------

Marker = collections.namedtuple("Marker", "len")        # a match of this length with distance 0xFFFFFFFF


class StreamWriter(XB.Lzma2Writer):
    """one raw LZMA1 stream (lc 3, lp 0, pb 2) from a packet list; xz_build's model and range encoder, no chunk layer"""

    def __init__(self):
        super().__init__()
        self.rc = XB._RangeEncoder()

    def put(self, packets):
        for pk in packets:
            if isinstance(pk, Marker):
                n = len(self.hist)
                self._packet(self.rc, XB.Match(1 << 32, pk.len))
                del self.hist[n:]
            else:
                self._packet(self.rc, pk)
        return self

    def raw(self):
        return XB._RangeEncoder.finish(_copy_rc(self.rc))


def _copy_rc(rc):
    c = XB._RangeEncoder()
    c.low, c.range, c.cache, c.cache_size, c.out = rc.low, rc.range, rc.cache, rc.cache_size, bytearray(rc.out)
    return c


def liblzma_raw(raw, dict_byte=20, limit=1 << 24):
    """(bytes, ended) of liblzma's raw LZMA1 decoder over `raw`, all input at once then LZMA_FINISH; ended is True at the
    marker, False when the input ran out (LZMA_BUF_ERROR), and 'data' for LZMA_DATA_ERROR; consumed bytes as third"""
    lib = _liblzma()
    strm = XS._LzmaStream()
    props = bytes([0x5D]) + struct.pack("<I", dict_size(dict_byte))
    filters = (_LzmaFilter * 2)()
    filters[0].id, filters[1].id = LZMA_FILTER_LZMA1, LZMA_VLI_UNKNOWN
    assert lib.lzma_properties_decode(C.byref(filters[0]), None, props, len(props)) == LZMA_OK
    assert lib.lzma_raw_decoder(C.byref(strm), filters) == LZMA_OK
    _libc.free(filters[0].options)
    src = C.create_string_buffer(bytes(raw), max(len(raw), 1))
    dst = C.create_string_buffer(limit)
    strm.next_in, strm.avail_in = C.addressof(src), len(raw)
    strm.next_out, strm.avail_out = C.addressof(dst), limit
    try:
        ret = lib.lzma_code(C.byref(strm), LZMA_RUN)
        while ret == LZMA_OK and strm.avail_out:
            ret = lib.lzma_code(C.byref(strm), LZMA_FINISH)
        out, used = dst.raw[:limit - strm.avail_out], len(raw) - strm.avail_in
    finally:
        lib.lzma_end(C.byref(strm))
    return out, (True if ret == LZMA_STREAM_END else "data" if ret == 9 else False), used


@functools.lru_cache(maxsize=None)
def stream_cases():
    """name -> (raw stream, dictionary byte): the hand-built streams of the rules and ABI tests"""
    L, M, R, S, K = XB.literals, XB.Match, XB.Rep, XB.ShortRep, Marker
    w = lambda pk: StreamWriter().put(pk).raw()     # noqa: E731
    out = {}
    out["match_273"] = (w(L(b"abc") + [M(3, 273), M(1, 2), K(2)]), 20)
    out["all_reps"] = (w(L(b"abcdefgh") + [M(8, 4), XB.Lit(0x78), R(0, 3), M(3, 5), R(1, 4), M(11, 2), M(2, 6), R(2, 2), R(3, 3), S(), XB.Lit(0x79), S(), S(),
                                        R(3, 9), R(1, 17), XB.Lit(0x7A), R(0, 273), R(2, 10), R(3, 18), K(2)]), 20)
    out["short_rep_at_0"] = (w([S()] + L(b"zz") + [K(2)]), 20)
    out["rep_at_0"] = (w([R(0, 5)] + L(b"zz") + [K(2)]), 20)
    out["dict_4096_equal"] = (w(L(noise(8, 5000, 3)) + [M(4096, 3), K(2)]), 12)
    out["dict_4096_one_past"] = (w(L(noise(8, 5000, 3)) + [M(4097, 3), K(2)]), 12)
    out["distance_equal_to_the_data"] = (w(L(b"0123456789") + [M(10, 4)] + L(b"zz") + [K(2)]), 20)
    out["distance_past_the_data"] = (w(L(b"0123456789") + [M(11, 4)] + L(b"zz") + [K(2)]), 20)
    out["marker_len_5"] = (w(L(b"hello") + [K(5)]), 20)
    out["marker_len_273"] = (w(L(b"hello") + [K(273)]), 20)
    out["empty"] = (w([K(2)]), 20)
    good = w(L(b"some literals and ") + [M(4, 6)] + L(b" a tail") + [K(2)])
    out["good"] = (good, 20)
    out["bytes_behind_the_marker"] = (good + b"\x01\x02\x03 behind", 20)
    out["first_init_byte_1"] = (b"\x01" + good[1:], 20)
    out["first_init_byte_255"] = (b"\xFF" + good[1:], 20)
    # a marker with a non-zero code behind it: the stream's last byte decides nothing but the code
    for delta in (1, 0x80):
        out["marker_code_%d" % delta] = (good[:-1] + bytes([(good[-1] + delta) & 0xFF]), 20)
    out["no_marker"] = (w(L(b"some literals and ") + [M(4, 6)] + L(b" a tail")), 20)
    # cut inside each symbol kind: the stream ends one to five bytes short of the symbol's last byte
    for name, pk in (("literal", L(noise(3, 40))), ("match", L(b"abcdefgh") + [M(8, 4), M(3, 20), M(70000 % 8 + 1, 9)]),
                     ("far_match", L(noise(4, 300)) + [M(290, 5)]), ("rep", L(b"abcdefgh") + [M(8, 4), XB.Lit(1), R(0, 30)]),
                     ("short_rep", L(b"abcdefgh") + [M(8, 4), XB.Lit(1), S()]), ("marker", L(b"abcdefgh") + [K(2)])):
        whole = w(pk + ([] if name == "marker" else L(b"tail") + [K(2)]))
        before = len(w(pk[:-1])) - 5 if len(pk) > 1 else 0
        for cut in sorted({max(before, 0), max(before, 0) + 2, len(whole) - 6, len(whole) - 5, len(whole) - 3, len(whole) - 1}):
            if 0 <= cut < len(whole):
                out["cut_%s_%d" % (name, cut)] = (whole[:cut], 20)
    return out


# ---- stream shapes ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def three():
    """three members, about 2.5 KB: the stream of the patch, cut and flip tests; and [(start, end)] of each"""
    parts = [text(1, 5000), noise(2, 700, 16), text(3, 4000)]
    ms = [member(p) for p in parts]
    spans, pos = [], 0
    for m in ms:
        spans.append((pos, pos + len(m)))
        pos += len(m)
    return b"".join(ms), spans, parts


@functools.lru_cache(maxsize=None)
def filter_shapes():
    """name -> image: the shapes of the filter tests"""
    t = text(5, 20000)
    one = member(t)
    a, b, c = three()[2]
    shapes = {"one_member": one, "empty_input_behind_a_member": member(b"abc")}
    for n in (0, 1, 65535, 65536, 65537):
        shapes["member_of_%d" % n] = member(text(n + 9, n))
        shapes["member_of_%d_between" % n] = member(a) + member(noise(n + 7, n)) + member(c)
    shapes["three_members"] = three()[0]
    for k in range(3):
        parts = [a, b, c]
        for field, kw in (("crc", {"crc": 0x12345678}), ("data_size", {"data_size": len(parts[k]) + 1}), ("data_size_small", {"data_size": len(parts[k]) - 1}),
                          ("member_size", {"member_size": len(member(parts[k])) + 1}), ("member_size_small", {"member_size": len(member(parts[k])) - 1})):
            shapes["patched_%s_member_%d" % (field, k)] = b"".join(member(p, **(kw if i == k else {})) for i, p in enumerate(parts))
    shapes["member_1_size_reaches_back"] = member(a) + member(b, member_size=len(member(a)) + len(member(b))) + member(c)
    shapes["huge_data_size"] = member(a) + member(b, data_size=1 << 60) + member(c)
    shapes["version_0_alone"] = member(a, version=0)
    shapes["version_0_between"] = member(a) + member(b, version=0) + member(c)
    shapes["version_0_first_and_last"] = member(a, version=0) + member(b) + member(c, version=0)
    shapes["junk_behind"] = one + b"junk behind the last member, more than twenty bytes of it"
    shapes["junk_short"] = one + b"xyz"
    shapes["junk_zeros"] = three()[0] + bytes(51)
    shapes["junk_begins_with_a_header"] = one + b"LZIP\x01\x14" + b"not a stream at all, just some text that follows a header shape"
    shapes["junk_is_a_bare_header"] = one + b"LZIP\x01\x14"
    shapes["junk_is_most_of_a_header"] = one + b"LZIP\x01"
    shapes["junk_contains_a_header_shape"] = one + b"xx" + b"LZIP\x01\x14" + member(b"hidden")
    shapes["junk_bad_version"] = one + b"LZIP\x02\x14" + member(b"hidden")[6:]
    shapes["junk_bad_dictionary"] = one + b"LZIP\x01\x0b" + member(b"hidden")[6:]
    shapes["header_shape_inside_the_data"] = member(b"LZIP\x01\x14" * 3 + noise(3, 64)) + member(noise(4, 100) + b"LZIP\x01\x0c" + noise(5, 30))
    shapes["dictionary_bytes"] = b"".join(member(text(40 + i, 3000), dict_byte=db) for i, db in enumerate((12, 0x2D, 0xF4, 29, 0xDD)))
    shapes["noise_64k_members"] = member(noise(9, 65536)) + member(noise(10, 65536)) + member(noise(11, 5))
    shapes["across_the_64k_boundary"] = member(text(6, 65536)) + member(text(7, 65530)) + member(text(8, 70000), version=0)
    shapes["bad_crc_behind_64k"] = member(text(6, 65536)) + member(a, crc=1)
    shapes["bad_crc_at_64k"] = member(text(6, 65536), crc=1) + member(a)
    shapes["bad_crc_at_64k_and_one"] = member(text(6, 65537), crc=1) + member(a)
    shapes["bad_crc_at_128k"] = member(a) + member(text(6, 131072), crc=1)
    for name, (raw, db) in stream_cases().items():
        plain = liblzma_raw(raw, db)[0]
        shapes["handbuilt_" + name] = member(a) + wrap(raw, plain, dict_byte=db) + member(c)
    return shapes


def flip_cases():
    """bit positions in the middle member of three(): every bit of its header and trailer, every 7th of its stream"""
    _, spans, _ = three()
    s, e = spans[1]
    return list(range(s * 8, (s + 6) * 8)) + list(range((s + 6) * 8, (e - 20) * 8, 7)) + list(range((e - 20) * 8, e * 8))


FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures", "lzip")


def fixtures():
    """[(manifest entry, image bytes)]"""
    with open(os.path.join(FIXTURE_DIR, "manifest.json")) as f:
        man = json.load(f)
    return [(m, open(os.path.join(FIXTURE_DIR, m["file"]), "rb").read()) for m in man]


# ---- the device ABI through ctypes (the mock library takes host pointers, the device library device pointers) ----------

UNKNOWN = 2 ** 64 - 1
HAS_CRC = 1
ST = {"OK": 0, "DATA": 32, "SRC_END": 33, "TRUNCATED": 34, "EARLY_END": 35, "SIZE_OVER": 36, "OUT_FULL": 37, "BAD_SIZE": 38, "BAD_CRC": 39,
      "REFUSED": 40}


class Member(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("src_end", C.c_uint64), ("data_size", C.c_uint64), ("dst_off", C.c_uint64), ("dst_cap", C.c_uint64),
                ("dict_size", C.c_uint32), ("crc32", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("status", C.c_uint32), ("crc32", C.c_uint32), ("out_len", C.c_uint64), ("consumed", C.c_uint64), ("valid", C.c_uint64)]


class Batch(C.Structure):
    _fields_ = [("d_src", C.c_void_p), ("src_bytes", C.c_uint64), ("d_members", C.c_void_p), ("n", C.c_uint32), ("reserved", C.c_uint32),
                ("d_dst", C.c_void_p), ("dst_cap", C.c_uint64), ("d_results", C.c_void_p)]


def expected_stream_result(raw, dict_byte, cap):
    """(status name, bytes, consumed or None) of one stream with both ends unknown, from liblzma's raw decoder"""
    out, ended, used = liblzma_raw(raw, dict_byte)
    if len(out) > cap:
        return "OUT_FULL", out[:cap], None
    if ended is True:
        return "OK", out, used
    return ("DATA" if ended == "data" else "TRUNCATED"), out, None


def mock_decode(lib, src, members, dst_cap):
    """la_gpu_lzip_decode of a library that takes host pointers: [(Result, bytes of the member's slot)]"""
    src = bytes(src)
    sbuf = C.create_string_buffer(src, max(len(src), 1))
    tab = (Member * max(len(members), 1))(*members)
    res = (Result * max(len(members), 1))()
    dst = C.create_string_buffer(max(dst_cap, 1))
    bt = Batch(C.addressof(sbuf), len(src), C.addressof(tab), len(members), 0, C.addressof(dst), dst_cap, C.addressof(res))
    lib.la_gpu_lzip_decode.argtypes = [C.c_void_p, C.POINTER(Batch)]
    assert lib.la_gpu_lzip_decode(None, C.byref(bt)) == 0
    return [(res[i], dst.raw[m.dst_off:m.dst_off + res[i].out_len]) for i, m in enumerate(members)]
