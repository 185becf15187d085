"""Support for the tests of xz filter chains (delta and BCJ filters in front of LZMA2): test buffers in which the
filters find work, and streams whose blocks carry such chains.  liblzma (Python's lzma, FORMAT_RAW) writes the filtered
LZMA2 data; xz_build wraps it in block headers that name the chain."""
import functools
import lzma
import random
import struct
import sys

import xz_build as XB
import xz_support as XS

DELTA, X86, POWERPC, IA64, ARM, ARMTHUMB, SPARC = 3, 4, 5, 6, 7, 8, 9
LZMA2 = {"id": lzma.FILTER_LZMA2, "preset": 0}
TILE, SUB = 16384, 256          # the kernels' tile and the bytes one x86 lane looks after


def spec(fid, prop):
    return {"id": fid, "dist": prop} if fid == DELTA else {"id": fid, "start_offset": prop}


def props(fid, prop):
    """the filter's property bytes in a block header"""
    if fid == DELTA:
        return bytes([prop - 1])
    return struct.pack("<I", prop) if prop else b""


def liblzma_unfilter(chain, data):
    """liblzma's decoders of `chain` [(id, prop)] run over `data`, whatever it holds"""
    raw = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[LZMA2])
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[spec(*f) for f in chain] + [LZMA2])


def liblzma_filter(chain, data):
    raw = lzma.compress(data, format=lzma.FORMAT_RAW, filters=[spec(*f) for f in chain] + [LZMA2])
    return lzma.decompress(raw, format=lzma.FORMAT_RAW, filters=[LZMA2])


@functools.lru_cache(maxsize=None)
def real_code(n=200 * 1024):
    with open(sys.executable, "rb") as f:
        return f.read(n)


@functools.lru_cache(maxsize=None)
def x86_buffers():
    r = random.Random(86)
    out = {"all_e8": b"\xE8" * 3000, "all_e9": b"\xE9" * 777}
    for top in (0x00, 0xFF):
        out["calls_top_%02x" % top] = b"".join(b"\xE8" + r.randbytes(3) + bytes([top]) for _ in range(700))
        out["dense_top_%02x" % top] = bytes(r.choice((0xE8, 0xE9, top, top, r.randrange(256))) for _ in range(4000))
    for gap in range(1, 8):         # 5 and 6: the distance at which the mask is reset
        unit = (b"\xE8" + b"\x00\xFF\x00\xFF\x00\xFF\x00")[:gap]
        out["spaced_%d" % gap] = unit * 400 + b"\x00" * 9
        out["spaced_%d_mixed" % gap] = b"".join((bytes([r.choice((0xE8, 0xE9))]) + bytes(r.choice((0, 0xFF, 0x12)) for _ in range(7)))[:gap]
                                                 for _ in range(400))
    for tail in range(0, 7):        # candidates in the last 5 bytes
        out["tail_%d" % tail] = r.randbytes(50) + b"\xE8" + b"\x00" * tail
        out["tail_ff_%d" % tail] = b"\x90" * 11 + b"\xE8\x01\x02\x03\xFF\xE8" + b"\xFF" * tail
    for n in range(0, 12):
        out["short_%d" % n] = (b"\xE8\x00\x00\x00\x00\xE9\xFF\xFF\xFF\xFF\xE8\x00")[:n]
    # one segment across a tile boundary: opcodes less than 6 apart from in front of the boundary to behind it
    out["segment_over_tile"] = r.randbytes(TILE - 40).replace(b"\xE8", b"\x00").replace(b"\xE9", b"\x00") + \
        b"".join(b"\xE8" + bytes(r.choice((0, 0xFF)) for _ in range(r.randrange(0, 5))) for _ in range(40)) + r.randbytes(300)
    out["real_code"] = real_code()
    return out


@functools.lru_cache(maxsize=None)
def dense(fid, seed, n):
    """candidate patterns of the filter every few bytes, noise between them"""
    r = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        k = r.randrange(4)
        if fid == DELTA:
            out += bytes((len(out) + j) * 3 & 0xFF for j in range(40)) + r.randbytes(3)
        elif k == 0:
            out += r.randbytes(r.randrange(1, 5))
        elif fid == X86:
            out += bytes([r.choice((0xE8, 0xE9))]) + r.randbytes(r.randrange(0, 4)) + bytes([r.choice((0, 0xFF))]) * r.randrange(1, 3)
        elif fid == ARM:
            out += r.randbytes(3) + b"\xEB"
        elif fid == POWERPC:
            out += bytes([0x48 | r.randrange(4)]) + r.randbytes(2) + bytes([(r.randrange(64) << 2) | 1])
        elif fid == SPARC:
            out += r.choice((bytes([0x40, r.randrange(0x40)]), bytes([0x7F, 0xC0 | r.randrange(0x40)]))) + r.randbytes(2)
        elif fid == ARMTHUMB:
            out += bytes([r.randrange(256), r.choice((0xF0, 0xF8)) | r.randrange(8)])
        else:           # IA-64: a bundle with a branch template and opcode 5 in some slots
            b = bytearray(r.randbytes(16))
            b[0] = (b[0] & 0xE0) | r.choice((0x10, 0x11, 0x12, 0x13, 0x16, 0x17, 0x18, 0x1C, 0x05))
            v = int.from_bytes(b, "little")
            for slot in range(3):
                if r.randrange(3):
                    at = 5 + 41 * slot
                    v &= ~((0xF << (at + 37)) | (0x7 << (at + 9)))
                    v |= 0x5 << (at + 37)
            out += v.to_bytes(16, "little")
    return bytes(out[:n])


def chained_block(plain, chain, cid=XB.CHECK_CRC64, sizes=True, **kw):
    """a block whose chain is `chain` [(id, prop)] then LZMA2, written by liblzma's encoders"""
    raw = lzma.compress(plain, format=lzma.FORMAT_RAW, filters=[spec(*f) for f in chain] + [dict(LZMA2, dict_size=1 << 20)])
    return XB.block(raw, plain, cid, comp=sizes, uncomp=sizes, extra_filters=[(fid, props(fid, p)) for fid, p in chain], **kw)


ALONE = [(DELTA, 4), (X86, 0), (POWERPC, 0x1000), (IA64, 0x20), (ARM, 0), (ARMTHUMB, 0xFFFFFFFE), (SPARC, 4)]
CHAINS = {"delta4_x86": [(DELTA, 4), (X86, 0)], "x86_delta1": [(X86, 0x1000), (DELTA, 1)], "delta_delta_delta": [(DELTA, 1), (DELTA, 255), (DELTA, 256)]}


@functools.lru_cache(maxsize=None)
def good_streams():
    """name -> image: streams every block of which liblzma decodes"""
    out = {}
    for fid, prop in ALONE:
        p = dense(fid, fid, 70001)
        out["alone_%02x" % fid] = XB.stream([chained_block(p, [(fid, prop)])], XB.CHECK_CRC64)
    for name, chain in CHAINS.items():
        p = dense(X86, len(name), 66000)
        out[name] = XB.stream([chained_block(p, chain, XB.CHECK_SHA256)], XB.CHECK_SHA256)
    mix = [[], [(X86, 0)], [(DELTA, 2)], [], [(ARM, 0)], [(DELTA, 4), (X86, 0)], [(ARMTHUMB, 0)], [], [(SPARC, 0)], [(IA64, 0)], [(POWERPC, 0)], [],
           [(DELTA, 256)], [(X86, 0xFFFFFFFB)], [(DELTA, 3), (DELTA, 3), (ARM, 4)], [(X86, 0)]]
    blocks = [chained_block(dense(c[-1][0] if c else X86, 40 + i, 5000 + 777 * i), c, XB.CHECK_CRC32) for i, c in enumerate(mix)]
    out["sixteen_mixed"] = XB.stream(blocks, XB.CHECK_CRC32)
    bare = [chained_block(dense(c[-1][0] if c else X86, 60 + i, 30000 + i), c, XB.CHECK_CRC64, sizes=False) for i, c in enumerate(mix[:6])]
    out["without_sizes"] = XB.stream(bare, XB.CHECK_CRC64)
    out["sized_and_bare"] = XB.stream([blocks[1], chained_block(dense(X86, 3, 9000), [(X86, 0)], XB.CHECK_CRC32, sizes=False), blocks[5]], XB.CHECK_CRC32)
    return out


def window_stream():
    """3.6 MB in blocks of 300 000 noise bytes with chains: windows of 1 MiB cut blocks"""
    chains = [[(X86, 0)], [(DELTA, 4)], [], [(ARM, 0), (DELTA, 1)]]
    return XB.stream([chained_block(XS.noise(60 + i, 300000), chains[i % 4], XB.CHECK_CRC32) for i in range(12)], XB.CHECK_CRC32)


@functools.lru_cache(maxsize=None)
def bad_streams():
    """name -> image: chains liblzma refuses (LZMA_OPTIONS_ERROR), and damaged data behind a sound chain"""
    t = XS.text(5, 3000)
    blk = lambda extra, **kw: XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, extra_filters=extra, **kw)], XB.CHECK_CRC32)     # noqa: E731
    out = {
        "delta_two_property_bytes": blk([(DELTA, b"\x00\x00")]),
        "delta_no_property": blk([(DELTA, b"")]),
        "bcj_three_property_bytes": blk([(X86, b"\x00\x00\x00")]),
        "bcj_five_property_bytes": blk([(ARM, b"\x00\x00\x00\x00\x00")]),
        "arm_offset_misaligned": blk([(ARM, struct.pack("<I", 2))]),
        "thumb_offset_misaligned": blk([(ARMTHUMB, struct.pack("<I", 1))]),
        "ia64_offset_misaligned": blk([(IA64, struct.pack("<I", 8))]),
        "lzma2_not_last": blk([(0x21, b"\x12"), (X86, b"")]),
        "lzma2_twice": blk([(X86, b""), (0x21, b"\x12")]),
        "bcj_last": blk([(DELTA, b"\x00")], filter_id=X86),
        "four_filters_none_lzma2": blk([(DELTA, b"\x00"), (X86, b""), (DELTA, b"\x03")], filter_id=DELTA, dict_byte=0),
        "unknown_filter_in_chain": blk([(X86, b""), (0x30, b"")]),
    }
    # a flipped byte in stored data: the check fails, over the unfiltered bytes
    p = XS.noise(33, 70000)
    good = chained_block(p, [(X86, 0)], XB.CHECK_CRC64)
    img = XB.stream([good], XB.CHECK_CRC64)
    at = img.index(good.image) + len(good.image) // 2
    out["flipped_stored_byte"] = XS.flip(img, at * 8 + 3)
    # an LZMA error at a known T: 74 008 filtered bytes in stored chunks, eight literals, then a match beyond the data
    for fid, prop in ((X86, 0), (DELTA, 4), (ARM, 0)):
        f = liblzma_filter([(fid, prop)], dense(fid, 90 + fid, 74000))
        w = XB.Lzma2Writer().raw_chunk(1, f[:65536]).raw_chunk(2, f[65536:])
        w.lzma_chunk(0xC0, XB.literals(b"abcdefgh") + [XB.Match(len(f) + 9, 4)] + XB.literals(b"zz"))
        out["lzma_error_%02x" % fid] = XB.stream([XB.block(w.image(), b"", XB.CHECK_CRC32, comp=False, uncomp=False,
                                                          extra_filters=[(fid, props(fid, prop))])], XB.CHECK_CRC32)
    return out


@functools.lru_cache(maxsize=None)
def near_boundary_streams():
    """name -> (image, plain): an LZMA error whose T lies within a few bytes of 64 KiB.  The block holds the FILTERED form
    of `plain` up to T -- stored chunks, then eight literals -- and then a match beyond the data."""
    out = {}
    for fid, prop in ((X86, 0), (ARM, 0), (IA64, 0)):
        plain = dense(fid, 70 + fid, 70000)
        f = liblzma_filter([(fid, prop)], plain)
        for t in range(65536 - 3, 65536 + 18):
            w = XB.Lzma2Writer().raw_chunk(1, f[:60000]).raw_chunk(2, f[60000:t - 8])
            w.lzma_chunk(0xC0, XB.literals(f[t - 8:t]) + [XB.Match(t + 1, 4)])
            out["%02x_T_%d" % (fid, t)] = (XB.stream([XB.block(w.image(), b"", XB.CHECK_CRC32, comp=False, uncomp=False,
                                                               extra_filters=[(fid, props(fid, prop))])], XB.CHECK_CRC32), plain)
    return out
