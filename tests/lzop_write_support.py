"""Support for the lzop WRITE tests: the named inputs, accept(), which holds an image to the promised stream shape and to
the reference's read loop restated over the Python decoder (lzop_support.reference_read), and an instruction lister over
the rules of lzop_support.decode.

No liblzo2 and no lzop stand behind this file; see lzop_support.py for what pins the Python decoder."""
import collections
import functools
import struct
import zlib

import lzop_support as LS

BLOCK = 65536
HEADER_BYTES = 38
MAX_DIST = 49151
LEVELS = {1: (2, 1), 2: (1, 5), 3: (1, 5), 4: (1, 5), 5: (1, 5), 6: (1, 5), 7: (3, 7), 8: (3, 8), 9: (3, 9)}   # level -> (method, level byte)


def worst(n):
    """la_lzo_enc_dev.h's proven worst case for the stream of a block of n bytes"""
    return n + n // 7 + 4


def header(level=5, mtime=0):
    """the 38 bytes of archive_write_add_filter_lzop.c:103-132 with the level's method and level bytes"""
    method, lv = LEVELS[level]
    h = struct.pack(">HHHBBIIIIB", 0x1030, 0x0940, 0x0940, method, lv, 0x0300000D, 0o100644, mtime, 0, 0)
    return LS.MAGIC + h + struct.pack(">I", zlib.adler32(h))


def high(seed, n):
    """random bytes, all above 0x7F: they never continue a run of letters"""
    return bytes(b | 0x80 for b in LS.randbytes(seed, n))


def pair(dist):
    """a 64-byte random marker twice, `dist` apart, in a run of one byte: the run keeps the matcher's single-slot table
    from losing the first marker and makes the block compress, so a wrongly coded match cannot hide in a stored block"""
    b = bytearray(b"r" * BLOCK)
    b[100:164] = b[100 + dist:164 + dist] = high(dist, 64)
    return bytes(b)


def gaps(lengths, total):
    """runs of one letter (seven letters in turn, so later runs find earlier ones) separated by random bytes of the
    given lengths in turn"""
    out = bytearray()
    k = 0
    while len(out) < total:
        out += bytes([65 + k % 7]) * (20 + k % 13) + high(1000 + k, lengths[k % len(lengths)])
        k += 1
    return bytes(out[:total])


@functools.lru_cache(maxsize=None)
def inputs():
    t = LS.text(7, 3 * BLOCK + 5)
    mk = high(5, 6)
    return {
        "one_byte": t[:1], "three_bytes": t[:3], "four_bytes": t[:4],
        "block_minus_1": t[:BLOCK - 1], "block": t[:BLOCK], "block_plus_1": t[:BLOCK + 1], "three_blocks_plus_5": t,
        "noise_2b5": LS.randbytes(3, 2 * BLOCK + BLOCK // 2),
        "text_noise_text": LS.text(2, 40000) + LS.randbytes(4, 20000) + LS.text(3, 40000),
        "run_3b": b"\x07" * (3 * BLOCK),
        "period3": b"abc" * 20000 + LS.randbytes(6, 500),
        "pair_20000": pair(20000), "pair_40000": pair(40000), "pair_49151": pair(49151), "pair_49152": pair(49152),
        "short_far": b"a" * 100 + mk + b"b" * (20000 - 6) + mk + b"c" * 1000,
        "trails": gaps((0, 1, 2, 3), 30000),
        "lits": gaps((4, 5, 18, 19, 20, 273, 274, 300), 30000),
        "long_first": LS.randbytes(8, 300) + b"x" * 3000,
    }


Instruction = collections.namedtuple("Instruction", "form distance length trail at")


def instructions(stream):
    """[(form, distance, length, trail, at)] of one block's stream, by the rules of lzop_support.decode: `form` is
    decode's name of it, `length` the literal or match bytes, `at` the output position in front of the instruction.  A
    literal form has distance 0; the end has length 0."""
    src = bytes(stream)
    out, ip, op, state = [], 0, 0, 0

    def run(base):
        nonlocal ip
        n = base
        while src[ip] == 0:
            n += 255
            ip += 1
        ip += 1
        return n + src[ip - 1]

    if src[0] > 17:
        n = src[0] - 17
        out.append(Instruction("first_byte_short" if n < 4 else "first_byte_long", 0, n, 0, op))
        ip, op, state = 1 + n, n, min(n, 4)
    while True:
        t = src[ip]
        ip += 1
        if t < 16 and state == 0:
            n = (run(15) if t == 0 else t) + 3
            out.append(Instruction("literals_long" if t == 0 else "literals_short", 0, n, 0, op))
            ip, op, state = ip + n, op + n, 4
            continue
        if t < 16:
            dist, mlen, trail, form = (src[ip] << 2) + (t >> 2) + (2049 if state == 4 else 1), 3 if state == 4 else 2, t & 3, "m1_3byte" if state == 4 else "m1_2byte"
            ip += 1
        elif t >= 64:
            dist, mlen, trail, form = (src[ip] << 3) + ((t >> 2) & 7) + 1, (t >> 5) + 1, t & 3, "m2"
            ip += 1
        else:
            m3 = t >= 32
            mlen = t & (31 if m3 else 7)
            form = ("m3" if m3 else "m4") + ("_short" if mlen else "_long")
            if mlen == 0:
                mlen = run(31 if m3 else 7)
            mlen += 2
            w = src[ip] | (src[ip + 1] << 8)
            ip += 2
            trail = w & 3
            if m3:
                dist = (w >> 2) + 1
            else:
                d = ((t & 8) << 11) + (w >> 2)
                if d == 0:
                    out.append(Instruction("end", 0, 0, 0, op))
                    assert ip == len(src)
                    return out
                dist = d + 16384
        out.append(Instruction(form, dist, mlen, trail, op))
        ip, op, state = ip + trail, op + mlen + trail, trail


def literal_mask(stream, n):
    """bytearray of n: 1 where the block's byte came from a literal"""
    mask = bytearray(n)
    for i in instructions(stream):
        if i.distance == 0:
            mask[i.at:i.at + i.length] = b"\x01" * i.length
        elif i.trail:
            mask[i.at + i.length:i.at + i.length + i.trail] = b"\x01" * i.trail
    return mask


def accept(img, data, level=5, block_size=BLOCK, forms=None):
    """The image is the promised stream: the template header with the level's bytes, blocks of the promised cut, the
    closing word and nothing behind; no block longer than its input, every stream within the proven worst case; and the
    reference's read loop returns the input.  Returns [{"off", "usize", "csize", "adler", "stream" (None: stored)}]."""
    img, data = bytes(img), bytes(data)
    assert len(img) >= HEADER_BYTES + 4, len(img)
    mtime = struct.unpack_from(">I", img, 25)[0]
    assert img[:HEADER_BYTES] == header(level, mtime), img[:HEADER_BYTES].hex()
    assert struct.unpack_from(">I", img, 34)[0] == zlib.adler32(img[9:34])
    blocks, at, done = [], HEADER_BYTES, 0
    while True:
        usize = struct.unpack_from(">I", img, at)[0]
        if usize == 0:
            break
        csize, adler = struct.unpack_from(">II", img, at + 4)
        want = min(block_size, len(data) - done)
        assert usize == want, (len(blocks), usize, want)      # every block but the last is a whole one
        assert csize <= usize
        payload = img[at + 12:at + 12 + csize]
        assert len(payload) == csize
        assert adler == zlib.adler32(data[done:done + usize])
        # (a container cannot show more: what reaches usize is stored.  The bound on the size the coder COUNTED is held where
        # that count is visible, tests/test_lzo_encode_rules.py)
        assert csize <= worst(usize)
        blocks.append({"off": at, "usize": usize, "csize": csize, "adler": adler, "stream": payload if csize < usize else None})
        at += 12 + csize
        done += usize
    assert done == len(data) and at + 4 == len(img), (done, len(data), at, len(img))
    assert LS.reference_read(img, forms=forms) == (data, 0, "")
    return blocks
