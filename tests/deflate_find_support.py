"""Support for the block-start tests (LA_GZ_OPT_BLOCK_STARTS, libarchive_amd/csrc/la_deflate_find_dev.h).

Two referees, neither of them the code under test:
  block_starts(body)   the TRUE block starts of a raw-deflate stream: the image's zlib through ctypes, inflate(Z_BLOCK),
                       which returns behind every end-of-block code with the count of unused bits in data_type;
  is_candidate(...)    the candidate rule in plain Python, written from RFC 1951 3.2.7 and zlib 1.2.11's inflate.c /
                       inftrees.c (a non-final dynamic block header zlib accepts, every bit of it inside the span).
"""
import ctypes as C
import random
import zlib

import deflate_support as DS

Z_BLOCK = 5
CLC_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
WORDS = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave", b"boundary", b"history", b"the", b"of",
         b"candidate", b"header", b"block", b"bit", b"confirm", b"refute", b"a", b"walk", b"table", b"code", b"length", b"distance"]


def word_text(n, seed=7):
    """text whose level-6 body has blocks of a few tens of KiB: words in a random order with random numbers between"""
    r = random.Random(seed)
    out, size = [], 0
    while size < n:
        w = r.choice(WORDS) if r.random() < 0.85 else b"%d" % r.randrange(100000)
        out.append(w)
        size += len(w) + 1
    return b" ".join(out)[:n]


def raw_deflate(plain, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, zdict=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy, zdict) if zdict else zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def block_starts(body):
    """[(bit offset, bfinal, btype)] of every block of the raw-deflate stream `body`, by zlib's own walk"""
    z = DS.libz()
    s = DS._ZStream()
    rc = z.inflateInit2_(C.byref(s), -15, z.zlibVersion(), C.sizeof(DS._ZStream))
    assert rc == DS.Z_OK, rc
    src = C.create_string_buffer(bytes(body), max(len(body), 1))
    osz = 1 << 22
    obuf = C.create_string_buffer(osz)
    bits = int.from_bytes(body, "little")
    starts = {0}
    try:
        s.next_in, s.avail_in = C.addressof(src), len(body)
        while True:
            s.next_out, s.avail_out = C.addressof(obuf), osz
            rc = z.inflate(C.byref(s), Z_BLOCK)
            if rc == DS.Z_STREAM_END:
                break
            assert rc == DS.Z_OK, (rc, s.msg)
            if s.data_type & 128:
                starts.add(int(s.total_in) * 8 - (s.data_type & 63))
    finally:
        z.inflateEnd(C.byref(s))
    out = []
    for p in sorted(starts):
        out.append((p, (bits >> p) & 1, (bits >> (p + 1)) & 3))
        if out[-1][1]:          # (zlib also returns behind the end-of-block code of the final block: nothing starts there)
            break
    return out


def true_candidates(body, behind=0):
    """the starts of the non-final dynamic blocks behind bit `behind`: what the finder must not miss"""
    return [p for p, fin, typ in block_starts(body) if fin == 0 and typ == 2 and p > behind]


class _Bits:
    def __init__(self, value, pos, end):
        self.v, self.pos, self.end = value, pos, end

    def take(self, n):
        if self.pos + n > self.end:
            return None
        x = (self.v >> self.pos) & ((1 << n) - 1)
        self.pos += n
        return x


def _code_state(lens):
    """inftrees.c: (over-subscribed, incomplete, longest length) of a set of code lengths"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    left = 1
    for l in range(1, 16):
        left = (left << 1) - count[l]
        if left < 0:
            return True, False, max(l for l in range(16) if count[l] or l == 0)
    mx = max([l for l in range(1, 16) if count[l]], default=0)
    return False, left > 0, mx


def _clc_decoder(cl):
    """canonical code of the 19 code-length-code lengths: {(length, code msb-first): symbol}"""
    table, code = {}, 0
    for l in range(1, 8):
        for s in range(19):
            if cl[s] == l:
                table[(l, code)] = s
                code += 1
        code <<= 1
    return table


def is_candidate_value(value, p, end_bits):
    """value: the span as one little-endian integer (bit k of the stream is bit k of it)"""
    r = _Bits(value, p, end_bits)
    if r.take(3) != 4:                          # BFINAL 0, then BTYPE 10 (first bit lowest)
        return False
    h = r.take(14)
    if h is None:
        return False
    nlen, ndist, ncode = (h & 31) + 257, ((h >> 5) & 31) + 1, (h >> 10) + 4
    if nlen > 286 or ndist > 30:
        return False
    cl = [0] * 19
    for i in range(ncode):
        v = r.take(3)
        if v is None:
            return False
        cl[CLC_ORDER[i]] = v
    over, incomplete, mx = _code_state(cl)
    if over or incomplete:                      # (inflate_table(CODES): an incomplete set is refused; the all-zero one, which
        return False                            # zlib reads as one-bit zeros, ends without an end-of-block code)
    table = _clc_decoder(cl)
    lens = []
    while len(lens) < nlen + ndist:
        code, sym = 0, None
        for l in range(1, 8):
            b = r.take(1)
            if b is None:
                return False
            code = (code << 1) | b
            if (l, code) in table:
                sym = table[(l, code)]
                break
        if sym is None:
            return False
        if sym < 16:
            lens.append(sym)
            continue
        x = r.take({16: 2, 17: 3, 18: 7}[sym])
        if x is None:
            return False
        if sym == 16:
            if not lens:
                return False
            val, rep = lens[-1], 3 + x
        else:
            val, rep = 0, (3 if sym == 17 else 11) + x
        if len(lens) + rep > nlen + ndist:
            return False
        lens += [val] * rep
    if lens[256] == 0:
        return False
    over, incomplete, mx = _code_state(lens[:nlen])
    if over or (incomplete and mx != 1):        # inflate_table(LENS): incomplete only as the lone 1-bit code
        return False
    over, incomplete, mx = _code_state(lens[nlen:])
    if over or (incomplete and mx > 1):         # inflate_table(DISTS): the same, and the empty code
        return False
    return True


HEADER_BYTES = 600      # above the longest header: 17 + 57 + 316 * (7 + 7) bits


def is_candidate(data, p, end_bits=None):
    end_bits = 8 * len(data) if end_bits is None else end_bits
    i = p >> 3
    return is_candidate_value(int.from_bytes(data[i:i + HEADER_BYTES], "little"), p & 7, end_bits - 8 * i)


def model_candidates(data, end_bits=None):
    """every candidate bit position of `data`, by the Python model"""
    end_bits = 8 * len(data) if end_bits is None else end_bits
    out = []
    for i in range(len(data)):
        w = int.from_bytes(data[i:i + 2], "little")
        for j in range(8):
            if (w >> j) & 7 == 4 and is_candidate(data, 8 * i + j, end_bits):
                out.append(8 * i + j)
    return out


# ---------------------------------------------------------------- streams of the filter tests (CPU stand-in and device)

GZ_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def gz_member(body, plain, crc=None, isize=None):
    crc = zlib.crc32(plain) & 0xFFFFFFFF if crc is None else crc
    isize = len(plain) & 0xFFFFFFFF if isize is None else isize
    return GZ_HEADER + body + crc.to_bytes(4, "little") + isize.to_bytes(4, "little")


def second_block_at(phase):
    """D D D(final) by tests/deflate_build.py, the second block starting at bit `phase` of its byte: image, plain, info"""
    import deflate_build as B
    t1, t2, t3 = (list(word_text(300, seed=s)) for s in (1, 2, 3))
    for pad in range(64):
        blocks = [B._dyn_auto(t1 + [65 + (pad * 7 + i) % 26 for i in range(pad)], random.Random(10 + phase), final=0),
                  B._dyn_auto(t2 + [B.M(40, 300), B.M(258, 500)], random.Random(20 + phase), final=0),
                  B._dyn_auto(t3 + [B.M(100, 700)], random.Random(phase), final=1)]
        image, plain, valid, _, info = B.build(blocks)
        assert valid
        if info["block_bits"][1] % 8 == phase:
            return image, plain, info
    raise AssertionError("no padding puts the second block at bit %d" % phase)


def far_match_stream():
    """Stored(32 768 bytes), then a dynamic block whose FIRST symbol is a match of 258 at distance 32 768, then a final
    fixed block: image, plain, info, the stored bytes"""
    import deflate_build as B
    base = bytes((i * 7 + (i >> 8)) & 255 for i in range(32768))
    blocks = [B.Stored(base, final=0), B._dyn_auto([B.M(258, 32768), 66, B.M(258, 32768)], random.Random(4), final=0),
              B.Fixed(list(b"end"), final=1)]
    image, plain, valid, _, info = B.build(blocks)
    assert valid
    return image, plain, info, base


_filter_streams = None


def filter_streams():
    """name -> gzip image of ONE member (good and damaged ones): what the block-start mode of the read filter is held to"""
    global _filter_streams
    if _filter_streams is not None:
        return _filter_streams
    out = {}
    text = word_text(600000, seed=21)
    for level in (6, 9, 1):
        out["text-level-%d" % level] = gz_member(raw_deflate(text, level), text)
    out["text-fixed-blocks"] = gz_member(raw_deflate(text[:300000], 6, zlib.Z_FIXED), text[:300000])
    for phase in range(8):
        image, plain, _ = second_block_at(phase)
        out["second-block-at-bit-%d" % phase] = gz_member(image, plain)
    image, plain, _, _ = far_match_stream()
    out["match-into-the-piece-before"] = gz_member(image, plain)
    inner = raw_deflate(word_text(300000, seed=9), 6)
    out["deflate-body-inside-stored-blocks"] = gz_member(raw_deflate(inner, 0), inner)
    noise = random.Random(77).randbytes(262144)
    out["noise-stored-blocks"] = gz_member(raw_deflate(noise, 6), noise)
    body = raw_deflate(text, 6)
    starts = [p for p, _, _ in block_starts(body)]
    whole = gz_member(body, text)
    for name, cut in (("cut-inside-a-header", starts[2] // 8 + 6), ("cut-inside-a-block", (starts[2] + starts[3]) // 16),
                      ("cut-after-a-block", (starts[3] + 7) // 8), ("cut-inside-the-trailer", len(body) + 5)):
        out[name] = whole[:len(GZ_HEADER) + cut]
    import deflate_support as DS
    for at in range(starts[2] + 3, starts[3]):       # (the first flip zlib refuses: in the header, most do)
        bad = bytearray(body)
        bad[at // 8] ^= 1 << (at % 8)
        if DS.zlib_inflate(bytes(bad))[0] == "data":
            break
    out["flipped-bit-in-the-third-block"] = gz_member(bytes(bad), text)
    out["wrong-crc32"] = gz_member(body, text, crc=zlib.crc32(text) ^ 1)
    out["wrong-isize"] = gz_member(body, text, isize=len(text) + 1)
    small = word_text(50000, seed=3)
    out["second-member-behind-the-first"] = whole + gz_member(raw_deflate(small, 6), small) + gz_member(raw_deflate(small[:999], 9), small[:999])
    _filter_streams = out
    return out
