"""Builders for the xz tests.

Container: block() wraps raw LZMA2 data in a block header (any of its options), padding and check; stream() puts blocks
between stream header, index and footer.  Every part can be written wrong on purpose.  Raw LZMA2 data comes from
lzma2() (Python's lzma, FORMAT_RAW) or from the encoder below.

Encoder: Lzma2Writer turns a chunk plan -- uncompressed chunks and LZMA chunks given as explicit packet lists (literal,
match, rep0..3, short rep) -- into LZMA2 bytes, so that tests can hand-build the paths an ordinary encoder rarely takes.
It is a plain LZMA range encoder (the arithmetic of the LZMA SDK's specification); it decides nothing itself."""
import collections
import ctypes as C
import functools
import hashlib
import lzma
import struct
import zlib

CHECK_NONE, CHECK_CRC32, CHECK_CRC64, CHECK_SHA256 = 0, 1, 4, 10
HEADER_MAGIC, FOOTER_MAGIC = b"\xFD7zXZ\x00", b"YZ"

Block = collections.namedtuple("Block", "image unpadded uncomp")


def check_size(cid):
    return 0 if cid == 0 else 4 if cid <= 3 else 8 if cid <= 6 else 16 if cid <= 9 else 32 if cid <= 12 else 64


def vli(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def crc64(data):
    lib = C.CDLL("liblzma.so.5")
    lib.lzma_crc64.restype = C.c_uint64
    lib.lzma_crc64.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64]
    return lib.lzma_crc64(bytes(data), len(data), 0)


def check_value(cid, plain):
    if cid == CHECK_CRC32:
        return struct.pack("<I", zlib.crc32(plain))
    if cid == CHECK_CRC64:
        return struct.pack("<Q", crc64(plain))
    if cid == CHECK_SHA256:
        return hashlib.sha256(plain).digest()
    return bytes(range(1, check_size(cid) + 1))      # an ID liblzma does not verify: anything


@functools.lru_cache(maxsize=None)
def lzma2(plain, lc=3, lp=0, pb=2, dict_size=1 << 20, preset=6):
    return lzma.compress(plain, format=lzma.FORMAT_RAW,
                         filters=[{"id": lzma.FILTER_LZMA2, "preset": preset, "lc": lc, "lp": lp, "pb": pb, "dict_size": dict_size}])


def block(raw, plain, cid, comp=True, uncomp=True, comp_value=None, uncomp_value=None, dict_byte=18, flags_or=0, filter_id=0x21,
          header_pad=b"", pad_byte=0, extra_filters=()):
    """One block: header (sizes present or not, or written wrong), raw LZMA2 data, padding, the check over `plain`."""
    flags = (0x40 if comp else 0) | (0x80 if uncomp else 0) | len(extra_filters) | flags_or
    body = bytes([flags])
    if comp:
        body += vli(len(raw) if comp_value is None else comp_value)
    if uncomp:
        body += vli(len(plain) if uncomp_value is None else uncomp_value)
    for fid, props in extra_filters:
        body += vli(fid) + vli(len(props)) + props
    body += vli(filter_id) + vli(1) + bytes([dict_byte]) + header_pad
    size = (1 + len(body) + 4 + 3) // 4 * 4
    head = bytes([size // 4 - 1]) + body + bytes(size - 4 - 1 - len(body))
    head += struct.pack("<I", zlib.crc32(head))
    chk = check_value(cid, plain)
    image = head + raw + bytes([pad_byte]) * (-len(raw) % 4) + chk
    return Block(image, size + len(raw) + len(chk), len(plain))


def stream(blocks, cid, records=None, index_pad=None, backward_delta=0, footer_check=None, header_flags=None):
    flags = bytes([0, cid]) if header_flags is None else header_flags
    out = HEADER_MAGIC + flags + struct.pack("<I", zlib.crc32(flags))
    for b in blocks:
        out += b.image
    if records is None:
        records = [(b.unpadded, b.uncomp) for b in blocks]
    index = b"\x00" + vli(len(records)) + b"".join(vli(u) + vli(n) for u, n in records)
    pad = bytes(-len(index) % 4)
    if index_pad is not None and pad:
        pad = (index_pad * 4)[:len(pad)]
    index += pad
    index += struct.pack("<I", zlib.crc32(index))
    fflags = bytes([0, cid if footer_check is None else footer_check])
    tail = struct.pack("<I", len(index) // 4 - 1 + backward_delta) + fflags
    return out + index + struct.pack("<I", zlib.crc32(tail)) + tail + FOOTER_MAGIC


# ---- the LZMA range encoder -----------------------------------------------------------------------------------

Lit = collections.namedtuple("Lit", "byte")
Match = collections.namedtuple("Match", "dist len")        # dist 1 = the byte just written
Rep = collections.namedtuple("Rep", "index len")            # index 0..3
ShortRep = collections.namedtuple("ShortRep", "")

P_IS_MATCH, P_IS_REP, P_IS_REP0, P_IS_REP1, P_IS_REP2, P_IS_REP0_LONG = 0, 192, 204, 216, 228, 240
P_DIST_SLOT, P_DIST_SPECIAL, P_DIST_ALIGN, P_LEN, P_REP_LEN, P_LITERAL = 432, 688, 802, 818, 1332, 1846


class _RangeEncoder:
    def __init__(self):
        self.low, self.range, self.cache, self.cache_size, self.out = 0, 0xFFFFFFFF, 0, 1, bytearray()

    def _shift_low(self):
        if self.low < 0xFF000000 or self.low >= 1 << 32:
            carry, tmp = self.low >> 32, self.cache
            while True:
                self.out.append((tmp + carry) & 0xFF)
                tmp = 0xFF
                self.cache_size -= 1
                if self.cache_size == 0:
                    break
            self.cache = (self.low >> 24) & 0xFF
        self.cache_size += 1
        self.low = (self.low & 0x00FFFFFF) << 8

    def _normalise(self):
        while self.range < 1 << 24:
            self.range = (self.range << 8) & 0xFFFFFFFF
            self._shift_low()

    def bit(self, probs, i, b):
        p = probs[i]
        bound = (self.range >> 11) * p
        if b == 0:
            self.range = bound
            probs[i] = p + ((2048 - p) >> 5)
        else:
            self.low += bound
            self.range -= bound
            probs[i] = p - (p >> 5)
        self._normalise()

    def direct(self, value, nbits):
        for i in reversed(range(nbits)):
            self.range >>= 1
            if (value >> i) & 1:
                self.low += self.range
            self._normalise()

    def finish(self):
        for _ in range(5):
            self._shift_low()
        return bytes(self.out)


class Lzma2Writer:
    """lzma_chunk(control, packets, props=(lc, lp, pb)) and raw_chunk(control, data) append chunks; image() ends the
    data with 0x00.  control is the kind (0x80, 0xA0, 0xC0, 0xE0; 1, 2): the size bits are filled in.  The writer keeps
    the model the way a decoder has to after that control byte, whether or not liblzma accepts the sequence."""

    def __init__(self):
        self.chunks, self.hist, self.dict_start = [], bytearray(), 0
        self.log = []       # (packet, bytes written when it was coded), for tests that check what a case holds
        self.lc, self.lp, self.pb = 3, 0, 2
        self._reset()

    def _reset(self):
        self.probs = [1024] * (P_LITERAL + (768 << (self.lc + self.lp)))
        self.state, self.reps = 0, [0, 0, 0, 0]

    def raw_chunk(self, control, data):
        assert 1 <= len(data) <= 1 << 16
        if control == 1:
            self.dict_start = len(self.hist)
        self.chunks.append(bytes([control]) + struct.pack(">H", len(data) - 1) + bytes(data))
        self.hist += data
        return self

    def lzma_chunk(self, control, packets, props=None):
        if control >= 0xC0:
            self.lc, self.lp, self.pb = props or (self.lc, self.lp, self.pb)
        if control >= 0xA0:
            self._reset()
        if control >= 0xE0:
            self.dict_start = len(self.hist)
        rc, start = _RangeEncoder(), len(self.hist)
        for pk in packets:
            self._packet(rc, pk)
        data, usize = rc.finish(), len(self.hist) - start
        assert 1 <= usize <= 1 << 21 and 1 <= len(data) <= 1 << 16, (usize, len(data))
        head = bytes([control | ((usize - 1) >> 16)]) + struct.pack(">HH", (usize - 1) & 0xFFFF, len(data) - 1)
        if control >= 0xC0:
            head += bytes([(self.pb * 5 + self.lp) * 9 + self.lc])
        self.chunks.append(head + data)
        return self

    def lzma_chunk_until(self, control, packets, csize):
        """an LZMA chunk that takes packets until its compressed data is exactly csize bytes (it has to come out even)"""
        if control >= 0xA0:
            self._reset()
        if control >= 0xE0:
            self.dict_start = len(self.hist)
        rc, start = _RangeEncoder(), len(self.hist)
        for pk in packets:
            self._packet(rc, pk)
            if len(rc.out) + rc.cache_size + 4 >= csize:
                break
        data, usize = rc.finish(), len(self.hist) - start
        assert len(data) == csize, (len(data), csize)
        head = bytes([control | ((usize - 1) >> 16)]) + struct.pack(">HH", (usize - 1) & 0xFFFF, len(data) - 1)
        if control >= 0xC0:
            head += bytes([(self.pb * 5 + self.lp) * 9 + self.lc])
        self.chunks.append(head + data)
        return self

    def image(self):
        return b"".join(self.chunks) + b"\x00"

    def plain(self):
        return bytes(self.hist)

    # -- one packet
    def _len(self, rc, base, n, pos_state):
        n -= 2
        if n < 8:
            rc.bit(self.probs, base, 0)
            self._tree(rc, base + 2 + pos_state * 8, 3, n)
        elif n < 16:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 0)
            self._tree(rc, base + 130 + pos_state * 8, 3, n - 8)
        else:
            rc.bit(self.probs, base, 1)
            rc.bit(self.probs, base + 1, 1)
            self._tree(rc, base + 258, 8, n - 16)

    def _tree(self, rc, base, nbits, value):
        sym = 1
        for i in reversed(range(nbits)):
            b = (value >> i) & 1
            rc.bit(self.probs, base + sym, b)
            sym = (sym << 1) | b

    def _reverse_tree(self, rc, base, nbits, value):
        sym = 1
        for i in range(nbits):
            b = (value >> i) & 1
            rc.bit(self.probs, base + sym, b)
            sym = (sym << 1) | b

    def _copy(self, dist0, n):
        for _ in range(n):
            self.hist.append(self.hist[-dist0 - 1] if dist0 < len(self.hist) else 0)   # (a distance beyond the data: any byte)

    def _packet(self, rc, pk):
        pos = len(self.hist)
        self.log.append((pk, pos))
        pos_state, st, pr = pos & ((1 << self.pb) - 1), self.state, self.probs
        if isinstance(pk, Lit):
            rc.bit(pr, P_IS_MATCH + st * 16 + pos_state, 0)
            prev = self.hist[-1] if pos > self.dict_start else 0      # (the byte in front of a dictionary reset reads as 0)
            lit = P_LITERAL + 768 * (((pos & ((1 << self.lp) - 1)) << self.lc) + (prev >> (8 - self.lc)))
            sym = 1
            if st < 7:
                for i in reversed(range(8)):
                    b = (pk.byte >> i) & 1
                    rc.bit(pr, lit + sym, b)
                    sym = (sym << 1) | b
            else:
                m, offset = self.hist[-self.reps[0] - 1] << 1, 0x100
                for i in reversed(range(8)):
                    match_bit, b = m & offset, (pk.byte >> i) & 1
                    rc.bit(pr, lit + offset + match_bit + sym, b)
                    sym = (sym << 1) | b
                    offset = offset & match_bit if b else offset & ~match_bit
                    m <<= 1
            self.hist.append(pk.byte)
            self.state = 0 if st < 4 else st - 3 if st < 10 else st - 6
            return
        rc.bit(pr, P_IS_MATCH + st * 16 + pos_state, 1)
        if isinstance(pk, Match):
            rc.bit(pr, P_IS_REP + st, 0)
            self._len(rc, P_LEN, pk.len, pos_state)
            d = pk.dist - 1
            slot = d if d < 4 else 2 * (d.bit_length() - 1) + ((d >> (d.bit_length() - 2)) & 1)
            self._tree(rc, P_DIST_SLOT + min(pk.len - 2, 3) * 64, 6, slot)
            if slot >= 4:
                nb = (slot >> 1) - 1
                base = (2 | (slot & 1)) << nb
                if slot < 14:
                    self._reverse_tree(rc, P_DIST_SPECIAL + base - slot - 1, nb, d - base)
                else:
                    rc.direct((d - base) >> 4, nb - 4)
                    self._reverse_tree(rc, P_DIST_ALIGN, 4, (d - base) & 15)
            self.reps = [d] + self.reps[:3]
            self.state = 7 if st < 7 else 10
            self._copy(d, pk.len)
            return
        rc.bit(pr, P_IS_REP + st, 1)
        if isinstance(pk, ShortRep):
            rc.bit(pr, P_IS_REP0 + st, 0)
            rc.bit(pr, P_IS_REP0_LONG + st * 16 + pos_state, 0)
            self.state = 9 if st < 7 else 11
            self._copy(self.reps[0], 1)
            return
        k = pk.index
        if k == 0:
            rc.bit(pr, P_IS_REP0 + st, 0)
            rc.bit(pr, P_IS_REP0_LONG + st * 16 + pos_state, 1)
        else:
            rc.bit(pr, P_IS_REP0 + st, 1)
            if k == 1:
                rc.bit(pr, P_IS_REP1 + st, 0)
            else:
                rc.bit(pr, P_IS_REP1 + st, 1)
                rc.bit(pr, P_IS_REP2 + st, k - 2)
            d = self.reps.pop(k)
            self.reps.insert(0, d)
        self._len(rc, P_REP_LEN, pk.len, pos_state)
        self.state = 8 if st < 7 else 11
        self._copy(self.reps[0], pk.len)


def literals(data):
    return [Lit(b) for b in data]
