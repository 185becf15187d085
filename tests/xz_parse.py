"""A small walker over a .xz image for the write tests: stream header, block headers (sizes, filter), LZMA2 chunk
headers, checks, index, footer.  It decodes nothing; it only follows the sizes the container states and asserts what the
format requires of them (CRC32s, zero padding, multiples of four)."""
import lzma
import struct
import zlib

MAGIC = b"\xFD7zXZ\x00"


def vli(buf, pos):
    v = 0
    for i in range(9):
        b = buf[pos + i]
        v |= (b & 0x7F) << (7 * i)
        if not b & 0x80:
            return v, pos + i + 1
    raise ValueError("variable-length integer longer than nine bytes")


def chunks(body):
    """[(control, uncompressed bytes, payload bytes or None when stored, offset of the control byte)] of LZMA2 data that
    ends with the end marker on body's last byte"""
    out, p = [], 0
    while True:
        c = body[p]
        if c == 0:
            assert p == len(body) - 1, "bytes behind the end marker"
            return out
        if c >= 0x80:
            usize = (((c & 0x1F) << 16) | (body[p + 1] << 8) | body[p + 2]) + 1
            csize = ((body[p + 3] << 8) | body[p + 4]) + 1
            hdr = 6 if c >= 0xC0 else 5
            out.append((c, usize, csize, p))
            p += hdr + csize
        else:
            assert c in (1, 2), c
            usize = ((body[p + 1] << 8) | body[p + 2]) + 1
            out.append((c, usize, None, p))
            p += 3 + usize


def walk(image):
    """ONE stream, nothing behind its footer.  Returns {"check": id, "blocks": [...], "records": [(unpadded, uncomp)],
    "index_off": n}; a block: off, header_size, comp, uncomp (None when the header leaves them out), dict_byte, data_off,
    unpadded, total, check (the field's bytes), chunks."""
    image = bytes(image)
    assert image[:6] == MAGIC and image[6] == 0
    assert struct.unpack("<I", image[8:12])[0] == zlib.crc32(image[6:8])
    check = image[7]
    cs = 0 if check == 0 else 4 if check <= 3 else 8 if check <= 6 else 16 if check <= 9 else 32 if check <= 12 else 64
    p, blocks = 12, []
    while image[p] != 0:
        hs = (image[p] + 1) * 4
        h = image[p:p + hs]
        assert struct.unpack("<I", h[-4:])[0] == zlib.crc32(h[:-4]), "block header CRC32"
        flags, q = h[1], 2
        assert flags & 0x3C == 0 and flags & 3 == 0, "one filter, no reserved bits"
        comp = uncomp = None
        if flags & 0x40:
            comp, q = vli(h, q)
        if flags & 0x80:
            uncomp, q = vli(h, q)
        fid, q = vli(h, q)
        psize, q = vli(h, q)
        assert fid == 0x21 and psize == 1
        dict_byte = h[q]
        assert not any(h[q + 1:-4]), "header padding"
        assert comp is not None, "the walker follows the compressed size"
        pad = -comp % 4
        assert not any(image[p + hs + comp:p + hs + comp + pad]), "block padding"
        body = image[p + hs:p + hs + comp]
        blocks.append({"off": p, "header_size": hs, "comp": comp, "uncomp": uncomp, "dict_byte": dict_byte, "data_off": p + hs,
                       "unpadded": hs + comp + cs, "total": hs + comp + pad + cs,
                       "check": image[p + hs + comp + pad:p + hs + comp + pad + cs], "chunks": chunks(body)})
        p += hs + comp + pad + cs
    index_off = p
    n, q = vli(image, p + 1)
    records = []
    for _ in range(n):
        a, q = vli(image, q)
        b, q = vli(image, q)
        records.append((a, b))
    while (q - index_off) % 4:
        assert image[q] == 0, "index padding"
        q += 1
    assert struct.unpack("<I", image[q:q + 4])[0] == zlib.crc32(image[index_off:q]), "index CRC32"
    q += 4
    f = image[q:q + 12]
    assert len(f) == 12 and f[10:] == b"YZ" and f[8:10] == image[6:8]
    assert struct.unpack("<I", f[:4])[0] == zlib.crc32(f[4:10]), "footer CRC32"
    assert (struct.unpack("<I", f[4:8])[0] + 1) * 4 == q - index_off, "backward size"
    assert q + 12 == len(image), "bytes behind the footer"
    return {"check": check, "blocks": blocks, "records": records, "index_off": index_off}


def raw_lzma2(body, dict_size=1 << 20):
    """liblzma on a block's body as raw LZMA2"""
    return lzma.decompress(body, format=lzma.FORMAT_RAW, filters=[{"id": lzma.FILTER_LZMA2, "dict_size": dict_size}])


def frame(blocks_image, first=True):
    """what la_gpu_xz_compress wrote (blocks back to back, the stream header in front under FIRST) as a whole stream:
    index and footer are added the way the write filter adds them"""
    body = bytes(blocks_image)
    head = body[:12] if first else MAGIC + b"\x00\x04" + struct.pack("<I", zlib.crc32(b"\x00\x04"))
    if first:
        body = body[12:]
    p, records = 0, []
    while p < len(body):
        hs = (body[p] + 1) * 4
        comp, q = vli(body, p + 2)
        uncomp, q = vli(body, q)
        records.append((hs + comp + 8, uncomp))
        p += hs + comp + (-comp % 4) + 8
    assert p == len(body)

    def enc(v):
        out = bytearray()
        while v >= 0x80:
            out.append((v & 0x7F) | 0x80)
            v >>= 7
        out.append(v)
        return bytes(out)
    ix = b"\x00" + enc(len(records)) + b"".join(enc(a) + enc(b) for a, b in records)
    ix += bytes(-len(ix) % 4)
    ix += struct.pack("<I", zlib.crc32(ix))
    tail = struct.pack("<I", len(ix) // 4 - 1) + b"\x00\x04"
    return head + body + ix + struct.pack("<I", zlib.crc32(tail)) + tail + b"YZ"
