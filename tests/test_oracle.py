"""Oracle pinning (CPU): the C restatement against the reference's own fixtures, the real
reference hash code (its stored outputs, and oracle/_ref when built), KATs and the documented
behaviour table."""
import hashlib
import json
import os
import random
import zlib

import pytest

import oracle_lib as O
import streams as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_fixtures")
MANIFEST = [e for e in json.load(open(os.path.join(GOLD, "manifest.json"))) if e["codec"] in ("lz4", "gzip")]


def test_hash_kats():
    assert O.xxh32(b"") == 0x02CC5D05
    assert O.xxh32(b"123456789") == 0x937BAD67
    assert O.crc32(b"123456789") == 0xCBF43926
    for flg_bd, hc in ((b"\x64\x70", 0xB9), (b"\x64\x40", 0xA7), (b"\x64\x50", 0x08), (b"\x64\x60", 0x85), (b"\x74\x40", 0xBD)):
        assert (O.xxh32(flg_bd) >> 8) & 0xFF == hc


def test_hash_against_real_reference_code():
    # the real reference code's outputs are stored (tests/golden/ref_outputs); where oracle/_ref is built, the live
    # reference code must still produce them
    gold = json.load(open(os.path.join(os.path.dirname(GOLD), "ref_outputs", "hash_vectors.json")))["vectors"]
    ref = O.ref_hash()
    rnd = random.Random(7)
    sizes = list(range(0, 70)) + [255, 256, 1000, 65536, 100003]
    assert [g["n"] for g in gold] == sizes
    for n, g in zip(sizes, gold):
        d = rnd.randbytes(n)
        s = rnd.getrandbits(32)
        assert hashlib.sha256(d).hexdigest() == g["input_sha256"] and s == g["seed"]
        assert O.xxh32(d, s) == g["xxh32"]
        k = rnd.randint(0, n)
        assert k == g["split"]
        if ref is not None:
            rx, rxs, rc = ref
            assert (rx(d, s), rxs([d[:k], d[k:]], s), rc(d)) == (g["xxh32"], g["xxh32_stream"], g["crc32"])
        assert O.xxh32_stream([d[:k], d[k:]], s) == g["xxh32_stream"] == g["xxh32"]
        assert O.crc32(d) == g["crc32"] == zlib.crc32(d)
        assert O.crc32(d[k:], O.crc32(d[:k])) == g["crc32"]
        assert O.crc32_combine(O.crc32(d[:k]), O.crc32(d[k:]), n - k) == g["crc32"]


@pytest.mark.parametrize("entry", MANIFEST, ids=[e["file"] for e in MANIFEST])
def test_reference_fixture_digests(entry):
    data = open(os.path.join(GOLD, entry["file"]), "rb").read()
    fn = O.lz4_stream_decode if entry["codec"] == "lz4" else O.gzip_stream_decode
    out, res = fn(data, entry["decoded_size"] + 4096)
    assert res.rc == 0 and res.errmsg == b""
    assert len(out) == entry["decoded_size"]
    assert hashlib.sha256(out.tobytes()).hexdigest() == entry["decoded_sha256"]


def test_reference_fixture_metadata():
    # libarchive/test/test_read_format_raw.c:122-148
    data = open(os.path.join(GOLD, "test_read_format_raw.data.gz"), "rb").read()
    out, res = O.gzip_stream_decode(data, 4096)
    assert out.tobytes() == b"foo\n"
    assert res.gz_name == b"test-file-name.data" and res.gz_mtime == 0x5CBAFD25
    assert O.gzip_bid(data) == 27
    lz = open(os.path.join(GOLD, "test_compat_lz4_1.tar.lz4"), "rb").read()
    assert O.lz4_bid(lz) == 48
    lg = open(os.path.join(GOLD, "test_compat_lz4_3.tar.lz4"), "rb").read()
    assert O.lz4_bid(lg) == 32
    # cat/test/test_expand.lz4 content checksum and cat/test/test_expand.gz trailer (Appendix B)
    ex = open(os.path.join(GOLD, "test_expand.lz4"), "rb").read()
    assert int.from_bytes(ex[-4:], "little") == 0x4B560639
    gz = open(os.path.join(GOLD, "test_expand.gz"), "rb").read()
    assert int.from_bytes(gz[-8:-4], "little") == 0x471DC33A and int.from_bytes(gz[-4:], "little") == 28


@pytest.mark.parametrize("name", sorted(S.appendix_d_lz4_cases()))
def test_lz4_behaviour_table(name):
    img, want, rc, msg = S.appendix_d_lz4_cases()[name]
    out, res = O.lz4_stream_decode(img, 1 << 20)
    assert (out.tobytes(), res.rc, res.errmsg.decode()) == (want, rc, msg)


def test_lz4_bid_rules():
    f = S.MAGIC + S.lz4_desc(0x64, 0x40) + bytes(8)
    assert O.lz4_bid(f) == 48
    assert O.lz4_bid(f[:10]) == 0                      # needs 11 bytes (lz4.c:150)
    assert O.lz4_bid(S.MAGIC + bytes([0x66, 0x40]) + bytes(8)) == 0   # reserved FLG bit
    assert O.lz4_bid(S.MAGIC + bytes([0x64, 0x41]) + bytes(8)) == 0   # reserved BD bit
    assert O.lz4_bid(S.MAGIC + bytes([0x64, 0x30]) + bytes(8)) == 0   # size id 3
    assert O.lz4_bid(S.MAGIC + bytes([0xA4, 0x40]) + bytes(8)) == 0   # version 2
    assert O.lz4_bid(S.LEGACY + bytes(8)) == 32


def test_gzip_behaviour_table():
    P = (b"All work and no play makes Jack a dull boy.\n" * 41)[:1800]
    ok = lambda img: O.gzip_stream_decode(img, 1 << 20)
    for img in (S.gz_member(P), S.gz_member(P, level=0), S.gz_member(P, strategy=zlib.Z_FIXED),
                S.gz_member(P, name=b"n", comment=b"c", extra=b"BC\x02\x00\x10\x00", hcrc=True)):
        out, res = ok(img)
        assert out.tobytes() == P and res.rc == 0
    # trailer CRC / ISIZE / header CRC16 wrong: ACCEPTED by the reference (F2), verdict reported separately
    for kw in ({"bad_crc": True}, {"bad_isize": True}):
        out, res = ok(S.gz_member(P, **kw))
        assert out.tobytes() == P and res.rc == 0 and res.gz_trailer_mismatch == 1
    m = S.gz_member(P)
    out, res = ok(m + S.gz_member(b"0123456789abc") + S.gz_member(b""))
    assert len(out) == 1813 and res.rc == 0
    for junk in (b"arbitrary junk", b"\x1f", b"\x1f\x8b\x08"):
        out, res = ok(m + junk)
        assert out.tobytes() == P and res.rc == 0
    out, res = ok(m + b"\x1f\x8b\x08\x20" + m[4:])     # reserved flag bit in the second header
    assert out.tobytes() == P and res.rc == 0
    out, res = ok(m[:40])
    assert (len(out), res.rc, res.errmsg) == (0, -30, b"truncated gzip input")
    out, res = ok(m[:-9])
    assert (len(out), res.rc, res.errmsg) == (0, -30, b"truncated gzip input")
    for cut in (4, 8):
        out, res = ok(m[:-cut])
        assert (len(out), res.rc, res.errmsg) == (0, -30, b"")


def test_gzip_metadata_snapshot():
    # name/mtime of the last header parsed during the first 64 KiB pull
    def three(n):
        return b"".join(S.gz_member(bytes([65 + i]) * n, name=nm, mtime=mt)
                        for i, (nm, mt) in enumerate(((b"first", 1000), (b"second", 2000), (b"third", 3000))))
    for n, nm, mt in ((5, b"third", 3000), (40000, b"second", 2000)):
        out, res = O.gzip_stream_decode(three(n), 1 << 20)
        assert (res.gz_name, res.gz_mtime, len(out)) == (nm, mt, 3 * n)
    img = S.gz_member(bytes(65536), name=b"first", mtime=1000) + S.gz_member(b"x", name=b"second", mtime=2000)
    out, res = O.gzip_stream_decode(img, 1 << 20)
    assert (res.gz_name, res.gz_mtime, len(out)) == (b"first", 1000, 65537)


def test_inflate_differential_against_system_zlib():
    rnd = random.Random(11)
    words = [rnd.randbytes(rnd.randint(1, 12)) for _ in range(40)]
    for t in range(300):
        n = rnd.randint(0, 5000)
        d = b"".join(rnd.choice(words) for _ in range(n // 6))[:n]
        co = zlib.compressobj(rnd.choice([0, 1, 6, 9]), zlib.DEFLATED, -15, 9,
                              rnd.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE]))
        c = co.compress(d) + co.flush()
        rc, cons, out = O.inflate_raw(c + b"tail", len(d) + 16)
        assert (rc, cons, out) == (0, len(c), d)
        m = bytearray(c)
        if m:
            m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
        try:
            z = zlib.decompressobj(-15)
            zo = z.decompress(bytes(m))
            kind = 0 if z.eof else 1
        except zlib.error:
            kind = 2
        if kind != 2 and len(zo) > 70000:
            continue
        rc, cons, out = O.inflate_raw(bytes(m), 70000)
        assert rc == kind
        if kind != 2:
            assert out == zo


def _lenient_classes(c: bytes):
    """Token walk of an LZ4 block (no output).  Returns (zero_offset, late_sequence):
    zero_offset   -- the chain meets a match offset of 0 (liblz4 1.9.3 lets it through, bytes indeterminate);
    late_sequence -- a sequence that is NOT the last one has its literals end inside the last 8 bytes of the
                     block: the format's end rule (and liblz4's safe loop, and this oracle) calls that
                     malformed, but 1.9.3's fast decode loop does not look for short literal runs."""
    ip, n = 0, len(c)
    zero = late = False
    while ip < n:
        tok = c[ip]; ip += 1
        ll = tok >> 4
        if ll == 15:
            while ip < n:
                x = c[ip]; ip += 1; ll += x
                if x != 255:
                    break
        ip += ll
        if ip + 2 > n:
            break
        if ip > n - 8:
            late = True
        if c[ip] == 0 and c[ip + 1] == 0:
            zero = True
        ip += 2
        if (tok & 15) == 15:
            while ip < n:
                x = c[ip]; ip += 1
                if x != 255:
                    break
    return zero, late


def _has_zero_offset(c: bytes) -> bool:
    """Token walk of an LZ4 block (no output): does the chain meet a match offset of 0?"""
    ip, n = 0, len(c)
    while ip < n:
        tok = c[ip]; ip += 1
        ll = tok >> 4
        if ll == 15:
            while ip < n:
                x = c[ip]; ip += 1; ll += x
                if x != 255:
                    break
        ip += ll
        if ip + 2 > n:
            return False
        if c[ip] == 0 and c[ip + 1] == 0:
            return True
        ip += 2
        if (tok & 15) == 15:
            while ip < n:
                x = c[ip]; ip += 1
                if x != 255:
                    break
    return False


def test_lz4_block_differential_against_system_liblz4():
    import ctypes as C
    try:
        l = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("no system liblz4")
    l.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    rnd = random.Random(5)
    words = [rnd.randbytes(rnd.randint(1, 12)) for _ in range(40)]
    for t in range(400):
        n = rnd.randint(0, 5000)
        d = b"".join(rnd.choice(words) for _ in range(n // 6))[:n]
        c = S.lz4_compress_block(d)
        cap = rnd.choice([len(d), len(d) + 3, len(d) + 20, 65536])
        assert O.lz4_block_decode(c, cap) == d
        m = bytearray(c)
        for _ in range(rnd.randint(1, 3)):
            m[rnd.randrange(len(m))] = rnd.getrandbits(8)
        if rnd.random() < 0.3 and len(m) > 2:
            m = m[:rnd.randrange(1, len(m))]
        m = bytes(m)
        buf = C.create_string_buffer(cap + 1)
        r = l.LZ4_decompress_safe(m, buf, len(m), cap)
        mine = O.lz4_block_decode(m, cap)
        if mine is None:
            # liblz4 may only disagree (accept what the oracle rejects) on the two documented input
            # classes (deliberate divergences): a match with offset 0, and a non-final
            # sequence whose literals end inside the block's last 8 bytes (fast-loop laxity of 1.9.3)
            assert r < 0 or any(_lenient_classes(m)), "oracle rejects a block liblz4 accepts, outside the documented classes"
            continue
        assert r >= 0 and mine == buf.raw[:r]
