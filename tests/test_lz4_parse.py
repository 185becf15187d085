"""The plain LZ4 block reader of the compressor tests (streams.lz4_parse_block / lz4_execute) on the CPU: what it
regenerates from liblz4's own blocks must be the input, its extension-byte records must be what a hand-written block
holds, and blocks that do not end where they should are refused."""
import ctypes as C
import random

import pytest

import streams as S


def _liblz4():
    try:
        lz = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.fail("no liblz4.so.1 in this image")
    lz.LZ4_compress_default.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int]
    return lz


def _inputs():
    rnd = random.Random(0x124)
    words = [rnd.randbytes(rnd.randint(2, 11)) for _ in range(200)]
    yield b"".join(rnd.choice(words) for _ in range(9000))
    yield bytes(65536)
    yield b"ab" * 300 + rnd.randbytes(300) + b"xyz" * 7000
    yield rnd.randbytes(1000)
    yield rnd.randbytes(20) + bytes(16335 + 19) + rnd.randbytes(16350) + bytes(40)
    for n in (0, 1, 12, 13, 14, 15, 16, 28, 29, 30, 269, 270, 271, 284, 285, 286, 525, 600):
        yield rnd.randbytes(n)                      # literal runs around the extension steps
        yield rnd.randbytes(7) + bytes(n + 12)      # match lengths around them


def test_regenerates_what_liblz4_compressed():
    lz = _liblz4()
    n_seq = 0
    lit_ext, match_ext = set(), set()
    for data in _inputs():
        buf = C.create_string_buffer(len(data) + len(data) // 255 + 64)
        n = lz.LZ4_compress_default(data, buf, len(data), len(buf))
        assert n > 0
        seqs, exts = S.lz4_parse_block(buf.raw[:n])
        assert S.lz4_execute(seqs) == data
        assert len(seqs) == len(exts) and seqs[-1][1:] == (0, 0)
        for (lit, off, ml), (le, me) in zip(seqs, exts):
            assert le[0] == (0 if len(lit) < 15 else (len(lit) - 15) // 255 + 1)
            assert me[0] == (0 if ml - 4 < 15 else (ml - 4 - 15) // 255 + 1)
            assert le[1] == (None if le[0] == 0 else (len(lit) - 15) % 255) and me[1] == (None if me[0] == 0 else (ml - 19) % 255)
            lit_ext.add(min(le[0], 65)); match_ext.add(min(me[0], 65))
        n_seq += len(seqs)
    assert n_seq > 2000 and {0, 1, 2, 65} <= lit_ext and {0, 1, 2, 65} <= match_ext, (n_seq, lit_ext, match_ext)


def test_hand_written_blocks():
    seqs, exts = S.lz4_parse_block(bytes([0x1F]) + b"a" + b"\x01\x00" + b"\x0a" + b"\x50" + b"bcdef")
    assert seqs == [(b"a", 1, 29), (b"bcdef", 0, 0)] and exts == [((0, None), (1, 10)), ((0, None), (0, None))]
    assert S.lz4_execute(seqs) == b"a" * 30 + b"bcdef"
    seqs, exts = S.lz4_parse_block(bytes([0xF0, 255, 0]) + bytes(270))
    assert [len(s[0]) for s in seqs] == [270] and exts == [((2, 0), (0, None))]
    seqs, exts = S.lz4_parse_block(bytes([0xFF, 0]) + bytes(15) + b"\x03\x00" + bytes([255, 255, 7]) + b"\x50" + b"12345")
    assert (len(seqs[0][0]), seqs[0][1], seqs[0][2]) == (15, 3, 4 + 15 + 517) and exts[0] == ((1, 0), (3, 7))
    assert S.lz4_parse_block(b"\x00") == ([(b"", 0, 0)], [((0, None), (0, None))])
    for bad in (b"", b"\x10", b"\x11a", b"\x01\x01", b"\x1fa\x01\x00\xff", b"\xf0\xff", b"\x14a\x01\x00", b"\x10a\x01"):
        with pytest.raises(ValueError):
            S.lz4_parse_block(bad)
    with pytest.raises(AssertionError):
        S.lz4_execute([(b"ab", 3, 4), (b"", 0, 0)])
