"""The gzip read filter in piece mode (LA_GZIP_FLUSH_POINTS=1): ONE member decoded from its flush points, a piece per
lane or wave, confirmed in stream order (la_filter_gzip.c, la_gz_pieces_build).  Through la_api.cat (= bsdcat) with
1 MiB windows, so that a member of a few MiB spans several.

Expected bytes are the plain input (zlib wrote or checked every stream); expected byte counts in front of an error are
the CPU filter model's (oracle/orc_filters.c through oracle_lib.gzip_stream_decode) for the same damaged stream."""
import random
import struct
import zlib

import pytest

import la_api
import oracle_lib as O
from test_gpu_lz4_write import ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu

ARCHIVE_FILTER_GZIP = 1
MARKER = b"\x00\x00\xff\xff"
WORDS = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave", b"boundary", b"history"]
STEP = 30000


def word_text(n, seed):
    r = random.Random(seed)
    return b" ".join(r.choice(WORDS) for _ in range(n // 4))[:n]


def trailer(plain):
    return struct.pack("<II", zlib.crc32(plain) & 0xFFFFFFFF, len(plain) & 0xFFFFFFFF)


def flushed_body(plain, flush, step=STEP, level=6, finish=True):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    pieces = [c.compress(plain[i:i + step]) + c.flush(flush) for i in range(0, len(plain), step)]
    return pieces, (c.flush() if finish else b"")


def member(body, plain, header=b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"):
    return header + body + trailer(plain)


@pytest.fixture(scope="module")
def plain():
    # text, a stretch of random bytes (stored blocks) and zeros: 3.3 MiB, a few windows of 1 MiB of compressed bytes
    return word_text(2_500_000, 1) + random.Random(2).randbytes(2_600_000) + bytes(300_000) + word_text(400_000, 3)


@pytest.fixture(scope="module")
def full_member(plain):
    pieces, tail = flushed_body(plain, zlib.Z_FULL_FLUSH)
    return pieces, tail, member(b"".join(pieces) + tail, plain)


@pytest.fixture()
def piece_mode(monkeypatch):
    monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", "1")
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    return monkeypatch


def cat(img, **kw):
    r = la_api.cat(img, **kw)
    return la_api.as_reference_tuple(r)


def test_own_writer_single_member_over_several_windows(gpu_ctx, plain, piece_mode):
    rc, img = write_lz4(plain, (("single-member", "1"),), 65537, codec="gzip")
    assert rc == ARCHIVE_OK and len(img) > 3 << 20 and zlib.decompress(img, 31) == plain
    piece_mode.setenv("LA_GPU_TRACE", "0")
    assert cat(img) == (plain, 0, "")
    assert cat(img, read_size=4099) == (plain, 0, "")
    # with the switch unset: today's path, the same bytes; and the default policy does not bid for it
    piece_mode.delenv("LA_GZIP_FLUSH_POINTS")
    assert cat(img) == (plain, 0, "")
    piece_mode.setenv("LA_GPU_BID", "auto")
    r = la_api.cat(img)
    assert ARCHIVE_FILTER_GZIP not in [c for c, _ in r.filters] and r.data == img
    piece_mode.setenv("LA_GZIP_FLUSH_POINTS", "1")
    r = la_api.cat(img)
    assert ARCHIVE_FILTER_GZIP in [c for c, _ in r.filters] and r.data == plain


def test_zlib_full_flush_with_name_and_mtime(gpu_ctx, plain, full_member, piece_mode):
    pieces, tail, _ = full_member
    header = b"\x1f\x8b\x08\x08" + struct.pack("<I", 1_700_000_000) + b"\x00\x03" + b"pieces.txt\x00"
    r = la_api.cat(member(b"".join(pieces) + tail, plain, header))
    assert la_api.as_reference_tuple(r) == (plain, 0, "")
    assert (r.pathname, r.mtime) == ("pieces.txt", 1_700_000_000)


def test_false_marker_in_stored_data_merges_the_pieces(gpu_ctx, piece_mode):
    a, b = word_text(200_000, 4), word_text(100_000, 5)
    noise = random.Random(6).randbytes(9000)
    stored = noise[:4000] + MARKER + noise[4000:8000] + MARKER + MARKER + noise[8000:]      # level 0: stored blocks
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(a[i:i + STEP]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(a), STEP))
    c0 = zlib.compressobj(0, zlib.DEFLATED, -15)
    mid = c0.compress(stored) + c0.flush(zlib.Z_FULL_FLUSH)
    assert mid.count(MARKER) == 4
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15)
    end = b"".join(c2.compress(b[i:i + STEP]) + c2.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(b), STEP)) + c2.flush()
    whole = a + stored + b
    assert zlib.decompress(body + mid + end, -15) == whole
    assert cat(member(body + mid + end, whole)) == (whole, 0, "")


def test_sync_flush_stream_falls_back(gpu_ctx, piece_mode):
    plain = word_text(900_000, 7)
    pieces, tail = flushed_body(plain, zlib.Z_SYNC_FLUSH)
    img = member(b"".join(pieces) + tail, plain)
    piece_mode.delenv("LA_GZIP_FLUSH_POINTS")
    today = cat(img)
    piece_mode.setenv("LA_GZIP_FLUSH_POINTS", "1")
    assert cat(img) == today == (plain, 0, "")


def test_member_that_turns_dependent_is_refused_by_name(gpu_ctx, piece_mode):
    """three windows and more of independent pieces, then pieces that need the output in front of them"""
    head = random.Random(8).randbytes(3_400_000)        # stored: 1 MiB of compressed bytes is about 1 MiB of these
    dep = word_text(400_000, 9)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(head[i:i + STEP]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(head), STEP))
    body += b"".join(c.compress(dep[i:i + STEP]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(dep), STEP)) + c.flush()
    whole = head + dep
    assert zlib.decompress(body, -15) == whole
    data, rc, msg = cat(member(body, whole))
    assert rc == la_api.ARCHIVE_FATAL and "blocks behind a flush point depend on earlier output" in msg
    # whole 64 KiB blocks of what stood in front of the first dependent piece (the first of them decodes alone), never a
    # wrong byte
    assert len(data) % 65536 == 0 and whole.startswith(data)
    assert len(head) - 65536 < len(data) <= len(head) + STEP


def test_damage_cut_and_trailer(gpu_ctx, plain, full_member, piece_mode):
    pieces, tail, img = full_member
    off5 = 10 + sum(len(p) for p in pieces[:5])
    # a bit flipped in piece 5: the model's byte count, the reference's message
    for at in (off5 + 7, off5 + len(pieces[5]) // 2):
        bad = bytearray(img)
        bad[at] ^= 0x10
        ref, res = O.gzip_stream_decode(bytes(bad), len(plain) + 65536)
        got = cat(bytes(bad))
        if res.rc == 0:     # (a flipped literal: only the CRC notices, and the reference does not look)
            assert got[1:] == (0, "") and len(got[0]) == len(plain)
        else:
            assert res.errmsg.decode() == "gzip decompression failed"
            assert got == (ref.tobytes(), la_api.ARCHIVE_FATAL, "gzip decompression failed"), (at, len(got[0]), got[1:], len(ref))
    # a cut inside piece 5
    cut = img[:off5 + len(pieces[5]) // 2]
    ref, res = O.gzip_stream_decode(cut, len(plain) + 65536)
    assert (res.rc, res.errmsg.decode()) == (la_api.ARCHIVE_FATAL, "truncated gzip input")
    assert cat(cut) == (ref.tobytes(), la_api.ARCHIVE_FATAL, "truncated gzip input")
    # a wrong CRC32 / ISIZE: accepted as the reference accepts it, refused under LA_GZIP_STRICT=1
    for k, text in ((-8, "gzip member CRC32 mismatch"), (-4, "gzip member ISIZE mismatch")):
        bad = bytearray(img)
        bad[k] ^= 1
        piece_mode.delenv("LA_GZIP_STRICT", raising=False)
        assert cat(bytes(bad)) == (plain, 0, "")
        piece_mode.setenv("LA_GZIP_STRICT", "1")
        data, rc, msg = cat(bytes(bad))
        assert (rc, msg) == (la_api.ARCHIVE_FATAL, text) and plain.startswith(data)
    assert cat(img) == (plain, 0, "")
    piece_mode.delenv("LA_GZIP_STRICT")


def test_what_follows_the_trailer(gpu_ctx, plain, full_member, piece_mode):
    pieces, tail, img = full_member
    second_plain = word_text(50_000, 10)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    second = co.compress(second_plain) + co.flush()
    assert cat(img + second) == (plain + second_plain, 0, "")
    assert cat(img + b"not a gzip header at all" * 3) == (plain, 0, "")
    assert cat(img + img) == (plain + plain, 0, "")
