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


# ---- branches of the piece walk that the streams above do not reach: slot growth, the slot and span limits, a member
# whose flush points stop, and a window of pieces right behind a window of members that asked for a retry ----

TOO_LARGE = "gzip member too large for the GPU data plane (4 GiB limit)"
GROW_SPANS = (100_000, 100_000, 100_000, 400_000, 400_000, 400_000, 400_000)


def run_stream(flush):
    """runs of one byte value between flush points: 400 000 of them are a few hundred compressed bytes, so the first
    slot of such a piece (64 KiB) is too small three times over"""
    plain = b"".join(bytes([65 + k]) * n for k, n in enumerate(GROW_SPANS))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces, at = [], 0
    for n in GROW_SPANS:
        pieces.append(c.compress(plain[at:at + n]) + c.flush(flush))
        at += n
    assert max(len(p) for p in pieces) < 1000
    return plain, member(b"".join(pieces) + c.flush(), plain)


def test_slots_grow_until_the_piece_fits(gpu_ctx, piece_mode):
    plain, img = run_stream(zlib.Z_FULL_FLUSH)
    assert zlib.decompress(img, 31) == plain
    assert cat(img) == (plain, 0, "")
    assert cat(img, read_size=4099) == (plain, 0, "")


def test_slot_limit_refuses_the_piece_that_cannot_fit(gpu_ctx, piece_mode):
    plain, img = run_stream(zlib.Z_FULL_FLUSH)
    piece_mode.setenv("LA_GZ_TEST_SLOT_LIMIT", "262144")
    # the ordinary path's message for the same limit (a member whose ISIZE claims too little)
    piece_mode.delenv("LA_GZIP_FLUSH_POINTS")
    fat = bytes(range(256)) * 4096
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    liar = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + c.compress(fat) + c.flush() + struct.pack("<II", zlib.crc32(fat), 10)
    ordinary = cat(liar)
    assert ordinary[1:] == (la_api.ARCHIVE_FATAL, TOO_LARGE)
    piece_mode.setenv("LA_GZIP_FLUSH_POINTS", "1")
    # the three pieces of 100 000 fit into 128 KiB; the fourth needs 400 000: whole 64 KiB blocks of the 300 000 in front
    k = 300_000 // 65536
    assert cat(img) == (plain[:k * 65536], la_api.ARCHIVE_FATAL, ordinary[2])


def test_span_limit_refuses_the_piece_that_is_too_long(gpu_ctx, piece_mode):
    rnd = random.Random(21)
    small, large = rnd.randbytes(200_000), rnd.randbytes(300_000)      # stored: a piece is as long as its step
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(small[i:i + 10_000]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(small), 10_000))
    body += b"".join(c.compress(large[i:i + STEP]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(large), STEP)) + c.flush()
    whole = small + large
    assert zlib.decompress(body, -15) == whole
    piece_mode.setenv("LA_GZ_TEST_SPAN_LIMIT", "20000")
    data, rc, msg = cat(member(body, whole))
    assert (rc, msg) == (la_api.ARCHIVE_FATAL, TOO_LARGE)
    # whole 64 KiB blocks of what stands in front of the first piece of 30 000
    assert data == whole[:(len(small) // 65536) * 65536]
    piece_mode.delenv("LA_GZ_TEST_SPAN_LIMIT")
    assert cat(member(body, whole)) == (whole, 0, "")


def no_flush_point_member(flush):
    """flush points for two windows of 1 MiB and more, then 2.5 MiB without one"""
    rnd = random.Random(22)
    head = rnd.randbytes(2_300_000)
    tail = rnd.randbytes(2_700_000).replace(b"\xff\xff", b"\xff\xfe")      # (no accidental 00 00 FF FF in the stored bytes)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(head[i:i + STEP]) + c.flush(flush) for i in range(0, len(head), STEP))
    rest = c.compress(tail) + c.flush()
    assert len(body) > 2 << 20 and len(rest) > 5 << 19 and MARKER not in rest
    return head, member(body + rest, head + tail)


def test_no_flush_point_within_the_widest_window(gpu_ctx, piece_mode):
    head, img = no_flush_point_member(zlib.Z_FULL_FLUSH)
    piece_mode.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    data, rc, msg = cat(img)
    assert rc == la_api.ARCHIVE_FATAL and "no flush point within LA_GPU_MAX_BATCH_MIB" in msg
    assert len(data) % 65536 == 0 and head.startswith(data) and len(head) - 65536 < len(data)


def members_with_a_planted_header(seed):
    """two members of stored data, 600 000 bytes each and free of 00 00 FF FF, so that the first 1 MiB window is walked as
    members; the second holds what looks like a member header, the boundary guess the decode refutes"""
    rnd = random.Random(seed)
    clean = lambda b: b.replace(b"\xff\xff", b"\xff\xfe").replace(b"\x1f\x8b", b"\x1f\x8c").replace(b"\x00", b"\x01")
    one = clean(rnd.randbytes(600_000))
    two = clean(rnd.randbytes(250_000)) + b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + clean(rnd.randbytes(350_000))
    img = b""
    for d in (one, two):
        co = zlib.compressobj(1, zlib.DEFLATED, 31)     # (random bytes: stored blocks, the last of them not an empty one)
        img += co.compress(d) + co.flush()
    assert MARKER not in img
    return one + two, img


def test_pieces_right_behind_members_that_asked_for_a_retry(gpu_ctx, plain, full_member, piece_mode):
    front_plain, front = members_with_a_planted_header(23)
    want, res = O.gzip_stream_decode(front + full_member[2], len(front_plain) + len(plain) + 65536)
    assert (want.tobytes(), res.rc) == (front_plain + plain, 0)
    assert cat(front + full_member[2]) == (front_plain + plain, 0, "")
    assert cat(front + full_member[2], read_size=70001) == (front_plain + plain, 0, "")
