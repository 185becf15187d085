"""The gzip read filter with LA_GZIP_FLUSH_POINTS=chain: ONE member whose pieces depend on each other (zlib's
Z_SYNC_FLUSH, pigz without -i) decoded from its flush points with LA_GZ_OPT_CHAIN, the last 32 KiB of the member's output
carried from window to window (la_filter_gzip.c).  Through la_api.cat (= bsdcat) with 1 MiB windows.

Expected bytes are the plain input (zlib wrote and checked every stream); expected byte counts in front of an error are
the CPU filter model's (oracle/orc_filters.c through oracle_lib.gzip_stream_decode) for the same damaged stream."""
import random
import struct
import zlib

import pytest

import la_api
import oracle_lib as O

pytestmark = pytest.mark.gpu

MARKER = b"\x00\x00\xff\xff"
WORDS = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave", b"boundary", b"history"]
STEP = 30000
HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def word_text(n, seed):
    r = random.Random(seed)
    return b" ".join(r.choice(WORDS) for _ in range(n // 4))[:n]


def trailer(plain):
    return struct.pack("<II", zlib.crc32(plain) & 0xFFFFFFFF, len(plain) & 0xFFFFFFFF)


def member(body, plain, header=HEADER):
    return header + body + trailer(plain)


@pytest.fixture(scope="module")
def plain():
    # text, random bytes (stored blocks), zeros, text again: the random part does not shrink, so the member is about
    # 3.5 MiB of compressed bytes, more than three 1 MiB windows
    a = word_text(500_000, 1)
    return a + random.Random(2).randbytes(3_600_000) + bytes(100_000) + a[:200_000]


@pytest.fixture(scope="module")
def sync_member(plain):
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    pieces = [c.compress(plain[i:i + STEP]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(plain), STEP)]
    tail = c.flush()
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        zlib.decompressobj(-15).decompress(pieces[1])
    img = member(b"".join(pieces) + tail, plain)
    assert len(img) > (3 << 20) + 300_000 and zlib.decompress(img, 31) == plain
    return pieces, tail, img


@pytest.fixture()
def chain_mode(monkeypatch):
    monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", "chain")
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    return monkeypatch


def cat(img, **kw):
    return la_api.as_reference_tuple(la_api.cat(img, **kw))


def test_sync_flush_member_with_name_and_mtime_across_windows(gpu_ctx, plain, sync_member, chain_mode):
    pieces, tail, _ = sync_member
    header = b"\x1f\x8b\x08\x08" + struct.pack("<I", 1_700_000_000) + b"\x00\x03" + b"chain.txt\x00"
    img = member(b"".join(pieces) + tail, plain, header)
    r = la_api.cat(img)
    assert la_api.as_reference_tuple(r) == (plain, 0, "")
    assert (r.pathname, r.mtime) == ("chain.txt", 1_700_000_000)
    assert cat(img, read_size=4099) == (plain, 0, "")
    # the default policy bids for it on its flush points
    chain_mode.setenv("LA_GPU_BID", "auto")
    r = la_api.cat(img)
    assert 1 in [c for c, _ in r.filters] and r.data == plain


def test_member_that_turns_dependent(gpu_ctx, chain_mode):
    """the stream of test_gpu_filter_flush_points.test_member_that_turns_dependent_is_refused_by_name: three windows and
    more of independent pieces, then pieces that need the output in front of them"""
    head = random.Random(8).randbytes(3_400_000)
    dep = word_text(400_000, 9)
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    body = b"".join(c.compress(head[i:i + STEP]) + c.flush(zlib.Z_FULL_FLUSH) for i in range(0, len(head), STEP))
    body += b"".join(c.compress(dep[i:i + STEP]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(dep), STEP)) + c.flush()
    whole = head + dep
    assert zlib.decompress(body, -15) == whole
    img = member(body, whole)
    assert cat(img) == (whole, 0, "")
    chain_mode.setenv("LA_GZIP_FLUSH_POINTS", "1")
    data, rc, msg = cat(img)
    assert rc == la_api.ARCHIVE_FATAL and "blocks behind a flush point depend on earlier output" in msg
    assert len(data) % 65536 == 0 and whole.startswith(data)


def test_damage_in_the_fourth_window(gpu_ctx, plain, sync_member, chain_mode):
    pieces, tail, img = sync_member
    # a piece that starts more than 3 MiB into the compressed stream, i.e. in the fourth 1 MiB window
    k, off = 0, len(HEADER)
    while off < (3 << 20) + 50_000:
        off += len(pieces[k])
        k += 1
    assert k < len(pieces) - 1
    seen_error = False
    for at in (off + 7, off + len(pieces[k]) // 2):
        bad = bytearray(img)
        bad[at] ^= 0x10
        ref, res = O.gzip_stream_decode(bytes(bad), len(plain) + 65536)
        got = cat(bytes(bad))
        if res.rc == 0:     # (a flipped literal or stored byte: only the CRC notices, and the reference does not look)
            assert got[1:] == (0, "") and len(got[0]) == len(plain)
        else:
            seen_error = True
            assert res.errmsg.decode() == "gzip decompression failed"
            assert len(ref) % 65536 == 0
            assert got == (ref.tobytes(), la_api.ARCHIVE_FATAL, "gzip decompression failed"), (at, len(got[0]), got[1:], len(ref))
    # a header byte of a stored block (LEN against NLEN) is damage whatever the data: the piece starts with one where the
    # input is random bytes
    bad = bytearray(img)
    bad[off + 1] ^= 0x01
    ref, res = O.gzip_stream_decode(bytes(bad), len(plain) + 65536)
    if res.rc != 0:
        seen_error = True
        assert cat(bytes(bad)) == (ref.tobytes(), la_api.ARCHIVE_FATAL, res.errmsg.decode())
    assert seen_error


def test_cut_behind_a_flush_point(gpu_ctx, plain, sync_member, chain_mode):
    pieces, tail, img = sync_member
    n = len(pieces) - 3
    cut = img[:len(HEADER) + sum(len(p) for p in pieces[:n])]
    assert cut.endswith(MARKER)
    ref, res = O.gzip_stream_decode(cut, len(plain) + 65536)
    assert (res.rc, res.errmsg.decode()) == (la_api.ARCHIVE_FATAL, "truncated gzip input")
    assert cat(cut) == (ref.tobytes(), la_api.ARCHIVE_FATAL, "truncated gzip input")


def test_trailer_mismatch(gpu_ctx, plain, sync_member, chain_mode):
    pieces, tail, img = sync_member
    for k, text in ((-8, "gzip member CRC32 mismatch"), (-4, "gzip member ISIZE mismatch")):
        bad = bytearray(img)
        bad[k] ^= 1
        chain_mode.delenv("LA_GZIP_STRICT", raising=False)
        assert cat(bytes(bad)) == (plain, 0, "")
        chain_mode.setenv("LA_GZIP_STRICT", "1")
        data, rc, msg = cat(bytes(bad))
        assert (rc, msg) == (la_api.ARCHIVE_FATAL, text) and plain.startswith(data)
    assert cat(img) == (plain, 0, "")
    chain_mode.delenv("LA_GZIP_STRICT")


def test_second_member_behind_the_trailer(gpu_ctx, plain, sync_member, chain_mode):
    pieces, tail, img = sync_member
    second_plain = word_text(50_000, 10)
    co = zlib.compressobj(6, zlib.DEFLATED, 31)
    second = co.compress(second_plain) + co.flush()
    assert cat(img + second) == (plain + second_plain, 0, "")
    assert cat(img + img) == (plain + plain, 0, "")


# ---- slot growth and the slot limit under chain, a member whose flush points stop, and a window of pieces right behind
# a window of members that asked for a retry: the streams of tests/test_gpu_filter_flush_points.py, written with
# Z_SYNC_FLUSH where the test is about the pieces ----

import test_gpu_filter_flush_points as F


def test_slots_grow_until_the_piece_fits(gpu_ctx, chain_mode):
    grow, img = F.run_stream(zlib.Z_SYNC_FLUSH)
    assert zlib.decompress(img, 31) == grow
    assert cat(img) == (grow, 0, "")
    assert cat(img, read_size=4099) == (grow, 0, "")


def test_slot_limit_refuses_the_piece_that_cannot_fit(gpu_ctx, chain_mode):
    grow, img = F.run_stream(zlib.Z_SYNC_FLUSH)
    chain_mode.setenv("LA_GZ_TEST_SLOT_LIMIT", "262144")
    assert cat(img) == (grow[:(300_000 // 65536) * 65536], la_api.ARCHIVE_FATAL, F.TOO_LARGE)


def test_no_flush_point_within_the_widest_window(gpu_ctx, chain_mode):
    head, img = F.no_flush_point_member(zlib.Z_SYNC_FLUSH)
    chain_mode.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    data, rc, msg = cat(img)
    assert rc == la_api.ARCHIVE_FATAL and "no flush point within LA_GPU_MAX_BATCH_MIB" in msg
    assert len(data) % 65536 == 0 and head.startswith(data) and len(head) - 65536 < len(data)


def test_pieces_right_behind_members_that_asked_for_a_retry(gpu_ctx, plain, sync_member, chain_mode):
    front_plain, front = F.members_with_a_planted_header(24)
    want, res = O.gzip_stream_decode(front + sync_member[2], len(front_plain) + len(plain) + 65536)
    assert (want.tobytes(), res.rc) == (front_plain + plain, 0)
    assert cat(front + sync_member[2]) == (front_plain + plain, 0, "")
