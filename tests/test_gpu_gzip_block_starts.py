"""One raw-deflate span with no flush point through la_gpu_gzip_decode with LA_GZ_OPT_PIECES | LA_GZ_OPT_CHAIN |
LA_GZ_OPT_BLOCK_STARTS (include/la_gpu.h): the device finds the candidate block starts itself, decodes a piece from each,
confirms those a confirmed piece ended on, and decodes the confirmed pieces as a chain.

The referee is the machine's zlib: inflate for the bytes and verdicts (tests/deflate_support.py), inflate(Z_BLOCK) for the
true block starts (tests/deflate_find_support.py).  How many pieces must be confirmed follows from those starts: the
caller's own start is piece 0, and every non-final dynamic block that starts behind it begins a piece -- were one of them
missing from the candidate table, two pieces would have merged and the count would be lower.  (A stream of N non-final
dynamic blocks and a final one, the first block at the caller's start, has N pieces: the first block is piece 0 itself.)

The source is [3 bytes of junk][the span][8 trailer bytes and junk]; src_bytes covers all of it, the span only its own
bytes.  The destination is prefilled with a guard byte; nothing outside [history, packed bytes] may change."""
import random
import zlib

import numpy as np
import pytest

import deflate_build as B
import deflate_find_support as F
import deflate_support as DS

pytestmark = pytest.mark.gpu

OPT_WAVE, OPT_LANE, OPT_TWO_PHASE, OPT_RAW, OPT_PIECES, OPT_CHAIN, OPT_BLOCK_STARTS = 2, 4, 8, 16, 64, 128, 256
ST_OK, ST_DATA, ST_TRUNC, ST_FULL, ST_PIECE_END = 0, 5, 6, 9, 18
LA_ERR_ARG = -3
JUNK_FRONT = b"\x5a\x84\x01"
JUNK_BEHIND = bytes([0x04, 0x80, 0x1d, 0xc7]) * 16       # (reads as headers of non-final dynamic blocks here and there)


def run(gpu_ctx, body, dst_cap, start_bit=0, hist=b"", first_byte=0, **kw):
    """the span is body[first_byte:], its true boundary at bit start_bit of its first byte"""
    import torch
    from libarchive_amd import gzip as G
    src = JUNK_FRONT + bytes(body) + JUNK_BEHIND
    d_src = torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).cuda()
    r = G.decode_block_starts(gpu_ctx, d_src, len(JUNK_FRONT) + first_byte, len(body) - first_byte, dst_cap, start_bit, hist, **kw)
    if r is None:
        return None
    dst = r.out.cpu().numpy()
    assert (dst[:r.lead - len(hist)] == r.guard).all(), "bytes in front of the history changed"
    assert dst[r.lead - len(hist):r.lead].tobytes() == hist, "the history changed"
    assert r.out_len <= dst_cap
    assert (dst[r.lead + dst_cap:] == r.guard).all(), "bytes behind dst_cap changed"
    r.bytes = dst[r.lead:r.lead + r.out_len].tobytes()
    return r


def check(r, want, status, pieces=None):
    print("status %d out_len %d consumed_bits %d candidates %d pieces %d" % (r.status, r.out_len, r.consumed_bits, r.candidates, r.pieces))
    assert r.status == status, (r.status, status)
    assert r.out_len == len(want), (r.out_len, len(want))
    if r.bytes != want:
        bad = next(i for i in range(len(want)) if r.bytes[i] != want[i])
        raise AssertionError("first wrong byte at %d of %d" % (bad, len(want)))
    assert r.crc32 == zlib.crc32(want) & 0xFFFFFFFF
    if status in (ST_OK, ST_PIECE_END, ST_FULL):
        assert r.boundary == (r.status, r.out_len, r.consumed_bits, r.crc32)
    else:
        st, n, bits, crc = r.boundary
        assert st == ST_PIECE_END and n <= r.out_len and crc == zlib.crc32(want[:n]) & 0xFFFFFFFF, r.boundary
    if pieces is not None:
        assert r.pieces == pieces, (r.pieces, pieces)
        assert r.candidates >= pieces - 1


@pytest.fixture(scope="module")
def text():
    return F.word_text(3 << 19, seed=5)          # 1.5 MiB


@pytest.mark.parametrize("level", [6, 9])
def test_text_body_every_true_start_confirmed(gpu_ctx, text, level):
    body = F.raw_deflate(text, level)
    true = F.true_candidates(body)
    assert len(true) >= 10, "the stream holds too few blocks to show anything"
    r = run(gpu_ctx, body + zlib.crc32(text).to_bytes(4, "little") + len(text).to_bytes(4, "little"), len(text))
    check(r, text, ST_OK, pieces=1 + len(true))
    assert (r.consumed_bits + 7) // 8 == len(body)


@pytest.mark.parametrize("how", ["level1", "fixed"])
def test_few_or_no_dynamic_blocks(gpu_ctx, text, how):
    plain = text[:400001]
    body = F.raw_deflate(plain, 1) if how == "level1" else F.raw_deflate(plain, 6, zlib.Z_FIXED)
    true = F.true_candidates(body)
    if how == "fixed":
        assert not true and all(typ == 1 for _, _, typ in F.block_starts(body))
    r = run(gpu_ctx, body, len(plain) + 7)
    check(r, plain, ST_OK, pieces=1 + len(true))


@pytest.mark.parametrize("phase", range(8))
def test_second_block_at_every_bit_of_its_byte(gpu_ctx, phase):
    image, plain, info = F.second_block_at(phase)
    trailer = zlib.crc32(plain).to_bytes(4, "little") + len(plain).to_bytes(4, "little")
    r = run(gpu_ctx, image + trailer, len(plain))
    check(r, plain, ST_OK, pieces=2)          # (the third block is final: it belongs to the second piece)
    # the final block ends where the builder says, in mid-byte or not, and the trailer behind it is not read as deflate
    assert r.consumed_bits == info["bits"]
    # the same stream entered at its second block: a start bit, and the first block's output as history
    at = info["block_bits"][1]
    first_len = next(o for bits, o in reversed(info["marks"]) if bits <= at)
    r = run(gpu_ctx, image + trailer, len(plain) - first_len, start_bit=at % 8, hist=plain[:first_len], first_byte=at // 8)
    check(r, plain[first_len:], ST_OK, pieces=1)
    assert r.consumed_bits == info["bits"] - 8 * (at // 8)


def test_some_final_block_ends_in_mid_byte():
    assert any(F.second_block_at(p)[2]["bits"] % 8 for p in range(8))


def test_match_from_the_first_symbol_into_the_piece_before(gpu_ctx):
    image, plain, info, base = F.far_match_stream()
    r = run(gpu_ctx, image, len(plain))
    check(r, plain, ST_OK, pieces=2)


def test_match_into_the_history_and_one_byte_beyond(gpu_ctx):
    image, plain, info, base = F.far_match_stream()
    at = info["block_bits"][1]
    r = run(gpu_ctx, image, len(plain) - 32768, start_bit=at % 8, hist=base, first_byte=at // 8)
    check(r, plain[32768:], ST_OK, pieces=1)
    r = run(gpu_ctx, image, len(plain) - 32768, start_bit=at % 8, hist=base[1:], first_byte=at // 8)
    check(r, b"", ST_DATA, pieces=1)
    verdict, _, out, msg = DS.zlib_inflate(image[at // 8:])      # (zlib without the history: the same verdict)
    assert at % 8 == 0 and verdict == "data" and out == b"" and "too far back" in msg


def test_adversarial_a_deflate_body_inside_stored_blocks(gpu_ctx):
    """every block start of the inner stream is a perfect candidate and every one is false: the outer stream is stored
    blocks, one piece, and its output is the inner stream's BYTES"""
    inner = F.raw_deflate(F.word_text(300000, seed=9), 6)
    outer = F.raw_deflate(inner, 0)
    assert all(typ == 0 for _, _, typ in F.block_starts(outer))
    held = F.model_candidates(outer)
    assert len(held) >= 2, "precondition: the input holds no false candidates"
    r = run(gpu_ctx, outer, len(inner))
    check(r, inner, ST_OK, pieces=1)
    assert r.candidates == len(held) and r.candidates > r.pieces


def test_noise_stored_blocks_only(gpu_ctx):
    noise = random.Random(77).randbytes(262144)
    body = F.raw_deflate(noise, 6)
    assert all(typ == 0 for _, _, typ in F.block_starts(body))
    r = run(gpu_ctx, body, len(noise))
    check(r, noise, ST_OK, pieces=1)


@pytest.fixture(scope="module")
def small():
    plain = F.word_text(600000, seed=21)
    body = F.raw_deflate(plain, 6)
    starts = F.block_starts(body)
    assert len(starts) >= 4 and all(typ == 2 for _, _, typ in starts)
    return plain, body, [p for p, _, _ in starts]


@pytest.mark.parametrize("where", ["inside-a-header", "inside-a-block", "after-a-block"])
def test_cut_body(gpu_ctx, small, where):
    plain, body, starts = small
    assert starts[2] % 8 != 0 or starts[3] % 8 != 0
    after = starts[2] if starts[2] % 8 else starts[3]
    cut = {"inside-a-header": starts[2] // 8 + 6, "inside-a-block": (starts[2] + starts[3]) // 16, "after-a-block": (after + 7) // 8}[where]
    verdict, _, want, _ = DS.zlib_inflate(body[:cut])
    assert verdict == "more" and want == plain[:len(want)] and len(want) > 0
    r = run(gpu_ctx, body[:cut], len(plain))
    check(r, want, ST_TRUNC)
    # where a caller with more input goes on from: the last block start whose header the cut left whole, and the bytes
    # zlib has produced when it stands there
    last = max(p for p in starts if F.is_candidate(body[:cut], p))
    _, _, upto, _ = DS.zlib_inflate(body[:(last + 7) // 8])
    assert r.boundary[1:3] == (len(upto), last), (r.boundary, len(upto), last)


def test_flipped_bit_in_the_third_block(gpu_ctx, small):
    import test_gpu_deflate_handbuilt as H
    plain, body, starts = small
    # the first bit behind the third block's type bits on whose flip zlib refuses the stream (a precondition: a flip that
    # only changes a literal shows nothing; in the header most flips do)
    for at in range(starts[2] + 3, starts[3]):
        bad = bytearray(body)
        bad[at // 8] ^= 1 << (at % 8)
        if DS.zlib_inflate(bytes(bad))[0] == "data":
            break
    else:
        raise AssertionError("no flip in the third block makes zlib refuse the stream")
    (st, out, _, _), = H.run_table(gpu_ctx, [(bytes(bad), len(plain))], OPT_WAVE | OPT_RAW)
    print("the wave kernel: status %d out_len %d" % (st, len(out)))
    r = run(gpu_ctx, bytes(bad), len(plain))
    assert st != ST_FULL
    check(r, out, st)


def test_dst_cap_one_byte_short(gpu_ctx, small):
    """the piece that does not fit is not delivered: the pieces in front of it are, and consumed names where it starts"""
    plain, body, starts = small
    r = run(gpu_ctx, body, len(plain) - 1)
    print("status %d out_len %d consumed_bits %d pieces %d" % (r.status, r.out_len, r.consumed_bits, r.pieces))
    assert r.status == ST_FULL
    # (the last piece starts at the last NON-FINAL block and holds the final block too)
    assert r.consumed_bits == starts[-2] and r.pieces == len(starts) - 2
    assert r.bytes == plain[:r.out_len] and r.crc32 == zlib.crc32(r.bytes) & 0xFFFFFFFF and 0 < r.out_len < len(plain)
    # ... and from there the rest decodes, with the last 32 KiB as history
    at = r.consumed_bits
    r2 = run(gpu_ctx, body, len(plain) - r.out_len, start_bit=at % 8, hist=plain[r.out_len - 32768:r.out_len], first_byte=at // 8)
    check(r2, plain[r.out_len:], ST_OK, pieces=1)


def test_option_is_refused_where_it_does_not_apply(gpu_ctx, small):
    plain, body, _ = small
    full = OPT_PIECES | OPT_CHAIN | OPT_BLOCK_STARTS
    for options in (OPT_BLOCK_STARTS, OPT_BLOCK_STARTS | OPT_PIECES, OPT_BLOCK_STARTS | OPT_CHAIN, full | OPT_LANE, full | OPT_TWO_PHASE):
        assert run(gpu_ctx, body, len(plain), options=options, expect_rc=LA_ERR_ARG) is None
    assert run(gpu_ctx, body, len(plain), src_bytes=1 << 29, expect_rc=LA_ERR_ARG) is None
    assert run(gpu_ctx, body, len(plain), hist=bytes(32769), lead=32768 + 128, expect_rc=LA_ERR_ARG) is None


def test_existing_instances_answer_as_before_with_the_option_clear(gpu_ctx):
    """the wave kernel's other instances (members, pieces) on the hand-built catalogue, whose expected bytes and statuses are
    the builder's model of zlib: option bit 256 clear, nothing of the new path is entered"""
    import test_gpu_deflate_handbuilt as H
    cases = B.handbuilt_cases()
    entries = [(c.image, len(c.plain) if c.valid else H.REFUSED_CAP) for c in cases]
    got = H.run_table(gpu_ctx, entries, OPT_WAVE | OPT_RAW)
    for c, (st, out, _, crc) in zip(cases, got):
        assert (st, out) == (c.status, c.plain), c.name
        if c.valid:
            assert crc == zlib.crc32(c.plain) & 0xFFFFFFFF, c.name
    # as pieces: a valid stream still ends LA_ST_OK with the same bytes (a piece ends like a member at a final block)
    got = H.run_table(gpu_ctx, entries, OPT_WAVE | OPT_PIECES)
    for c, (st, out, _, _) in zip(cases, got):
        if c.valid:
            assert (st, out) == (ST_OK, c.plain), c.name
