"""GPU parity for the match phase of the LDS-window expand kernel: hand-built blocks whose matches wait on each other
in long chains, with every copy class (16 bytes and more, 8..15, 4..7, 1..3, overlapping with periods 1..15), sources
that straddle the 32-sequence flag words, blocks of more than 4096 sequences (the segmented form) and deflate
members with 3-byte matches 32 KiB back.  Every output is compared with the oracle and with the bytes the
generator meant."""
import random
import struct
import zlib

import pytest

import oracle_lib as O
import streams as S
from test_gpu_lz4 import gpu_decode
from test_gpu_gzip import ST_OK, _dynamic_block, gpu_inflate, trailer

pytestmark = pytest.mark.gpu


def _lz4_varlen(n):
    return b"\xff" * (n // 255) + bytes([n % 255])


def lz4_block_from_sequences(seqs, tail):
    """seqs: (literal bytes, offset, match length >= 4); tail: the literals of the last sequence (>= 5 bytes, so the
    block ends as LZ4 requires).  Returns (encoded block, decoded bytes)."""
    enc, out = bytearray(), bytearray()
    for lit, off, mlen in seqs:
        assert 1 <= off <= len(out) + len(lit) and mlen >= 4
        ll, ml = len(lit), mlen - 4
        enc.append((min(ll, 15) << 4) | min(ml, 15))
        if ll >= 15:
            enc += _lz4_varlen(ll - 15)
        enc += lit
        enc += struct.pack("<H", off)
        if ml >= 15:
            enc += _lz4_varlen(ml - 15)
        out += lit
        for _ in range(mlen):
            out.append(out[-off])
    ll = len(tail)
    enc.append(min(ll, 15) << 4)
    if ll >= 15:
        enc += _lz4_varlen(ll - 15)
    enc += tail
    out += tail
    return bytes(enc), bytes(out)


def _check_blocks(ctx, blocks):
    """blocks: list of (encoded, decoded), at most 64 KiB decoded each; one frame, block checksums on."""
    img, plain = S.lz4_frame([(p, S.lz4_block(e, bsum=True)) for e, p in blocks], flg=0x74)
    out, rc, msg = gpu_decode(ctx, img)
    ref, res = O.lz4_stream_decode(img, len(plain) + 16)
    assert (rc, msg) == (0, "") and res.rc == 0
    assert out == plain == ref.tobytes()


def _chain(rnd, nseq, lo, hi):
    """every match starts its source at the start of the previous match (its length drawn from lo..hi): each one
    waits for the one before, a dependency chain nseq deep; a match longer than the previous one overlaps itself"""
    seqs, prev = [], None
    for i in range(nseq):
        lit = rnd.randbytes(1)
        mlen = rnd.randint(lo, hi)
        off = (prev + 1) if prev is not None else 1
        seqs.append((lit, off, mlen))
        prev = mlen
    return seqs


def test_chain_through_every_match(gpu_ctx):
    rnd = random.Random(0xDC01)
    blocks = []
    for lo, hi in ((4, 7), (8, 15), (16, 47), (4, 60), (48, 90)):
        nseq = 2000 if hi <= 15 else min(2000, 60000 // (hi + 1))
        blocks.append(lz4_block_from_sequences(_chain(rnd, nseq, lo, hi), rnd.randbytes(8)))
    _check_blocks(gpu_ctx, blocks)


def test_short_and_long_periods_side_by_side(gpu_ctx):
    """overlapping matches with periods 1..7 and 8..15 next to each other, and next to matches that do not overlap"""
    rnd = random.Random(0xDC02)
    blocks = []
    for _ in range(4):
        seqs, n = [], 0
        while n < 60000:
            lit = rnd.randbytes(rnd.randint(0, 20))
            n += len(lit)
            kind = rnd.randrange(3)
            if kind == 0:
                off, mlen = rnd.randint(1, 7), rnd.randint(4, 80)
            elif kind == 1:
                off, mlen = rnd.randint(8, 15), rnd.randint(16, 120)
            else:
                off, mlen = rnd.randint(16, 2000), rnd.randint(4, 48)
            off = min(off, n)
            if off == 0:
                lit, n = rnd.randbytes(1), n + 1
                off = 1
            seqs.append((lit, off, mlen))
            n += mlen
        blocks.append(lz4_block_from_sequences(seqs, rnd.randbytes(6)))
    _check_blocks(gpu_ctx, blocks)


def test_sources_across_flag_words(gpu_ctx):
    """short sequences (so 32 of them span about 250 bytes) whose sources reach back over several of them: the
    sequences a match waits for lie on both sides of a 32-sequence flag word, often in the literal part"""
    rnd = random.Random(0xDC03)
    blocks = []
    for _ in range(4):
        seqs, n = [], 0
        while n < 30000:
            lit = rnd.randbytes(rnd.randint(1, 4))
            n += len(lit)
            mlen = rnd.randint(4, 12)
            off = rnd.randint(1, min(n, 400))
            seqs.append((lit, off, mlen))
            n += mlen
        blocks.append(lz4_block_from_sequences(seqs, rnd.randbytes(5)))
    _check_blocks(gpu_ctx, blocks)


def test_more_than_4096_sequences(gpu_ctx):
    """64 KiB blocks of 6000 to 9000 sequences: the segmented form of the kernel, with chains across segments"""
    rnd = random.Random(0xDC04)
    blocks = []
    for nseq, lo, hi in ((6000, 4, 8), (9000, 4, 5)):
        seqs = _chain(rnd, nseq // 2, lo, hi)
        n = sum(len(l) + m for l, _, m in seqs)
        while len(seqs) < nseq and n < 65000:
            lit = rnd.randbytes(rnd.randint(0, 2))
            n += len(lit)
            mlen = rnd.randint(4, 6)
            off = rnd.randint(1, min(n, 9000))
            seqs.append((lit, off, mlen))
            n += mlen
        enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(5))
        assert len(plain) <= 65536 and len(seqs) > 4096
        blocks.append((enc, plain))
    _check_blocks(gpu_ctx, blocks)


def test_deflate_three_byte_matches_32k_back(gpu_ctx):
    """deflate members whose matches are all 3 bytes long (the 1..3-byte copy class), from 32768 bytes back (the
    farthest a deflate distance reaches) and from 1..3 bytes back (periods below the length)"""
    ll_lens = [9] * 256 + [5, 5] + [6] * 28		# complete codes: 256 / 512 + 2 / 32 + 28 / 64 = 1
    d_lens = [4, 4] + [5] * 28			# 2 / 16 + 28 / 32 = 1
    rnd = random.Random(0xDC05)
    bodies, datas = [], []
    for t in range(4):
        plain = bytearray(rnd.randbytes(33000))
        ops = list(plain)
        while len(plain) < 65000:
            if rnd.random() < 0.7:
                plain += plain[-32768:-32768 + 3]
                ops.append((0, 0, 29, 32768 - 24577))	# length 3; distance code 29 + 13 extra bits
            else:
                d = rnd.randint(1, 3)
                for _ in range(3):
                    plain.append(plain[-d])
                ops.append((0, 0, d - 1, 0))
            if rnd.random() < 0.2:
                b = rnd.randrange(256)
                plain.append(b)
                ops.append(b)
        body = _dynamic_block(ll_lens, d_lens, ops).done()
        assert zlib.decompress(body, -15) == bytes(plain)
        bodies.append(body + trailer(bytes(plain)))
        datas.append(bytes(plain))
    res, sm = gpu_inflate(gpu_ctx, bodies, [len(d) for d in datas])
    for (st, out, cons, crc), d in zip(res, datas):
        assert (st, out, crc) == (ST_OK, d, zlib.crc32(d) & 0xFFFFFFFF)
