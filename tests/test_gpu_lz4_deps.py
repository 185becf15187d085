"""GPU parity for the dependency kernel of the lz4 window path (la_lz4_deps.hip): it finds, ahead of the LDS-window expand
kernel, what every match has to wait for -- one word per sequence, the first sequence under the match source in the low
16 bits and the number of sequences whose match must be in the window above them.  A word that waits for too little
shows in the decoded bytes only as a race, so every case here does two things: it decodes the image with the words
(options 0), with the search inside the expand kernel (LA_LZ4_OPT_SEARCH_IN_EXPAND) and with the in-order kernel, and
compares each result with the oracle and with the bytes the generator meant; and it fetches the words of its window
blocks (la_gpu_lz4_debug_deps) and compares them, for equality, with the rule restated below over the fetched table
entries."""
import bisect
import random

import pytest

import oracle_lib as O
import streams as S
from test_gpu_lz4 import gpu_decode
from test_gpu_lz4_depchains import lz4_block_from_sequences

pytestmark = pytest.mark.gpu


def rule_words(seq, olen):
    """The words of one block from its table entries (lit_src | lit_len << 16 | dst << 32 | off << 48) and its decoded
    length.  Sequence k puts its literals at dst and its match behind them; the match reads min(mlen, off) bytes from
    dst + lit_len - off (an overlapping match reads its own bytes behind that), and what lies at or behind dst is the
    sequence's own.  q: the last earlier sequence that starts at or before the source; qe: the last that starts at or
    before the source's last byte; the matches of q .. qe are waited for, without qe's when the source ends inside
    qe's literals.  Nothing is waited for by sequence 0, by an empty match, or by a source inside the own literals."""
    ent = [int(e) for e in seq]
    lit_len = [(e >> 16) & 0xFFFF for e in ent]
    dst = [(e >> 32) & 0xFFFF for e in ent]
    off = [e >> 48 for e in ent]
    ns, words = len(ent), []
    for k in range(ns):
        if k == 0:
            words.append(0)
            continue
        d, mdst = dst[k], dst[k] + lit_len[k]
        mlen = ((dst[k + 1] if k + 1 < ns else olen & 0xFFFF) - mdst) & 0xFFFF
        s0 = mdst - off[k]
        q = bisect.bisect_right(dst, s0, 0, k) - 1
        cnt = 0
        if mlen and s0 < d:
            hi = min(s0 + min(mlen, off[k]) - 1, d - 1)
            qe = bisect.bisect_right(dst, hi, 0, k) - 1
            cnt = qe - q + 1 - (1 if hi < dst[qe] + lit_len[qe] else 0)
        words.append(q | (cnt << 16))
    return words


def _frame(blocks):
    """blocks: (encoded, decoded) or (encoded, decoded, stored flag); one frame, block and content checksums on"""
    return S.lz4_frame([(b[1], S.lz4_block(b[0], stored=len(b) > 2 and b[2], bsum=True)) for b in blocks], flg=0x74)


def _decode_all_ways(ctx, img):
    """the three expand paths against the oracle; returns the oracle's (bytes, rc, message)"""
    from libarchive_amd import _native as N
    ref, res = O.lz4_stream_decode(img, 1 << 23)
    want = (ref.tobytes(), res.rc, res.errmsg.decode())
    for opt in (0, N.LA_LZ4_OPT_SEARCH_IN_EXPAND, N.LA_LZ4_OPT_EXPAND_INORDER):
        assert gpu_decode(ctx, img, options=opt) == want, opt
    return want


def _words(ctx, img, which):
    """{block: (fetched words, rule's words)} for the blocks in `which` = {block: decoded length}, from a decode with
    the words in use"""
    from libarchive_amd.lz4 import decode_image
    _, _, _, plan = decode_image(ctx, img, options=0)
    got = {}
    for b, olen in which.items():
        seq, deps = ctx.lz4_debug_deps(plan.batch, b, cap=4096)
        got[b] = ([int(w) for w in deps], rule_words(seq, olen), seq)
    return got


def _check(ctx, blocks, window=None):
    """decodes one frame of `blocks` every way and compares the words of the blocks listed in `window` (default: all)
    with the rule; returns {block: words}"""
    img, plain = _frame(blocks)
    out, rc, msg = _decode_all_ways(ctx, img)
    assert (rc, msg) == (0, "") and out == plain
    which = {b: len(blocks[b][1]) for b in (range(len(blocks)) if window is None else window)}
    res = {}
    for b, (got, want, seq) in _words(ctx, img, which).items():
        assert len(seq) > 0, b
        assert got == want, (b, [(k, hex(g), hex(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8])
        res[b] = got
    return res


def _fillers(rnd, n, lit_len, mlen):
    """n sequences of lit_len literals and an mlen-byte match that copies from the block's first bytes (a source in the
    literals of sequence 0: no wait); returns (sequences, start of each sequence, start of each match, bytes so far)"""
    seqs, pos, mstart, cur = [], [], [], 0
    for k in range(n):
        ll = max(lit_len, mlen) if k == 0 else lit_len
        pos.append(cur)
        mstart.append(cur + ll)
        seqs.append((rnd.randbytes(ll), cur + ll, mlen))       # offset back to byte 0
        cur += ll + mlen
    return seqs, pos, mstart, cur


def test_source_placement(gpu_ctx):
    """probes behind 40 sequences of 6 literals + 6 match bytes: a source that starts exactly at a sequence's position,
    one byte before it, that ends on the last literal byte of the last touched sequence (which drops out of the count),
    on the first byte of that sequence's match (it stays), and that lies wholly inside one literal run (count 0)"""
    rnd = random.Random(0xDE01)
    seqs, pos, mstart, cur = _fillers(rnd, 40, 6, 6)
    probes = []     # (index of the probe sequence, expected q, expected count)

    def probe(target, mlen, q, cnt):
        nonlocal cur
        lit = rnd.randbytes(2)
        seqs.append((lit, cur + len(lit) - target, mlen))
        probes.append((len(seqs) - 1, q, cnt))
        cur += len(lit) + mlen

    probe(pos[10], 12, 10, 1)               # literals and match of 10, nothing of 11
    probe(pos[10] - 1, 7, 9, 1)             # last match byte of 9, then literals of 10 only: 10 drops out
    probe(mstart[20] - 8, 8, 19, 1)         # ends on the last literal byte of 20: match of 19 only
    probe(mstart[20] - 7, 8, 19, 2)         # ends on the first byte of 20's match: it stays
    probe(pos[30] + 1, 4, 30, 0)            # inside the literals of 30
    probe(pos[5] + 2, 30, 5, 3)             # over 5, 6 and into the match of 7
    enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(5))
    assert len(plain) <= 8192
    words = _check(gpu_ctx, [(enc, plain)])[0]
    for k, q, cnt in probes:
        assert words[k] == q | (cnt << 16), (k, hex(words[k]), q, cnt)


def test_waits_across_flag_words(gpu_ctx):
    """a chain through every match (sequences 31, 32 and 33 all wait), and sources that cover 33 and 70 earlier
    sequences: counts above 32, ranges over two and three 32-sequence flag words"""
    rnd = random.Random(0xDE02)
    chain, prev = [], None
    for i in range(100):
        mlen = rnd.randint(4, 9)
        chain.append((rnd.randbytes(1), prev + 1 if prev is not None else 1, mlen))
        prev = mlen
    enc_c, plain_c = lz4_block_from_sequences(chain, rnd.randbytes(5))
    seqs, pos, mstart, cur = _fillers(rnd, 200, 1, 4)
    seqs.append((b"xy", cur + 2 - pos[40], pos[73] - pos[40]))      # exactly sequences 40 .. 72
    k33, cur = len(seqs) - 1, cur + 2 + pos[73] - pos[40]
    seqs.append((b"", cur - pos[20], pos[90] - pos[20]))            # exactly sequences 20 .. 89
    k70 = len(seqs) - 1
    enc_w, plain_w = lz4_block_from_sequences(seqs, rnd.randbytes(5))
    assert len(plain_c) <= 8192 and len(plain_w) <= 8192
    words = _check(gpu_ctx, [(enc_c, plain_c), (enc_w, plain_w)])
    for k in (31, 32, 33):
        assert words[0][k] >> 16 >= 1, (k, hex(words[0][k]))
    assert words[1][k33] == 40 | (33 << 16) and words[1][k70] == 20 | (70 << 16)


def test_overlapping_matches(gpu_ctx):
    """off = 1..15 with mlen > off: the source is one period, not the match length"""
    rnd = random.Random(0xDE03)
    seqs, n = [(rnd.randbytes(20), 7, 5)], 25
    for rep in range(6):
        for off in range(1, 16):
            lit = rnd.randbytes(rnd.randint(0, 2))
            mlen = off + rnd.randint(1, 40)
            seqs.append((lit, off, mlen))
            n += len(lit) + mlen
    enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(5))
    assert len(plain) <= 8192
    words = _check(gpu_ctx, [(enc, plain)])[0]
    assert any(w >> 16 for w in words) and not all(w >> 16 for w in words[1:-1])


def test_block_sizes(gpu_ctx):
    """a literal-only block, one match only, exactly 4096 sequences (the last block the window launch takes), 4097
    sequences in the same batch (segmented launch, search in the kernel), and a block that decodes to exactly 65 536
    bytes (its 16-bit end position reads 0)"""
    rnd = random.Random(0xDE04)
    lit_only = lz4_block_from_sequences([], rnd.randbytes(100))
    one = lz4_block_from_sequences([(b"abcd", 2, 8)], rnd.randbytes(5))

    def many(nseq):
        seqs, n = [], 0
        for k in range(nseq - 1):       # the block's last sequence is its closing literals
            lit = rnd.randbytes(rnd.randint(1, 2))
            n += len(lit)
            seqs.append((lit, rnd.randint(1, min(n, 3000)), rnd.randint(4, 8)))
            n += seqs[-1][2]
        return lz4_block_from_sequences(seqs, rnd.randbytes(5))

    b4096, b4097 = many(4096), many(4097)
    seqs, n = [], 0
    for k in range(2000):
        lit = rnd.randbytes(4)
        n += 4
        seqs.append((lit, rnd.randint(1, n), 28))
        n += 28
    full = lz4_block_from_sequences(seqs, rnd.randbytes(65536 - n))
    assert len(full[1]) == 65536 and len(b4097[1]) <= 65536
    blocks = [lit_only, one, b4096, b4097, full]
    words = _check(gpu_ctx, blocks, window=(0, 1, 2, 4))
    assert words[0] == [0] and len(words[1]) == 2 and len(words[2]) == 4096 and len(words[4]) == 2001
    from libarchive_amd.lz4 import decode_image
    _, _, _, plan = decode_image(gpu_ctx, _frame(blocks)[0], options=0)
    assert len(gpu_ctx.lz4_debug_deps(plan.batch, 3, cap=8192)[0]) == 4097


def test_window_block_behind_an_odd_length_block(gpu_ctx):
    """the slab offset of the second block is not 16-aligned"""
    rnd = random.Random(0xDE05)
    odd = lz4_block_from_sequences([], rnd.randbytes(101))
    seqs, n = [], 0
    for k in range(300):
        lit = rnd.randbytes(rnd.randint(0, 5))
        n += len(lit)
        if n == 0:
            lit, n = b"q", 1
        seqs.append((lit, rnd.randint(1, n), rnd.randint(4, 20)))
        n += seqs[-1][2]
    _check(gpu_ctx, [odd, lz4_block_from_sequences(seqs, rnd.randbytes(7))])


def _random_block(rnd, size):
    seqs, n = [], 0
    while n < size:
        lit = rnd.randbytes(rnd.randint(0, 6))
        n += len(lit)
        if n == 0:
            lit, n = rnd.randbytes(1), 1
        seqs.append((lit, rnd.randint(1, n), rnd.randint(4, 40)))
        n += seqs[-1][2]
    return lz4_block_from_sequences(seqs, rnd.randbytes(5))


def test_routing_leaves_other_blocks_alone(gpu_ctx):
    """one frame of window blocks, a stored block, a block of few long sequences (general kernel) and a block whose
    payload fails the parse: bytes, return code and message are the oracle's, and the window blocks on both sides of
    the others have the rule's words"""
    rnd = random.Random(0xDE06)
    w0, w1, w2 = (_random_block(rnd, 3000) for _ in range(3))
    raw = rnd.randbytes(700)
    stored = (raw, raw, True)
    long_seqs = lz4_block_from_sequences([(b"ab", 2, 4000)], rnd.randbytes(5))
    good = [w0, stored, long_seqs, w1]
    _check(gpu_ctx, good, window=(0, 3))
    bad_payload = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # a match with offset 0
    img, _ = _frame(good + [(bad_payload, b"")] + [w2])
    out, rc, msg = _decode_all_ways(gpu_ctx, img)
    assert (rc, msg) == (-30, "lz4 decompression failed") and out == b"".join(b[1] for b in good)
    for b, (got, want, seq) in _words(gpu_ctx, img, {0: len(w0[1]), 3: len(w1[1]), 5: len(w2[1])}).items():
        assert len(seq) > 0 and got == want, b


def test_sweep_of_random_blocks(gpu_ctx):
    """200 seeded random blocks of about 4 KiB (match lengths 4..40, offsets uniform over the output so far) in one batch"""
    rnd = random.Random(0xDE07)
    _check(gpu_ctx, [_random_block(rnd, 4096) for _ in range(200)])
