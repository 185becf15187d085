"""GPU parity for the dependency kernel's walks by looks (la_lz4_deps.hip, la_lz4_dep_walk.h): hand-built blocks that
put the two walks of pass 3 where a look of several positions can go wrong -- many sequence starts in one 32-byte output
chunk, a walk that the sequence's own index ends and not a position, a walk longer than any look, blocks of very few
and of 4 095 and 4 096 sequences -- and blocks that make the fill loops of the plan and of the chunk map run long.

Every case decodes its image with the words (options 0), with the search inside the expand kernel
(LA_LZ4_OPT_SEARCH_IN_EXPAND, which still walks step by step) and with the in-order kernel, compares each with the oracle
and the generator's bytes, and compares the fetched words (la_gpu_lz4_debug_deps) and literal plans
(la_gpu_lz4_debug_literal_plan) of its window blocks, for equality, with the rules as test_gpu_lz4_deps.py and
lz4_literal_plan_rule.py restate them."""
import random
import struct

import numpy as np
import pytest

import streams as S
import test_gpu_lz4_deps as D
from test_gpu_lz4_depchains import lz4_block_from_sequences
from test_gpu_lz4_literal_plan import _plans

pytestmark = pytest.mark.gpu


def _check(ctx, blocks, window=None):
    """one frame of `blocks`: decoded every way, words and plans of the blocks in `window` (default: all) against the
    rules; returns {block: words}"""
    words = D._check(ctx, blocks, window)
    _plans(ctx, D._frame(blocks)[0], {b: len(blocks[b][0]) for b in words})
    return words


def _head(rnd):
    """32 bytes: the sequences behind it start on a chunk edge"""
    return [(rnd.randbytes(28), 7, 4)]


def test_eight_starts_in_one_chunk(gpu_ctx):
    """sixteen 4-byte sequences without literals fill the output chunks [32, 64) and [64, 96): eight sequence starts
    each.  Probes read from the first and the last byte of each of the sixteen (the chunks' first and last bytes among
    them), 4, 5 and 8 bytes and up to each chunk's end: the first walk ends on every entry of a look, the second one
    starts on every one and runs over up to sixteen"""
    rnd = random.Random(0x100C5)
    seqs = _head(rnd) + [(b"", 16, 4) for _ in range(16)]
    cur, probes = 96, []
    for j in range(16):
        for target in (32 + 4 * j, 32 + 4 * j + 3):
            for mlen in (4, 5, 8, 64 - target, 96 - target):
                if mlen < 4:
                    continue
                lit = rnd.randbytes(2)
                seqs.append((lit, cur + 2 - target, mlen))
                if target + mlen <= 96:     # (behind byte 95 the probes themselves follow: the rule alone speaks there)
                    # a 4-byte sequence without literals: nothing drops out of the count
                    probes.append((len(seqs) - 1, 1 + j, (target + mlen - 1 - 32) // 4 + 1 - j))
                cur += 2 + mlen
    words = _check(gpu_ctx, [lz4_block_from_sequences(seqs, rnd.randbytes(6))])[0]
    for k, q, cnt in probes:
        assert words[k] == q | (cnt << 16), (k, hex(words[k]), q, cnt)


@pytest.mark.parametrize("res", range(8))
def test_walk_ended_by_the_own_index(gpu_ctx, res):
    """sequence k stands right behind a run of 4-byte sequences and reads the offsets 4 .. 40 back from its own first
    byte, overlapping itself up to its own start: both walks run into k - 1, the bound, with positions of later
    sequences (and of k itself) behind it in the array.  k mod 8 = res: the bound on every entry of a look"""
    rnd = random.Random(0x100C6 + res)
    seqs, probes = _head(rnd), []
    for off in range(4, 41):
        run = 10 + (res - (len(seqs) + 10)) % 8
        seqs += [(b"", 12, 4)] * run
        assert len(seqs) % 8 == res
        seqs.append((b"", off, 44))
        probes.append((len(seqs) - 1, off))
    words = _check(gpu_ctx, [lz4_block_from_sequences(seqs, rnd.randbytes(6))])[0]
    for k, off in probes:
        # the run's sequences start every 4 bytes up to k's own start: the source's first byte lies in sequence
        # k - ceil(off / 4), its last byte is the one in front of k
        q = k - (off + 3) // 4
        assert words[k] == q | ((k - q) << 16), (k, off, hex(words[k]))


def test_a_walk_longer_than_any_look(gpu_ctx):
    """a source of 300 bytes over 4-byte sequences: 75 of them, the loop behind the second walk's first look; and the
    same source from one byte further in (76 sequences touched)"""
    rnd = random.Random(0x100C7)
    seqs = _head(rnd) + [(b"", 20, 4) for _ in range(120)]
    cur = 32 + 480
    first = 32 + 4 * 20
    seqs.append((b"ab", cur + 2 - first, 300))
    cur += 302
    seqs.append((b"cd", cur + 2 - (first + 1), 300))
    words = _check(gpu_ctx, [lz4_block_from_sequences(seqs, rnd.randbytes(6))])[0]
    assert words[121] == 21 | (75 << 16) and words[122] == 21 | (76 << 16), (hex(words[121]), hex(words[122]))


def _many(rnd, nseq):
    """a block of exactly nseq sequences, the closing literals being the last one"""
    seqs, n = [], 0
    for k in range(nseq - 1):
        lit = rnd.randbytes(rnd.randint(1, 2))
        n += len(lit)
        seqs.append((lit, rnd.randint(1, min(n, 3000)), rnd.randint(4, 8)))
        n += seqs[-1][2]
    return lz4_block_from_sequences(seqs, rnd.randbytes(5))


def test_sequence_counts(gpu_ctx):
    """1, 2, 3, 4, 5, 7, 8, 9, 4 095 and 4 096 sequences: fewer than a look holds, and the array's last entries, where
    no look is taken"""
    rnd = random.Random(0x100C8)
    counts = (1, 2, 3, 4, 5, 7, 8, 9, 4095, 4096)
    blocks = [_many(rnd, n) for n in counts]
    assert all(len(b[1]) <= 65536 for b in blocks)
    words = _check(gpu_ctx, blocks)
    assert [len(words[b]) for b in range(len(counts))] == list(counts)
    # sources right in front of the last sequences of the full blocks: walks that end at index 4 093 and 4 094
    for n in (4095, 4096):
        seqs, cur = [], 0
        for k in range(n - 3):
            lit = b"x" if k == 0 else b""
            seqs.append((lit, 1, 4))
            cur += len(lit) + 4
        seqs.append((b"", 8, 12))      # over the two sequences in front of it, into itself
        seqs.append((b"", 4, 4))
        blk = lz4_block_from_sequences(seqs, rnd.randbytes(5))
        w = _check(gpu_ctx, [blk])[0]
        assert len(w) == n and w[n - 3] == (n - 5) | (2 << 16) and w[n - 2] == (n - 3) | (1 << 16)


def test_block_that_ends_at_65536(gpu_ctx):
    """the block decodes to exactly 65 536 bytes and its last sequence has no match: the position behind it reads 0"""
    rnd = random.Random(0x100C9)
    seqs, n = [], 0
    for k in range(2200):
        lit = rnd.randbytes(rnd.randint(0, 3) if k else 4)
        n += len(lit)
        seqs.append((lit, rnd.randint(1, n), rnd.randint(4, 40)))
        n += seqs[-1][2]
    blk = lz4_block_from_sequences(seqs, rnd.randbytes(65536 - n))
    assert len(blk[1]) == 65536
    assert len(_check(gpu_ctx, [blk])[0]) == 2201


def test_long_fills(gpu_ctx):
    """literal runs of 300 and 1 000 bytes (10 and 32 entries of the plan from one sequence), matches of 300 and 2 000
    bytes (10 and 63 entries of the chunk map), a first sequence that starts its match at byte 500 (the map's lead-in),
    and closing literals of 3 000 bytes (the plan's tail)"""
    rnd = random.Random(0x100CA)
    seqs = [(rnd.randbytes(500), 100, 300), (rnd.randbytes(300), 700, 6), (b"", 4, 2000), (rnd.randbytes(1000), 50, 4),
            (rnd.randbytes(1), 3000, 300), (rnd.randbytes(31), 1, 33), (rnd.randbytes(32), 64, 32)]
    for k in range(300):
        seqs.append((rnd.randbytes(k % 70), rnd.randint(1, 4000), 4 + (k * 37) % 200))
    blk = lz4_block_from_sequences(seqs, rnd.randbytes(3000))
    assert len(blk[1]) <= 65536
    _check(gpu_ctx, [blk])


def test_other_blocks_between_window_blocks(gpu_ctx):
    """a stored block, a block of few long sequences, a 4 097-sequence block and one that fails the parse between window
    blocks: left alone, and the window blocks on both sides have the rule's words and plans"""
    rnd = random.Random(0x100CB)
    w0, w1, w2, w3 = (D._random_block(rnd, 3000) for _ in range(4))
    raw = rnd.randbytes(700)
    long_seqs = lz4_block_from_sequences([(b"ab", 2, 4000)], rnd.randbytes(5))
    good = [w0, (raw, raw, True), w1, long_seqs, w2, _many(rnd, 4097), w3]
    _check(gpu_ctx, good, window=(0, 2, 4, 6))
    bad_payload = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # a match with offset 0
    blocks = good + [(bad_payload, b""), w0]
    img, _ = D._frame(blocks)
    out, rc, msg = D._decode_all_ways(gpu_ctx, img)
    assert (rc, msg) == (-30, "lz4 decompression failed") and out == b"".join(b[1] for b in good)
    for b, (got, want, seq) in D._words(gpu_ctx, img, {0: len(w0[1]), 6: len(w3[1]), 8: len(w0[1])}).items():
        assert len(seq) > 0 and got == want, b
    _plans(gpu_ctx, img, {b: len(blocks[b][0]) for b in (0, 2, 4, 6, 8)})


def test_generated_blocks_of_1_to_64_kib(gpu_ctx):
    """64 blocks of the bench generator, 1 .. 64 KiB decoded, one frame each in one image"""
    parts, plains, olen, src_len = [], [], {}, {}
    for i in range(1, 65):
        img, plain = S.synth_lz4_stream(0x100CC00 + i, 0, 1, blocks_per_frame=1, block_size=i * 1024, nthreads=1)
        head = img[:11].tobytes()
        assert head[:4] == S.MAGIC and head[4] == 0x74     # magic, FLG, BD, HC, then the block's length word
        word = struct.unpack("<I", head[7:11])[0]
        if not word >> 31:
            olen[i - 1], src_len[i - 1] = plain.size, word
        parts.append(img)
        plains.append(plain.tobytes())
    assert len(olen) >= 60
    img = np.concatenate(parts)
    out, rc, msg = D._decode_all_ways(gpu_ctx, img)
    assert (rc, msg) == (0, "") and out == b"".join(plains)
    for b, (got, want, seq) in D._words(gpu_ctx, img, olen).items():
        assert len(seq) > 0 and got == want, (b, [(k, hex(g), hex(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w][:8])
    _plans(gpu_ctx, img, src_len)
