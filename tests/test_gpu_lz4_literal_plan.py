"""GPU parity for the literal plan of the lz4 window path: the dependency kernel (la_lz4_deps.hip) writes, per 32-byte
chunk of a block's payload, the first sequence with literals in or behind the chunk, and the LDS-window expand kernel
starts its literal phase from those entries instead of building the index itself.  Every case decodes its image with the
plan (options 0), with the kernel's own index (LA_LZ4_OPT_SEARCH_IN_EXPAND) and with the in-order kernel, compares each
with the oracle and with the generator's bytes, and fetches the plan of its window blocks
(la_gpu_lz4_debug_literal_plan) to compare it, for equality, with the rule restated in lz4_literal_plan_rule.py over
the fetched table entries."""
import ctypes as C
import random

import numpy as np
import pytest

import lz4_literal_plan_rule as R
import oracle_lib as O
from test_gpu_lz4_depchains import lz4_block_from_sequences
from test_gpu_lz4_deps import _decode_all_ways, _frame, _random_block

pytestmark = pytest.mark.gpu


def _plans(ctx, img, which):
    """{block: (table entries, fetched plan)} for the blocks in `which` = {block: payload length}, from one decode
    with the plan in use; every fetched plan is compared with the rule"""
    from libarchive_amd.lz4 import decode_image
    _, _, _, plan = decode_image(ctx, img, options=0)
    res = {}
    for b, src_len in which.items():
        seq = ctx.lz4_debug_deps(plan.batch, b, cap=4096)[0]
        got = [int(x) for x in ctx.lz4_debug_literal_plan(plan.batch, b)]
        want = R.rule_plan(seq, src_len)
        assert len(seq) > 0 and len(got) == R.plan_entries(src_len), (b, len(seq), len(got))
        assert got == want, (b, [(c, g, w) for c, (g, w) in enumerate(zip(got, want)) if g != w][:8])
        res[b] = (seq, got)
    return res


def _check(ctx, blocks, window=None):
    """one frame of `blocks` decoded every way, the plans of the blocks in `window` (default: all) against the rule"""
    img, plain = _frame(blocks)
    out, rc, msg = _decode_all_ways(ctx, img)
    assert (rc, msg) == (0, "") and out == plain
    return _plans(ctx, img, {b: len(blocks[b][0]) for b in (range(len(blocks)) if window is None else window)})


def _runs(seq):
    """(first payload byte, payload byte behind the last one) of every literal run with bytes in it"""
    return [(ls, ls + ll) for ls, ll, _, _ in map(R.fields, seq) if ll]


LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 270, 1000)


def _placement_blocks():
    rnd = random.Random(0x11B0)
    blocks, seqs, n = [], [], 0
    for ll in LENGTHS:
        for fill in range(40):
            for lit in (rnd.randbytes(fill + (n == 0)), rnd.randbytes(ll)):
                n += len(lit)
                seqs.append((lit, rnd.randint(1, n), rnd.randint(4, 9)))
                n += seqs[-1][2]
            if n > 12000:
                blocks.append(lz4_block_from_sequences(seqs, rnd.randbytes(6)))
                seqs, n = [], 0
    blocks.append(lz4_block_from_sequences(seqs, rnd.randbytes(6)))
    return blocks


def test_run_lengths_and_placements(gpu_ctx):
    """literal runs of 0 .. 9, 15, 16, 270 and 1 000 bytes behind fillers of 0 .. 39 literals: every run length starts
    on every payload offset mod 4, runs start on every offset mod 32 and end 0 .. 3 bytes short of, on and 1 .. 3
    bytes past a chunk edge"""
    res = _check(gpu_ctx, _placement_blocks())
    runs = [r for seq, _ in res.values() for r in _runs(seq)]
    for ll in LENGTHS[1:]:
        assert {ls & 3 for ls, le in runs if le - ls == ll} == {0, 1, 2, 3}, ll
    assert {ls & 31 for ls, le in runs} == set(range(32))
    assert {le & 31 for ls, le in runs} >= {29, 30, 31, 0, 1, 2, 3}
    assert sum(R.fields(e)[1] == 0 for seq, _ in res.values() for e in seq) >= 40


def test_many_sequences_in_one_chunk(gpu_ctx):
    """eight sequences of no or one literal inside one payload chunk: more than the six entries a thread asks for"""
    rnd = random.Random(0x11B1)
    seqs = [(rnd.randbytes(29), 7, 4)] + [(rnd.randbytes(i & 1), 5, 4) for i in range(8)] + [(rnd.randbytes(30), 9, 6)]
    seq, plan = _check(gpu_ctx, [lz4_block_from_sequences(seqs, rnd.randbytes(9))])[0]
    starts = [R.fields(e)[0] for e in seq]
    assert sum(1 for s in starts if s >> 5 == 1) == 9 and plan[1] == 1      # the chunk's thread walks sequences 1 .. 9


def test_runs_across_the_thread_batch_edges(gpu_ctx):
    """a run across payload chunks 511 | 512 (the second chunk of thread 0) and one across 1 023 | 1 024 (the second
    trip of the literal phase, payload above 32 KiB)"""
    rnd = random.Random(0x11B2)
    fill = lambda count: [(rnd.randbytes(14), rnd.randint(1, 14), 4) for _ in range(count)]      # 17 payload bytes each
    seqs = fill(963) + [(rnd.randbytes(40), 100, 4)] + fill(960) + [(rnd.randbytes(40), 100, 4)] + fill(20)
    enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(50))
    assert len(enc) > 32768 + 64 and len(plain) <= 65536
    seq, plan = _check(gpu_ctx, [(enc, plain)])[0]
    for edge, k in ((16384, 963), (32768, 963 + 1 + 960)):
        ls, ll, _, _ = R.fields(seq[k])
        assert ll == 40 and ls < edge - 3 and ls + ll > edge + 3 and plan[edge >> 5] == k, (edge, ls)


def test_long_runs(gpu_ctx):
    """a run of 5 000 bytes, and one of 60 000 bytes in a block with enough short sequences to stay a window block"""
    rnd = random.Random(0x11B3)
    short = lambda count: [(rnd.randbytes(1), rnd.randint(1, 1 + 5 * i), 4) for i in range(count)]
    b5 = lz4_block_from_sequences(short(20) + [(rnd.randbytes(5000), 77, 8)] + short(20), rnd.randbytes(9))
    b60 = lz4_block_from_sequences(short(70) + [(rnd.randbytes(60000), 300, 5)] + short(70), rnd.randbytes(9))
    assert len(b60[1]) <= 65536 and 142 * 512 > len(b60[1])
    res = _check(gpu_ctx, [b5, b60])
    assert max(le - ls for ls, le in _runs(res[1][0])) == 60000 and res[1][1].count(70) > 1800


def test_block_sizes(gpu_ctx):
    """blocks of one and of two sequences; first runs at payload offsets 1, 2 and 3; 4 096 sequences, and 4 097 in the
    same batch (segmented launch: no plan); a block that decodes to exactly 65 536 bytes, its closing literals up to
    the last byte"""
    rnd = random.Random(0x11B4)
    lit_only = lz4_block_from_sequences([], rnd.randbytes(100))
    one = lz4_block_from_sequences([(b"abcd", 2, 8)], rnd.randbytes(5))
    firsts = [lz4_block_from_sequences([(rnd.randbytes(ll), 1, 4)], rnd.randbytes(5)) for ll in (14, 269, 270)]

    def many(nseq):
        seqs, n = [], 0
        for k in range(nseq - 1):
            lit = rnd.randbytes(rnd.randint(1, 2))
            n += len(lit)
            seqs.append((lit, rnd.randint(1, min(n, 3000)), rnd.randint(4, 8)))
            n += seqs[-1][2]
        return lz4_block_from_sequences(seqs, rnd.randbytes(5))

    b4096, b4097 = many(4096), many(4097)
    seqs, n = [], 0
    for k in range(2000):
        n += 4
        seqs.append((rnd.randbytes(4), rnd.randint(1, n), 28))
        n += 28
    full = lz4_block_from_sequences(seqs, rnd.randbytes(65536 - n))
    assert len(full[1]) == 65536
    blocks = [lit_only, one] + firsts + [b4096, b4097, full]
    res = _check(gpu_ctx, blocks, window=(0, 1, 2, 3, 4, 5, 7))
    assert [len(res[b][0]) for b in (0, 1, 5, 7)] == [1, 2, 4096, 2001]
    assert [R.fields(res[b][0][0])[0] for b in (2, 3, 4)] == [1, 2, 3]
    assert _runs(res[7][0])[-1][1] == len(full[0])
    from libarchive_amd.lz4 import decode_image
    _, _, _, plan = decode_image(gpu_ctx, _frame(blocks)[0], options=0)
    assert len(gpu_ctx.lz4_debug_deps(plan.batch, 6, cap=8192)[0]) == 4097
    assert len(gpu_ctx.lz4_debug_literal_plan(plan.batch, 6)) == 0


def test_last_block_of_the_image(gpu_ctx):
    """payloads of 65 .. 97 bytes (1 .. 33 mod 32) in the image's last block: the last chunk is short in every way"""
    rnd = random.Random(0x11B5)
    lead = _random_block(rnd, 500)
    for want in range(65, 98):
        last = lz4_block_from_sequences([(rnd.randbytes(8), 3, 4)], rnd.randbytes(want - 13))
        assert len(last[0]) == want
        _check(gpu_ctx, [lead, last])


def test_window_block_behind_an_odd_length_block(gpu_ctx):
    """the slab offset of the second block is not 16-aligned, its payload offset odd"""
    rnd = random.Random(0x11B6)
    odd = lz4_block_from_sequences([], rnd.randbytes(101))
    _check(gpu_ctx, [odd, _random_block(rnd, 3000), _random_block(rnd, 777)])


def test_rows_that_name_the_same_payload_twice(gpu_ctx):
    """a caller-built block table: every block of the image twice in a row and once more at the end.  The plans lie
    by table slot, so each row has its own and all of them are the rule's.  (The table's room follows the image's
    length: a stored block that no row names makes the image long enough for twelve slots.)"""
    import torch
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import Lz4DevicePlan
    rnd = random.Random(0x11B7)
    blocks = [_random_block(rnd, size) for size in (900, 4000, 150, 2500)]
    pad = rnd.randbytes(40000)
    img, _ = _frame(blocks + [(pad, pad, True)])
    ref, res = O.lz4_stream_decode(img, 1 << 20)
    assert res.rc == 0 and ref.tobytes() == b"".join(b[1] for b in blocks) + pad
    image = np.frombuffer(img, dtype=np.uint8)
    idx = N.lz4_index(image, at_eof=True)
    rows = [0, 0, 1, 1, 2, 2, 3, 3, 0, 1, 2, 3]
    tab = idx.blocks[np.asarray(rows)].copy()
    hand = N.Lz4Index(tab, idx.frames[:0].copy(), idx.end_kind, idx.consumed, int(tab["dst_cap"].astype(np.uint64).sum()))
    plan = Lz4DevicePlan(gpu_ctx, torch.from_numpy(image.copy()).to("cuda:0"), hand)
    plan.run(0)
    out_len, dst_off, bst, _ = [a.copy() for a in plan.arrays()]
    assert not bst.any() and out_len.tolist() == [len(blocks[r][1]) for r in rows]
    assert plan.d_dst[:int(dst_off[-1])].cpu().numpy().tobytes() == b"".join(blocks[r][1] for r in rows)
    for i, r in enumerate(rows):
        seq = gpu_ctx.lz4_debug_deps(plan.batch, i, cap=4096)[0]
        got = [int(x) for x in gpu_ctx.lz4_debug_literal_plan(plan.batch, i)]
        assert len(seq) > 0 and got == R.rule_plan(seq, len(blocks[r][0])), i


def test_routing_leaves_other_blocks_alone(gpu_ctx):
    """a stored block, a block of few long sequences (general kernel) and a block whose payload fails, between window
    blocks: bytes, return code and message are the oracle's, the window blocks have the rule's plans and the others
    none"""
    from libarchive_amd.lz4 import decode_image
    rnd = random.Random(0x11B8)
    w0, w1, w2 = (_random_block(rnd, 3000) for _ in range(3))
    raw = rnd.randbytes(700)
    long_seqs = lz4_block_from_sequences([(b"ab", 2, 4000)], rnd.randbytes(5))
    good = [w0, (raw, raw, True), long_seqs, w1]
    _check(gpu_ctx, good, window=(0, 3))
    bad_payload = bytes([0x10]) + b"A" + b"\x00\x00" + bytes([0x50]) + b"12345"      # a match with offset 0
    img, _ = _frame(good + [(bad_payload, b"")] + [w2])
    out, rc, msg = _decode_all_ways(gpu_ctx, img)
    assert (rc, msg) == (-30, "lz4 decompression failed") and out == b"".join(b[1] for b in good)
    _plans(gpu_ctx, img, {0: len(w0[0]), 3: len(w1[0]), 5: len(w2[0])})
    _, _, _, plan = decode_image(gpu_ctx, img, options=0)
    assert [len(gpu_ctx.lz4_debug_literal_plan(plan.batch, b)) for b in (1, 2, 4)] == [0, 0, 0]


def test_a_smaller_image_behind_a_larger_one(gpu_ctx):
    """two images back to back on one context, the second with fewer blocks, shorter payloads and fewer literals per
    block: every entry the second decode can read is its own, nothing of the first one's shows"""
    rnd = random.Random(0x11B9)
    big = [_random_block(rnd, 6000) for _ in range(12)]
    small = []
    for _ in range(7):
        seqs, n = [(rnd.randbytes(2), 1, 30)], 32
        while n < 1500:
            seqs.append((rnd.randbytes(rnd.randint(0, 1)), rnd.randint(1, n), rnd.randint(20, 40)))
            n += len(seqs[-1][0]) + seqs[-1][2]
        small.append(lz4_block_from_sequences(seqs, rnd.randbytes(5)))
    assert max(len(b[0]) for b in small) * 4 < min(len(b[0]) for b in big)
    _check(gpu_ctx, big)
    _check(gpu_ctx, small)


def test_no_plan_behind_a_decode_that_searches_in_the_expand_kernel(gpu_ctx):
    from libarchive_amd import _native as N
    from libarchive_amd.lz4 import decode_image
    rnd = random.Random(0x11BA)
    blk = _random_block(rnd, 2000)
    img, plain = _frame([blk])
    buf = np.zeros(64, dtype=np.uint16)
    for opt, want in ((0, R.plan_entries(len(blk[0]))), (N.LA_LZ4_OPT_SEARCH_IN_EXPAND, N.LA_ERR_ARG)):
        out, rc, msg, plan = decode_image(gpu_ctx, img, options=opt)
        assert rc == 0 and out.tobytes() == plain
        got = N.gpu_lib().la_gpu_lz4_debug_literal_plan(gpu_ctx._h, C.byref(plan.batch), 0, buf.ctypes.data, 64)
        assert got == want, (opt, got)


def test_sweep_of_random_blocks(gpu_ctx):
    """200 seeded random blocks of about 4 KiB (literal runs of 0 .. 6 bytes, match lengths 4 .. 40) in one batch"""
    rnd = random.Random(0x11BB)
    _check(gpu_ctx, [_random_block(rnd, 4096) for _ in range(200)])
