"""GPU parity for the dword-wise literal placement of the lz4 window kernel (la_lz4_fast.hip, DEPS = true): a chunk's
thread picks, for each of the chunk's eight dwords, the one run of the six it fetched that stores it
(la_lz4_lit_run_dwords, la_dev.h), where the other instantiations walk the dwords once per run.  Every case decodes its
image with default options (the dword-wise form), with LA_LZ4_OPT_SEARCH_IN_EXPAND (the run-wise form in the same
kernel) and with the in-order kernel; each must equal the oracle and the generator's bytes.  What a case is meant to
contain is asserted on its parsed table (lz4_literal_plan_rule.py)."""
import random

import pytest

import lz4_literal_plan_rule as R
from test_gpu_lz4_depchains import lz4_block_from_sequences
from test_gpu_lz4_deps import _decode_all_ways, _frame, _random_block

pytestmark = pytest.mark.gpu


def _check(ctx, blocks):
    """one frame of `blocks` decoded every way; returns every block's parsed table"""
    img, plain = _frame(blocks)
    assert plain == b"".join(b[1] for b in blocks)
    out, rc, msg = _decode_all_ways(ctx, img)
    assert (rc, msg) == (0, "") and out == plain
    return [R.parse_block(b[0])[0] for b in blocks]


def _runs(ent):
    return [(ls, ls + ll) for ls, ll, _, _ in map(R.fields, ent)]


def _starts_per_chunk(ent):
    count = {}
    for ls, _ in _runs(ent):
        count[ls >> 5] = count.get(ls >> 5, 0) + 1
    return count


LENGTHS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 270)


def test_run_lengths_and_placements(gpu_ctx):
    """literal runs of 0 .. 9, 15, 16 and 270 bytes behind fillers of 0 .. 39 literals: every length starts on every
    payload offset mod 4, runs start on every offset mod 32 and end 0 .. 3 bytes short of, on and 1 .. 3 bytes past a
    chunk edge"""
    rnd = random.Random(0x1E10)
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
    runs = [r for ent in _check(gpu_ctx, blocks) for r in _runs(ent)]
    for ll in LENGTHS:
        assert {ls & 3 for ls, le in runs if le - ls == ll} == {0, 1, 2, 3}, ll
    assert {ls & 31 for ls, le in runs if le > ls} == set(range(32))
    assert {le & 31 for ls, le in runs if le > ls} >= {29, 30, 31, 0, 1, 2, 3}


@pytest.mark.parametrize("count", range(1, 10))
def test_sequences_starting_in_one_chunk(gpu_ctx, count):
    """1 .. 9 sequences of no or one literal start in the payload's second chunk: up to the six runs a thread places
    dword by dword, and the loop behind them"""
    rnd = random.Random(0x1E20 + count)
    seqs = [(rnd.randbytes(28), 7, 4)] + [(rnd.randbytes(i & 1), 5, 4) for i in range(count - 1)] + [(rnd.randbytes(40), 9, 6)]
    ent, = _check(gpu_ctx, [lz4_block_from_sequences(seqs, rnd.randbytes(9))])
    assert _starts_per_chunk(ent)[1] == count


def test_one_lane_with_six_runs(gpu_ctx):
    """a run of 2 500 bytes gives every chunk of a wave one run, then six runs start in one chunk of the same wave:
    the run slots behind the first belong to one lane; and a block of long runs only, whose waves skip them all"""
    rnd = random.Random(0x1E30)
    for first in range(2500, 2532):     # (the length that puts the six short runs into one chunk)
        seqs = [(rnd.randbytes(first), 40, 5)] + [(rnd.randbytes(1), 9, 4) for _ in range(6)] + [(rnd.randbytes(1500), 77, 4)]
        lone = lz4_block_from_sequences(seqs, rnd.randbytes(300))
        if max(_starts_per_chunk(R.parse_block(lone[0])[0]).values()) >= 6:
            break
    long_only = lz4_block_from_sequences([(rnd.randbytes(3000), 100, 8), (rnd.randbytes(4000), 2000, 8)], rnd.randbytes(900))
    ent, ent_long = _check(gpu_ctx, [lone, long_only])
    per = _starts_per_chunk(ent)
    busy = [c for c, v in per.items() if v >= 6]
    assert len(busy) == 1 and busy[0] < 128 and all(v <= 2 for c, v in per.items() if c != busy[0])
    assert max(_starts_per_chunk(ent_long).values()) == 1


def test_block_sizes(gpu_ctx):
    """blocks of one and of two sequences; first runs at payload offsets 1, 2 and 3; a block that decodes to exactly
    65 536 bytes, its closing literals up to the last byte; a block of 4 097 sequences (segmented kernel, run-wise form)
    between window blocks"""
    rnd = random.Random(0x1E40)
    lit_only = lz4_block_from_sequences([], rnd.randbytes(100))
    one = lz4_block_from_sequences([(b"abcd", 2, 8)], rnd.randbytes(5))
    firsts = [lz4_block_from_sequences([(rnd.randbytes(ll), 1, 4)], rnd.randbytes(5)) for ll in (14, 269, 270)]
    seqs, n = [], 0
    for k in range(4096):
        lit = rnd.randbytes(rnd.randint(1, 2))
        n += len(lit)
        seqs.append((lit, rnd.randint(1, min(n, 3000)), rnd.randint(4, 8)))
        n += seqs[-1][2]
    b4097 = lz4_block_from_sequences(seqs, rnd.randbytes(5))
    seqs, n = [], 0
    for k in range(2000):
        n += 4
        seqs.append((rnd.randbytes(4), rnd.randint(1, n), 28))
        n += 28
    full = lz4_block_from_sequences(seqs, rnd.randbytes(65536 - n))
    assert len(full[1]) == 65536
    ents = _check(gpu_ctx, [lit_only, one] + firsts + [_random_block(rnd, 3000), b4097, full, _random_block(rnd, 777)])
    assert [len(ents[b]) for b in (0, 1, 6, 7)] == [1, 2, 4097, 2001]
    assert [R.fields(ents[b][0])[0] for b in (2, 3, 4)] == [1, 2, 3]
    assert _runs(ents[7])[-1][1] == len(full[0])


def test_payload_above_32_kib(gpu_ctx):
    """a payload of more than 32 KiB, the literal phase's second trip: a run across payload chunks 511 | 512 (the
    second chunk of thread 0) and one across 1 023 | 1 024, and twice behind them sixteen one-byte runs in a row (64
    payload bytes: some chunk holds eight of them)"""
    rnd = random.Random(0x1E50)
    fill = lambda count: [(rnd.randbytes(14), rnd.randint(1, 14), 4) for _ in range(count)]      # 17 payload bytes each
    six = lambda: [(rnd.randbytes(1), 3, 4) for _ in range(16)]
    seqs = (fill(963) + [(rnd.randbytes(40), 100, 4)] + fill(960) + [(rnd.randbytes(40), 100, 4)] + fill(8) + six()
            + fill(1070) + six() + fill(20))
    enc, plain = lz4_block_from_sequences(seqs, rnd.randbytes(50))
    assert len(enc) > 32768 + 64 and len(plain) <= 65536 and len(seqs) < 4096
    ent, = _check(gpu_ctx, [(enc, plain)])
    for edge, k in ((16384, 963), (32768, 963 + 1 + 960)):
        ls, ll, _, _ = R.fields(ent[k])
        assert ll == 40 and ls < edge - 3 and ls + ll > edge + 3, (edge, ls)
    assert sum(1 for c, v in _starts_per_chunk(ent).items() if c >= 1024 and v >= 6) >= 2


def test_last_chunk_of_1_to_31_bytes(gpu_ctx):
    """payloads of 65 .. 95 bytes in the image's last block: the last chunk holds 1 .. 31 bytes"""
    rnd = random.Random(0x1E60)
    lead = _random_block(rnd, 500)
    for want in range(65, 96):
        last = lz4_block_from_sequences([(rnd.randbytes(8), 3, 4)], rnd.randbytes(want - 13))
        assert len(last[0]) == want
        _check(gpu_ctx, [lead, last])


def test_sweep_of_random_blocks(gpu_ctx):
    """200 seeded random blocks of about 4 KiB (literal runs of 0 .. 6 bytes, match lengths 4 .. 40) in one batch"""
    rnd = random.Random(0x1E70)
    _check(gpu_ctx, [_random_block(rnd, 4096) for _ in range(200)])
