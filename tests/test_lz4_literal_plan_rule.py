"""The literal plan of the lz4 window path without a GPU: the rule of la_dev.h (la_lz4_lit_chunk_edge) restated in
lz4_literal_plan_rule.py, applied to generated blocks.  Literals placed from the plan as whole dwords with their spill,
then the matches in order, give the generator's bytes; no payload dword is stored for two runs; a block's plan fits the
bytes its table slot leaves it, for every payload length the format allows."""
import random
import struct

import lz4_literal_plan_rule as R


def _varlen(n):
    return b"\xff" * (n // 255) + bytes([n % 255])


def _block(seqs, tail):
    """(literals, offset, match length >= 4) sequences and the closing literals -> (encoded, decoded)"""
    enc, out = bytearray(), bytearray()
    for lit, off, mlen in seqs + [(tail, 0, 0)]:
        ll, ml = len(lit), mlen - 4
        enc.append((min(ll, 15) << 4) | (min(ml, 15) if off else 0))
        if ll >= 15:
            enc += _varlen(ll - 15)
        enc += lit
        out += lit
        if off:
            assert 1 <= off <= len(out) and mlen >= 4
            enc += struct.pack("<H", off)
            if ml >= 15:
                enc += _varlen(ml - 15)
            for _ in range(mlen):
                out.append(out[-off])
    return bytes(enc), bytes(out)


def _random_block(rnd, size, max_lit):
    seqs, n = [], 0
    while n < size:
        ll = rnd.choice((0, 0, 1, 2, 3, 5, 9, 15, 16, 31, 33, rnd.randint(0, max_lit)))
        if n == 0 and ll == 0:
            ll = 1
        n += ll
        seqs.append((rnd.randbytes(ll), rnd.randint(1, n), rnd.randint(4, 40)))
        n += seqs[-1][2]
    return _block(seqs, rnd.randbytes(rnd.randint(5, 40)))


def _apply(enc, plain):
    ent, olen = R.parse_block(enc)
    assert olen == len(plain)
    plan = R.rule_plan(ent, len(enc))
    assert len(plan) == R.plan_entries(len(enc))
    win, stored = R.place_literals(plan, ent, enc, olen)
    assert max(stored, default=0) <= 1
    assert R.copy_matches(win, ent, olen) == plain
    return ent, plan, stored


def test_plan_reproduces_generated_blocks():
    """300 random blocks: literal runs of 0 .. 1 200 bytes, zero-length runs in a row, matches of 4 .. 40 bytes"""
    rnd = random.Random(0x11A0)
    for i in range(300):
        enc, plain = _random_block(rnd, rnd.randint(1, 6000), (8, 70, 300, 1200)[i % 4])
        ent, plan, stored = _apply(enc, plain)
        lit_dwords = set()
        for e in ent:
            ls, ll, _, _ = R.fields(e)
            lit_dwords.update(range(ls >> 2, (ls + ll + 3) >> 2) if ll else ())
        assert {p for p, n in enumerate(stored) if n} == lit_dwords     # every dword that meets a run, and no other


def test_entries_are_the_first_sequence_with_literals_behind_the_chunk_start():
    """the entries against the definition, sequence by sequence; NONE only behind the last literal byte"""
    rnd = random.Random(0x11A1)
    for _ in range(50):
        enc, plain = _random_block(rnd, 3000, 100)
        ent, plan, _ = _apply(enc, plain)
        ends = [R.fields(e)[0] + R.fields(e)[1] for e in ent]
        assert ends[-1] == len(enc) and plan[-1] == R.chunk_edge(len(enc))
        for c, k in enumerate(plan[:-1]):
            assert k != R.NONE and ends[k] > 32 * c and (k == 0 or ends[k - 1] <= 32 * c)


def test_chunks_behind_the_last_literal_have_no_entry():
    """a table whose literals end short of the payload (the rule is stated over entries, whoever made them)"""
    ent = [0 | 10 << 16 | 0 << 32 | 4 << 48, 13 | 40 << 16 | 18 << 32]
    plan = R.rule_plan(ent, 200)
    assert plan == [0, 1, R.NONE, R.NONE, R.NONE, R.NONE, R.NONE, 2]


def test_edges():
    """one sequence; two; a first run at payload offsets 1, 2 and 3; runs that end 0 .. 3 bytes short of, on and past a
    chunk edge; eight sequences of no or one literal inside one chunk; a run of 60 000 bytes; a block of 65 536 bytes
    whose closing literals reach the last byte"""
    rnd = random.Random(0x11A2)
    _apply(*_block([], rnd.randbytes(7)))
    _apply(*_block([(b"abcd", 2, 8)], rnd.randbytes(5)))
    for ll in (1, 14, 15 + 254, 15 + 255):      # token, then 0, 1 or 2 length bytes in front of the first literal
        enc, plain = _block([(rnd.randbytes(ll), 1, 4)], rnd.randbytes(5))
        ent, _, _ = _apply(enc, plain)
        assert R.fields(ent[0])[0] == (1, 1, 2, 3)[(1, 14, 269, 270).index(ll)]
    for short in range(-3, 4):
        for start in range(0, 8):
            seqs = [(rnd.randbytes(start + 1), 1, 4)]
            used = len(_block(seqs, b"")[0]) - 1        # payload bytes in front of the next token
            seqs.append((rnd.randbytes(max(0, 64 - short - used - 1)), 3, 5))
            _apply(*_block(seqs, rnd.randbytes(6)))
    tiny = [(rnd.randbytes(40), 7, 4)] + [(rnd.randbytes(i & 1), 5, 4) for i in range(8)]
    ent, plan, _ = _apply(*_block(tiny, rnd.randbytes(9)))
    assert plan[2] >= 6     # the chunk behind them starts at the seventh sequence or later
    _apply(*_block([(rnd.randbytes(60000), 100, 12)], rnd.randbytes(20)))
    enc, plain = _block([(rnd.randbytes(4), 2, 28)] * 1000, rnd.randbytes(65536 - 32000))
    assert len(plain) == 65536
    _apply(enc, plain)


def test_plan_fits_the_slot():
    """16-bit entries, one byte of plan buffer per table slot entry; a chunk count has 12 bits"""
    for src_len in range(0, 65536 + 1):
        assert 2 * R.plan_entries(src_len) <= R.slot_entries(src_len), src_len
    assert R.plan_entries(65536) == 2049 and R.slot_entries(0) == 8
