"""The dword-wise literal placement of the lz4 window kernel without a GPU: the owner rule of la_dev.h
(la_lz4_lit_run_dwords) restated in lz4_literal_dword_rule.py, applied to generated blocks chunk by chunk from the
literal plan.  Every payload dword has at most one owner; the stores of the dword-wise form are, as a set of (window
offset, payload dword) pairs, those of the run-wise form; and those stores, then the matches in order, give the
generator's bytes."""
import random

import lz4_literal_dword_rule as D
import lz4_literal_plan_rule as R
from test_lz4_literal_plan_rule import _block, _random_block


def _apply(enc, plain):
    ent, olen = R.parse_block(enc)
    assert olen == len(plain)
    plan = R.rule_plan(ent, len(enc))
    stores, most = [], 0
    for c in range(R.chunk_edge(len(enc))):
        if plan[c] == R.NONE:
            continue
        by_dword, claims = D.stores_by_dword(ent, plan[c], 32 * c)
        by_run = D.stores_by_run(ent, plan[c], 32 * c)
        assert max(claims) <= 1, (c, claims)                            # at most one owner
        assert len(by_dword) == len(set(by_dword)) == len(by_run)       # nothing stored twice
        assert set(by_dword) == set(by_run), (c, by_dword, by_run)      # the same stores either way
        stores += by_dword
        most = max(most, sum(1 for e in ent[plan[c]:] if 32 * c <= R.fields(e)[0] < 32 * c + 32))
    assert R.copy_matches(D.place(stores, enc, olen), ent, olen) == plain
    want, stored = R.place_literals(plan, ent, enc, olen)               # and the window the plan's own interpreter makes
    assert D.place(stores, enc, olen)[:len(want)] == want and max(stored, default=0) <= 1
    return ent, plan, most


def test_rule_against_its_definition():
    """every run position and length around one chunk: the dwords are those that hold a byte of the run, and dword m
    lies where its first byte's output position says"""
    for c0 in (0, 32, 4096):
        for ls in range(max(0, c0 - 40), c0 + 40):
            for ll in range(0, 75):
                r = D.run_dwords(ls, ls + ll, 1000, c0)
                hold = [m for m in range(8) if any(ls <= c0 + 4 * m + i < ls + ll for i in range(4))]
                if not hold:
                    assert r is None
                    continue
                assert list(range(r[0], r[1])) == hold
                assert all(r[2] + 4 * m == 1000 + (c0 + 4 * m - ls) for m in hold) and r[2] + 4 * hold[0] >= 1000 - 3


def test_generated_blocks():
    """300 random blocks: literal runs of 0 .. 1 200 bytes, zero-length runs in a row, matches of 4 .. 40 bytes"""
    rnd = random.Random(0x1E00)
    most = 0
    for i in range(300):
        enc, plain = _random_block(rnd, rnd.randint(1, 6000), (8, 70, 300, 1200)[i % 4])
        most = max(most, _apply(enc, plain)[2])
    assert most > D.RUNS_AT_ONCE      # some chunk went on run by run behind its sixth sequence


def test_hand_cases():
    """runs of 0 .. 9, 15, 16 and 270 bytes on every payload offset mod 32; 1 .. 9 sequences starting in one chunk; first
    runs at payload offsets 1, 2 and 3; blocks of one and two sequences; a last chunk of 1 .. 31 bytes; a payload above
    32 KiB; a block of 65 536 bytes closed by literals"""
    rnd = random.Random(0x1E01)
    for ll in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 270):
        for fill in range(40):
            seqs = [(rnd.randbytes(fill + 1), 1, 4), (rnd.randbytes(ll), rnd.randint(1, fill + 5), rnd.randint(4, 9)),
                    (rnd.randbytes(3), 2, 5)]
            _apply(*_block(seqs, rnd.randbytes(6)))
    for count in range(1, 10):
        tiny = [(rnd.randbytes(30), 7, 4)] + [(rnd.randbytes(i & 1), 5, 4) for i in range(count)] + [(rnd.randbytes(33), 9, 6)]
        ent, plan, most = _apply(*_block(tiny, rnd.randbytes(9)))
        assert most >= count
    for ll in (14, 269, 270):       # token, then 0, 1 or 2 length bytes in front of the first literal
        ent, _, _ = _apply(*_block([(rnd.randbytes(ll), 1, 4)], rnd.randbytes(5)))
        assert R.fields(ent[0])[0] == (1, 2, 3)[(14, 269, 270).index(ll)]
    _apply(*_block([], rnd.randbytes(7)))
    _apply(*_block([(b"abcd", 2, 8)], rnd.randbytes(5)))
    for want in range(65, 98):
        enc, plain = _block([(rnd.randbytes(8), 3, 4)], rnd.randbytes(want - 13))
        assert len(enc) == want
        _apply(enc, plain)
    enc, plain = _block([(rnd.randbytes(14), rnd.randint(1, 14), 4) for _ in range(1950)], rnd.randbytes(50))
    assert len(enc) > 32768 + 64 and len(plain) <= 65536
    _apply(enc, plain)
    enc, plain = _block([(rnd.randbytes(4), 2, 28)] * 1000, rnd.randbytes(65536 - 32000))
    assert len(plain) == 65536
    _apply(enc, plain)
