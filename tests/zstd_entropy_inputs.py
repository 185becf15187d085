"""Inputs for the tests of the zstd compressor's entropy flags (LA_ZSTDC_FULL_ALPHABET / LA_ZSTDC_FIT_TABLES) and of the
reader they take their census from (test infrastructure; see test_gpu_zstd_compress_entropy.py and
test_zstd_parse_modes.py).  Everything is seeded.  The builders that shape a block's sequences know how the block
matcher looks for matches (zstd_edge_inputs.py says how); they use that only to AIM: what a test asserts is read from
the image the device wrote.
"""
import random

import numpy as np

import zstd_edge_inputs as E


def text(rnd, n):
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 9))) for _ in range(400)]
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + rnd.choice([b" ", b" ", b" ", b", ", b".\n"])
    return bytes(out[:n])


def skewed256(rnd, n):
    """i.i.d. bytes min(255, int(Exp(0.03))): all 256 values occur, order-0 entropy about 6.5 bits"""
    return bytes(min(255, int(rnd.expovariate(0.03))) for _ in range(n))


def gaussian_f32(seed, n):
    return np.random.default_rng(seed).standard_normal(n // 4 + 1).astype("<f4").tobytes()[:n]


def utf8_text(rnd, n):
    """words over Latin, Greek and Cyrillic (two bytes a character) and CJK (three bytes) letters"""
    pools = ["abcdefghijklmnopqrstuvwxyz", "αβγδεζηθικλμνξοπρστυφχψω", "абвгдежзийклмнопрстуфхцчшщыэюя", "日本語漢字仮名交文章東京大阪京都山川田中"]
    words = []
    for _ in range(300):
        pool = rnd.choice(pools)
        words.append("".join(rnd.choice(pool) for _ in range(rnd.randint(1, 7))).encode("utf-8"))
    out = bytearray()
    while len(out) < n:
        out += rnd.choice(words) + rnd.choice([b" ", b" ", b", ", "。".encode("utf-8"), b"\n"])
    return bytes(out[:n])


def two_symbols(rnd, n, a=0x80, b=0xFF):
    """a and b at random, never four equal bytes in a row"""
    out = bytearray()
    while len(out) < n:
        c = rnd.choice((a, b))
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == c:
            c = a + b - c
        out.append(c)
    return bytes(out)


def alphabet(rnd, n, largest, present):
    """n bytes over `present` different values, the largest of them `largest`, geometrically skewed (every value occurs)"""
    syms = rnd.sample(range(largest), present - 1) + [largest]
    rnd.shuffle(syms)
    out = bytearray(syms)
    while len(out) < n:
        out.append(syms[min(present - 1, int(rnd.expovariate(6.0 / present)))])
    return bytes(out[:n])


def flat_permutations(rnd, n_symbols, rounds):
    """every value below n_symbols exactly `rounds` times (random permutations one after the other): Shannon code
    lengths are all equal, so are the weights a Huffman tree description would send"""
    out = bytearray()
    for _ in range(rounds):
        p = list(range(n_symbols))
        rnd.shuffle(p)
        out += bytes(p)
    return bytes(out)


def small_alphabet(rnd, n, k=8):
    """skewed bytes below k, no repeated four-byte string: a tree of so few weights is smallest in the direct form"""
    return E.no_repeat(rnd, n, list(range(k)), [2 * (k - i) for i in range(k)])


def rows(rnd, n, width=81):
    """Every byte repeats the one `width` (1 modulo 5) bytes before it, except every fifth, which is new and differs
    from it.  A new byte is carried along for five rows, one place further each row, so the only four-byte strings
    that occur twice are the four carried bytes in front of each new one: the matcher finds, unit after unit, one
    literal and a four-byte match `width` back (where the table slot still holds the source), and every sequence has
    the same match-length and offset code."""
    assert width % 5 == 1 and width >= 64
    out = bytearray(rnd.randbytes(width))
    while len(out) < n:
        above = out[len(out) - width]
        out.append(rnd.choice([b for b in range(256) if b != above]) if len(out) % 5 == 4 else above)
    return bytes(out[:n])


def flat_block(rnd, n_symbols, rounds, tail):
    """flat_permutations as a block's literals, then `tail` bytes that one match covers (lit_block), so that the
    block is a compressed one whatever its literals section becomes"""
    for _ in range(100):
        data = E.lit_block(flat_permutations(rnd, n_symbols, rounds), n_symbols * rounds + tail)
        if data is not None:
            return data
    raise AssertionError("no flat block")


def same_ll_code(rnd):
    """a block of four sequences whose literal lengths all have code 25 (64..127), with different match lengths; it
    ends with its last match"""
    sb = E.SeqBlock(rnd)
    sb.literals(64)
    sb.add(3, 70)
    for ll, ml in ((70, 10), (90, 13), (100, 24)):
        sb.add(ll, ml)
    return bytes(sb.out)


def few_sequences(rnd):
    """five sequences with five literal-length, match-length and (nearly) offset codes"""
    sb = E.SeqBlock(rnd)
    sb.literals(64)
    sb.add(3, 70)
    for ll, ml in ((1, 5), (9, 12), (20, 36), (40, 7)):
        sb.add(ll, ml)
    return sb.finish(600)


def many_sequences(rnd, n):
    """short repeats of 5..9 bytes at offsets below 200 between 0..3 literals: thousands of sequences in a block"""
    out = bytearray()
    while len(out) < n:
        out += rnd.randbytes(rnd.randint(0, 3))
        k = rnd.randint(5, 9)
        out += bytes(out[-k - rnd.randint(1, 200):][:k]) if len(out) > 300 else rnd.randbytes(k)
    return bytes(out[:n])


def entropy_inputs():
    """[(name, bytes)]: the data shapes and designed blocks of the entropy tests"""
    rnd = random.Random(0xE27)
    return [
        ("skewed256", skewed256(rnd, 150000)),
        ("gaussian_f32", gaussian_f32(11, 140000)),
        ("flat_random", rnd.randbytes(131072)),
        ("utf8_text", utf8_text(rnd, 150000)),
        ("two_symbols", two_symbols(rnd, 20000)),
        ("alphabet_129", alphabet(rnd, 30000, 129, 130)),
        ("alphabet_200", alphabet(rnd, 30000, 200, 150)),
        ("alphabet_255", alphabet(rnd, 30000, 255, 256)),
        ("flat_256", flat_block(random.Random(0xF256), 256, 12, 600)),
        ("flat_128", flat_block(random.Random(0xF128), 128, 24, 600)),
        ("small_alphabet", small_alphabet(random.Random(0x5A), 400)),
        ("rows", rows(random.Random(0x805), 131072)),
        ("same_ll_code", same_ll_code(random.Random(0x11C))),
        ("few_sequences", few_sequences(random.Random(0xFE5))),
        ("unit_stream", E.unit_stream(60000)),
        ("short_repeats", many_sequences(random.Random(0x5E9), 140000)),
    ]
