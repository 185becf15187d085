"""The device zstd compressor (la_zstd_comp.hip) at the format's edges.  Every image goes through check_image of
test_gpu_zstd_compress.py (libzstd, the oracle, the device decoder, header shape) and through the plain reader
zstd_parse.py, whose own reconstruction must equal the input; every test then ends with a CENSUS read from the parsed
images alone: the exact sequence counts and header forms, code values, literals-section forms and stream end marks
that were written.  The inputs (zstd_edge_inputs.py) are designed to land on those edges; whether they did is never
assumed -- a census line that the images do not show fails with its name.

Two census lines the format itself rules out for this compressor, and which are therefore not asked: Offset_Code 17
and the offset value 2^17.  Offset_Value is offset + 3, a match starts at least four bytes before the end of a block
of at most 2^17 bytes and never reaches into an earlier block, so the largest value is 2^17 - 4 + 3 = 2^17 - 1, whose
code is 16.  That value is asked for.
"""
import random

import pytest

import test_gpu_zstd_compress as T
import zstd_build as B
import zstd_edge_inputs as E
import zstd_parse as P
import zstd_support as Z

pytestmark = pytest.mark.gpu

CHECKSUM = 1
BLOCK_MAX = 131072
UNIT_BLOCK = E.unit_stream(BLOCK_MAX)
DEVICE_DECODER = True       # (False on the bench: a compressor broken on purpose is judged by the host-side readers alone)


def _image(gpu_ctx, data, bs, bpf, deep=True):
    """compress, run every reader, return the parsed frames"""
    img = T.compress(gpu_ctx, data, bs, bpf, CHECKSUM)
    T.check_image(gpu_ctx, T._z(), Z.oracle_lib(), data, img, bs, bpf, CHECKSUM, device=DEVICE_DECODER)
    frames = P.parse(img, deep)
    if deep:
        assert P.plain_of(frames) == data, "the plain reader's reconstruction differs from the input"
    return frames


def _blocks(frames):
    return [b for f in frames for b in f["blocks"]]


def _report(missing):
    assert not missing, "census: " + "; ".join(missing)


# ---------------------------------------------------------------- sequence counts
def _nseq_of(gpu_ctx, data):
    fr = P.parse(T.compress(gpu_ctx, data, BLOCK_MAX, 1, CHECKSUM), deep=False)
    b = fr[0]["blocks"][0]
    return b["nseq"] if b["type"] == 2 else None


def _find_count(gpu_ctx, want, lo, hi):
    """the length (a multiple of 4 in [lo, hi]) at which the unit construction gives exactly `want` sequences: the
    count grows by at most one per unit, so a bisection on the cheap header walk finds it"""
    while lo < hi:
        mid = (lo + hi) // 8 * 4
        got = _nseq_of(gpu_ctx, UNIT_BLOCK[:mid])
        if got is None or got < want:
            lo = mid + 4
        else:
            hi = mid
    return lo


def test_sequence_counts_and_header_forms(gpu_ctx):
    rnd = random.Random(0x5E0)
    seen = {}
    skew = E.no_repeat(rnd, 400, range(12), [2 ** -(s / 2) for s in range(12)])
    b = _blocks(_image(gpu_ctx, skew, BLOCK_MAX, 1))[0]
    seen[b.get("nseq")] = (b["type"], b.get("nseq_form"), b["lit"]["type"] if b["type"] == 2 else None)
    for want in (127, 128, 0x7EFF, 0x7F00):
        n = _find_count(gpu_ctx, want, 4 * want, min(BLOCK_MAX, 4 * want + 1024))
        b = _blocks(_image(gpu_ctx, UNIT_BLOCK[:n], BLOCK_MAX, 1))[0]
        print("unit construction: %d bytes -> %s sequences" % (n, b.get("nseq")))
        if b["type"] == 2:
            seen[b["nseq"]] = (2, b["nseq_form"], b["lit"]["type"])
    missing = []
    if seen.get(0, (0,))[0] != 2 or seen[0][2] != 2:
        missing.append("no compressed block of 0 sequences with Huffman literals (saw %s)" % (seen.get(0),))
    for want, form in ((0, 1), (127, 1), (128, 2), (0x7EFF, 2), (0x7F00, 3)):
        if seen.get(want, (0, 0))[:2] != (2, form):
            missing.append("Number_of_Sequences %d in a %d-byte header not seen (saw %s)" % (want, form, sorted(seen)))
    _report(missing)


# ---------------------------------------------------------------- literal-length, match-length and offset codes
LL_TOP = {c: B.LL_BASE[c] + (1 << B.LL_BITS[c]) - 1 for c in range(16, 35)}
ML_TOP = {c: B.ML_BASE[c] + (1 << B.ML_BITS[c]) - 1 for c in range(32, 52)}


def _code_inputs():
    """[(data, block size)]"""
    rnd = random.Random(0xC0DE5)
    out = []
    small_ll = list(range(0, 64)) * 3
    small_ml = list(range(4, 131)) * 2
    rnd.shuffle(small_ll)
    rnd.shuffle(small_ml)
    # shuffled pairs (pack_pairs sorts: give it slices)
    blocks = []
    for k in range(0, len(small_ml), 32):
        blocks += E.pack_pairs(rnd, small_ll[k * 3 // 4:k * 3 // 4 + 24], small_ml[k:k + 32], 4096)
    out.append((b"".join(blocks), 4096))
    big_ll = [B.LL_BASE[c] for c in range(25, 36)] + [LL_TOP[c] for c in range(25, 35)]
    big_ml = [B.ML_BASE[c] for c in range(43, 53)] + [ML_TOP[c] for c in range(43, 52)]
    out.append((b"".join(E.pack_pairs(rnd, big_ll, big_ml, BLOCK_MAX)), BLOCK_MAX))
    near = [(1 << k) - 3 - d for k in range(3, 7) for d in (1, 0)]              # offsets 4, 5, 12, 13, 28, 29, 60, 61
    out.append((b"".join(E.lit_case(rnd, off, 256, range(256)) for off in near), 256))
    far = [(1 << k) - 3 - d for k in range(7, 17) for d in (1, 0)]
    out.append((b"".join(E.offset_gadgets(rnd, far, BLOCK_MAX) + [E.farthest_offset_block(rnd, BLOCK_MAX)]), BLOCK_MAX))
    return out


def code_census(blocks):
    ll, ml, ov = set(), set(), set()
    llc, mlc, ofc = set(), set(), set()
    for b in blocks:
        for s in (b.get("seqs") or []):
            ll.add(s[0]); ml.add(s[1]); ov.add(s[2]); llc.add(s[3]); mlc.add(s[4]); ofc.add(s[5])
    missing = []
    missing += ["LL code %d not seen" % c for c in range(36) if c not in llc]
    missing += ["ML code %d not seen" % c for c in range(1, 53) if c not in mlc]
    missing += ["OF code %d not seen" % c for c in range(2, 17) if c not in ofc]
    for c in range(16, 36):
        if B.LL_BASE[c] not in ll:
            missing.append("LL code %d lowest value %d not seen" % (c, B.LL_BASE[c]))
        if c < 35 and LL_TOP[c] not in ll:
            missing.append("LL code %d top value %d not seen" % (c, LL_TOP[c]))
    for c in range(32, 53):
        if B.ML_BASE[c] not in ml:
            missing.append("ML code %d lowest value %d not seen" % (c, B.ML_BASE[c]))
        if c < 52 and ML_TOP[c] not in ml:
            missing.append("ML code %d top value %d not seen" % (c, ML_TOP[c]))
    for k in range(3, 18):
        if (1 << k) - 1 not in ov:
            missing.append("offset value 2^%d - 1 not seen" % k)
        if k < 17 and 1 << k not in ov:
            missing.append("offset value 2^%d not seen" % k)
    return missing


def test_every_code_and_both_ends_of_its_extra_bits(gpu_ctx):
    blocks = []
    for data, bs in _code_inputs():
        nb = len(data) // bs
        for a in range(0, nb, 64):          # frames of at most 64 blocks
            part = data[a * bs:(a + 64) * bs]
            blocks += _blocks(_image(gpu_ctx, part, bs, len(part) // bs))
    assert all(b["type"] == 2 for b in blocks), [b["type"] for b in blocks]
    _report(code_census(blocks))


# ---------------------------------------------------------------- literals sections
def _literal_inputs():
    """({block size: [block]}, the two end-mark sweeps)"""
    rnd = random.Random(0x117)
    low = lambda k, skew=2.0: (range(k), [2 ** -(s / skew) for s in range(k)])
    high = range(129, 256)
    by = {}

    def add(size, n, symbols, weights=None):
        by.setdefault(size, []).append(E.lit_case(rnd, n, size, symbols, weights))

    add(256, 20, high)                                          # raw, 1-byte header
    add(256, 31, *low(4))                                       # 31: raw
    add(256, 32, *low(4))                                       # 32: Huffman, 3 weights
    add(256, 40, *low(5))                                       # 4 weights
    two = bytes([1, 1, 1, 0]) + bytes([0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0]) * 3 + bytes([0, 1, 0])
    by[256].append((two * 7)[:256])                             # two symbols, 40 literals: only position 0 can be a source
    add(1024, 200, range(128))                                  # flat: Huffman is not smaller
    add(1024, 200, high)                                        # raw, 2-byte header
    for n in (4095, 4096):
        add(8192, n, high)                                      # raw, 2- and 3-byte header
    for n in (1023, 1024):
        add(4096, n, *low(24, 3.0))                             # one stream / four streams
    for n in (16383, 16384):
        add(32768, n, *low(40, 8.0))                            # 4- and 5-byte header
    for top in (128, 129):                                      # largest symbol 128: header byte 255; 129: raw
        syms, w = low(12)
        add(4096, 900, list(syms) + [top], w + [0.05])
    # code lengths: 63 symbols of 129 (Shannon length 6 at up to 8256 literals), 66 that occur once (clamped to 11)
    counts = {s: 129 for s in range(63)}
    counts.update({s: 1 for s in range(63, 129)})
    for _ in range(20):
        blk = E.lit_block(E.exact_counts(rnd, counts), 16384)
        if blk is not None:
            break
    by[16384] = [blk]
    sweep_a = [E.lit_case(rnd, n, 512, *low(6)) for n in range(40, 104)]
    sweep_b = [E.lit_case(rnd, n, 4096, *low(16, 3.0)) for n in range(1024, 1088)]
    return by, sweep_a, sweep_b


def shannon_kraft(data):
    """2048 x the Kraft sum of the literals' Shannon code lengths ceil(log2(n / f)) clamped to [1, 11]"""
    n, k = len(data), 0
    for s in set(data):
        f, l = data.count(s), 0
        while (f << l) < n:
            l += 1
        k += 1 << (11 - min(max(l, 1), 11))
    return k


def literal_census(blocks, sweep_blocks):
    lits = [b["lit"] for b in blocks if b["type"] == 2]
    raw = [l for l in lits if l["type"] == 0]
    huf = [l for l in lits if l["type"] == 2]
    missing = []

    def want(what, cond):
        if not cond:
            missing.append(what + " not seen")

    for h in (1, 2, 3):
        want("raw literals with a %d-byte header" % h, any(l["hdr"] == h for l in raw))
    for h in (3, 4, 5):
        want("Huffman literals with a %d-byte header" % h, any(l["hdr"] == h for l in huf))
    want("31 literals written raw", any(l["regen"] == 31 for l in raw))
    want("32 literals Huffman-coded", any(l["regen"] == 32 for l in huf))
    want("1023 literals in one stream", any(l["regen"] == 1023 and l["streams"] == 1 for l in huf))
    want("1024 literals in four streams", any(l["regen"] == 1024 and l["streams"] == 4 for l in huf))
    want("4095 raw literals with a 2-byte header", any(l["regen"] == 4095 and l["hdr"] == 2 for l in raw))
    want("4096 raw literals with a 3-byte header", any(l["regen"] == 4096 and l["hdr"] == 3 for l in raw))
    want("16383 Huffman literals with a 4-byte header", any(l["regen"] == 16383 and l["hdr"] == 4 for l in huf))
    want("16384 Huffman literals with a 5-byte header", any(l["regen"] == 16384 and l["hdr"] == 5 for l in huf))
    want("largest symbol 128 with 128 weights written (header byte 255)", any(len(l["weights"]) == 128 for l in huf))
    want("largest symbol 129 written raw", any(max(l["data"]) == 129 and l["regen"] >= 32 for l in raw))
    want("an odd weight count", any(len(l["weights"]) % 2 == 1 for l in huf))
    want("an even weight count", any(len(l["weights"]) % 2 == 0 for l in huf))
    want("two symbols with one-bit codes", any(sorted(l["lengths"].values()) == [1, 1] for l in huf))
    want("code length 11 after Shannon lengths whose clamped Kraft sum exceeds 1",
         any(l["max_bits"] == 11 and shannon_kraft(l["data"]) > 2048 for l in huf))
    want("literals of bytes up to 128 left raw because Huffman was not smaller",
         any(l["regen"] >= 32 and max(l["data"]) <= 128 and len(set(l["data"])) > 1 for l in raw))
    counts = sorted(b["lit"]["regen"] for b in sweep_blocks if b["type"] == 2 and b["lit"]["type"] == 2)
    runs = [c for c in counts if all(c + d in counts for d in range(64))]
    want("64 consecutive literal counts in the end-mark sweep (saw %s)" % counts[:3], bool(runs))
    marks = [m for b in sweep_blocks if b["type"] == 2 and b["lit"]["type"] == 2 for m in b["lit"]["end_marks"]]
    for mod, r in ((32, 0), (32, 31), (8, 0), (8, 7)):
        want("a stream end mark on bit %d mod %d" % (r, mod), any(m % mod == r for m in marks))
    return missing


def test_literals_sections(gpu_ctx):
    by, sweep_a, sweep_b = _literal_inputs()
    blocks = []
    for size, blks in sorted(by.items()):
        blocks += _blocks(_image(gpu_ctx, b"".join(blks), size, len(blks)))
    sweep = _blocks(_image(gpu_ctx, b"".join(sweep_a), 512, 64)) + _blocks(_image(gpu_ctx, b"".join(sweep_b), 4096, 64))
    _report(literal_census(blocks + sweep, sweep))


# ---------------------------------------------------------------- frames
def test_frame_content_size_field_widths(gpu_ctx):
    rnd = random.Random(0xFC5)
    text = T._text(rnd, 70000)
    widths = {}
    for n, bs, bpf in ((255, 256, 1), (256, 256, 1), (65791, 16448, 4), (65792, 16448, 4)):
        assert bs * bpf >= n
        fr = _image(gpu_ctx, text[:n], bs, bpf)
        assert len(fr) == 1
        widths[n] = fr[0]["fcs_bytes"]
    fr = _image(gpu_ctx, text[:4 * 16448 + 1], 16448, 4)
    widths["tail"] = [f["fcs_bytes"] for f in fr]
    missing = []
    for n, w in ((255, 1), (256, 2), (65791, 2), (65792, 4), ("tail", [4, 1])):
        if widths[n] != w:
            missing.append("content size %s: field of %s bytes, not %s" % (n, widths[n], w))
    _report(missing)


# ---------------------------------------------------------------- every small length
def _patterns(n):
    rnd = random.Random(0x1E46)
    per67 = rnd.randbytes(67)
    norep = E.no_repeat(rnd, n, range(64))
    return {"period2": (b"ab" * n)[:n], "period5": (b"abcde" * n)[:n], "period67": (per67 * (n // 67 + 1))[:n], "norepeat": norep}


def test_every_small_length(gpu_ctx):
    z = T._z()
    lengths = list(range(1, 201)) + list(range(4090, 4101))
    pats = _patterns(4100)
    types = set()
    for name, text in sorted(pats.items()):
        for n in lengths:
            data = text[:n]
            img = T.compress(gpu_ctx, data, 4096, 2, CHECKSUM)
            assert Z.zstd_decompress(z, img, n + 16) == data, (name, n)
            fr = P.parse(img)
            assert P.plain_of(fr) == data, (name, n)
            assert len(fr) == 1 and len(fr[0]["blocks"]) == (2 if n > 4096 else 1)
            types |= {b["type"] for b in fr[0]["blocks"]}
    _report(["no block of type %d in the length sweep" % t for t in (0, 2) if t not in types])


# ---------------------------------------------------------------- neighbours in the workspace
def test_raw_rle_and_dense_blocks_side_by_side(gpu_ctx):
    rnd = random.Random(0xAB)
    parts = [rnd.randbytes(BLOCK_MAX), bytes([7]) * BLOCK_MAX, UNIT_BLOCK, bytes([9]) * BLOCK_MAX, UNIT_BLOCK, rnd.randbytes(BLOCK_MAX - 5)]
    blocks = _blocks(_image(gpu_ctx, b"".join(parts), BLOCK_MAX, 3, deep=False))     # (the round trip is the check here)
    got = [b["type"] for b in blocks]
    dense = [b["nseq"] for b in blocks if b["type"] == 2]
    missing = []
    if got != [0, 1, 2, 1, 2, 0]:
        missing.append("block types %s, not raw, RLE, compressed, RLE, compressed, raw" % got)
    if not dense or min(dense) < 0x7F00:
        missing.append("no 3-byte sequence count next to the raw and RLE blocks (counts %s)" % dense)
    _report(missing)


# ---------------------------------------------------------------- a compressed form larger than the block
def test_sequences_that_cost_more_than_they_save(gpu_ctx):
    """800 four-byte matches at offsets of 2^16 and more, each behind 64 literals that stay raw: a sequence costs 36
    bits (4 + 4 + 5 state bits, 6 literal-length bits, 16 offset bits, and one more behind the very long first run)
    and saves 32, so literals plus sequences come to about 350 bytes MORE than the block and past the 64 bytes of
    slack its workspace slot has: the sequence bit writer has to stop storing (its `over` path) and the block has to
    leave as a Raw_Block.  The image cannot show that the writer ran out of room, only that nothing else went wrong:
    the block is raw and the compressed blocks on either side of it in the workspace are intact."""
    rnd = random.Random(0xC057)
    text = T._text(rnd, BLOCK_MAX)
    blocks = _blocks(_image(gpu_ctx, text + E.costly_block(rnd) + text, BLOCK_MAX, 3))
    got = [b["type"] for b in blocks]
    _report([] if got == [2, 0, 2] else ["block types %s, not compressed, raw, compressed" % got])
