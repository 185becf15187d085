"""The plain zstd reader of the compressor tests (zstd_parse.py) against libzstd, on the CPU: frames from the
hand-written writer (zstd_build.py) restricted to what the device compressor can write, the writer's whole hand-built
set (the reader must either refuse a frame for a feature it does not support or regenerate exactly what libzstd does),
and libzstd's own level-1 output where that happens to use only those features."""
import random

import pytest

import zstd_build as B
import zstd_parse as P
import zstd_support as Z


def _z():
    z = Z.libzstd()
    if z is None:
        pytest.fail("no libzstd.so.1 in this image")
    return z


def _restricted_frames():
    """(name, blocks, frame keywords): direct weights, predefined tables, offset values above 3 only"""
    rnd = random.Random(0x9A45E)
    text = bytes(97 + min(int(rnd.expovariate(0.4)), 25) for _ in range(40000))
    low = bytes(min(int(rnd.expovariate(0.2)), 128) for _ in range(3000))
    out = []
    for n in (0, 1, 31, 32, 4095, 4096, 70000):
        out.append(("raw-literals-%d" % n, [B.Raw(B.HIST), B.Comp(B._bytes(rnd, n), [(0, 4, 3 + 9)] if n % 2 == 0 else [])], {}))
        out.append(("rle-literals-%d" % n, [B.Raw(B.HIST), B.Comp(b"r" * n, [(n, 5, 3 + 9)], lit=B.Lit("rle"))], {"checksum": True}))
    for n, streams, sf in ((40, 1, 0), (1023, 1, 0), (1024, 4, 2), (16383, 4, 2), (16384, 4, 3), (40000, 4, 3), (500, 4, 3)):
        out.append(("huf-%d-%d-streams" % (n, streams), [B.Comp(text[:n], [(5, 5, 3 + 3), (0, 7, 3 + 1)], lit=B.Lit("huf", streams=streams, sf=sf))], {}))
    for nsent in (1, 2, 3, 16, 127, 128):
        d = bytes(min(int(rnd.expovariate(3.0 / (nsent + 1))), nsent) for _ in range(40 * (nsent + 1))) + bytes(range(nsent + 1))
        w = B.huf_weights_for(d)
        assert len(w) == nsent + 1
        out.append(("huf-%d-weights" % nsent, [B.Comp(d, [(1, 4, 3 + 1)], lit=B.Lit("huf", weights=w, streams=4 if len(d) > 1023 else 1))], {}))
    out.append(("huf-two-symbols", [B.Comp(b"\x00\x01\x01\x00\x00\x00\x01\x00" * 9, [], lit=B.Lit("huf", streams=1))], {}))
    deep = b"".join(bytes([i]) * (1 if i == 0 else 1 << (i - 1)) for i in range(12))
    out.append(("huf-depth-11", [B.Comp(bytes(rnd.sample(list(deep), len(deep))), [(1, 4, 3 + 1)], lit=B.Lit("huf", streams=4))], {}))
    for n in (1, 64, 127, 128, 129, 0x7EFF, 0x7F00, 0x7F01):
        if n < 200:
            seqs = [(i % 3, 4 + i % 40, 3 + 1 + (i * 7) % 64) for i in range(n)]
        else:                                                          # (128 KiB hold no more than four bytes each)
            seqs = [(1 if i % 64 == 0 else 0, 4, 3 + 1 + (i * 7) % 64) for i in range(n)]
        out.append(("nseq-%d" % n, [B.Raw(B.HIST), B.Comp(low[:sum(s[0] for s in seqs) + 2], seqs)], {"window": (8, 0), "single": False}))
    # every LL / ML code at both ends of its extra bits, far offsets
    blocks = [B.Raw(B._bytes(rnd, B.BLOCK_MAX))]
    for c in range(16, 35):
        for ll in (B.LL_BASE[c], B.LL_BASE[c] + (1 << B.LL_BITS[c]) - 1):
            blocks.append(B.Comp(bytes([c]) * ll, [(ll, 4, 3 + 2 + c)], lit=B.Lit("rle")))
    for c in range(32, 52):
        for ml in (B.ML_BASE[c], B.ML_BASE[c] + (1 << B.ML_BITS[c]) - 1):
            blocks.append(B.Comp(b"", [(0, ml, 3 + min((1 << (c - 32)) * 7, 100000))]))
    blocks.append(B.Comp(b"w" * 65536, [(65536, 65536, 3 + 131068)], lit=B.Lit("rle")))
    blocks.append(B.Comp(low[:100], [(50, 65539, 3 + 65533), (50, 4, 3 + 65532)], lit=B.Lit("huf", streams=1)))
    out.append(("codes", blocks, {"window": (12, 0), "single": False, "checksum": True}))
    for n in (255, 256, 65791, 65792):
        out.append(("fcs-%d" % n, [B.Raw(B._bytes(rnd, min(n, 60000))), B.Rle(7, n - min(n, 60000))], {"single": True}))
    return out


RESTRICTED = _restricted_frames()


@pytest.mark.parametrize("name,blocks,kw", RESTRICTED, ids=[r[0] for r in RESTRICTED])
def test_restricted_writer_frames(name, blocks, kw):
    z = _z()
    census = {}
    img, plain = B.frame(blocks, census=census, **kw)
    assert Z.zstd_decompress(z, img, len(plain) + 16) == plain         # libzstd judges the writer
    fr = P.parse(img)
    assert len(fr) == 1 and fr[0]["plain"] == plain
    comps = [b for b in blocks if isinstance(b, B.Comp)]
    got = [b for b in fr[0]["blocks"] if b["type"] == 2]
    assert [b["nseq"] for b in got] == [len(c.seqs) for c in comps]
    for b, c in zip(got, comps):
        assert [s[:3] for s in b["seqs"]] == c.seqs and b["lit"]["data"] == c.literals
        assert all(B.LL_BASE[s[3]] <= s[0] and B.ML_BASE[s[4]] <= s[1] and 1 << s[5] <= s[2] < 2 << s[5] for s in b["seqs"])
        assert b["nseq_form"] == (1 if b["nseq"] < 128 else 2 if b["nseq"] < 0x7F00 else 3)
    assert fr[0]["fcs_bytes"] == [k for k in (0, 1, 2, 4, 8) if census.get("fcs_%d_bytes" % k)][0]
    shallow = P.parse(img, deep=False)[0]
    assert [(b["type"], b.get("nseq")) for b in shallow["blocks"]] == [(b["type"], b.get("nseq")) for b in fr[0]["blocks"]]


def test_literals_records():
    """header length, stream count and sizes, end-mark positions, weights and code lengths as the writer chose them"""
    lits = bytes([0, 1, 1, 0, 0, 0, 1, 0] * 5 + [1])                  # 41 one-bit codes: the end mark sits on bit 41
    img, _ = B.frame([B.Comp(lits, [], lit=B.Lit("huf", streams=1))])
    lit = P.parse(img)[0]["blocks"][0]["lit"]
    assert (lit["type"], lit["hdr"], lit["streams"], lit["regen"], lit["comp"]) == (2, 3, 1, 41, 2 + 6)
    assert lit["weights"] == [1] and lit["lengths"] == {0: 1, 1: 1} and lit["max_bits"] == 1
    assert lit["stream_sizes"] == [6] and lit["end_marks"] == [41]
    lits = bytes([0, 1] * 16 * 4 + [0, 1, 0])                         # four streams of 33, 33, 33 and 32 one-bit codes
    img, _ = B.frame([B.Comp(lits, [], lit=B.Lit("huf", streams=4, sf=2))])
    lit = P.parse(img)[0]["blocks"][0]["lit"]
    assert (lit["hdr"], lit["streams"], lit["stream_sizes"], lit["end_marks"]) == (4, 4, [5, 5, 5, 5], [33, 33, 33, 32])
    for n, hdr in ((31, 1), (32, 2), (4095, 2), (4096, 3)):
        img, _ = B.frame([B.Raw(B.HIST), B.Comp(bytes(n), [(n, 4, 3 + 60)], lit=B.Lit("rle"))])
        lit = P.parse(img)[0]["blocks"][1]["lit"]
        assert (lit["type"], lit["hdr"], lit["regen"]) == (1, hdr, n)


def test_handbuilt_set_refused_or_equal_to_libzstd():
    z = _z()
    parsed = refused = 0
    for c in B.handbuilt_cases():
        if not c.valid:
            continue
        try:
            fr = P.parse(c.image)
        except P.ParseError:
            refused += 1
            continue
        parsed += 1
        assert P.plain_of(fr) == c.plain == Z.zstd_decompress(z, c.image, len(c.plain) + 16), c.name
    assert parsed >= 150 and refused >= 50, (parsed, refused)         # both sides of the restriction are exercised


def test_libzstd_level_1_output_where_it_fits():
    z = _z()
    rnd = random.Random(0x11B)
    parsed = with_sequences = 0
    for it in range(400):
        n = rnd.choice([0, 1, 5, 20, 60, 200, 600, 2000])
        data = Z.gen(rnd, n, rnd.randint(0, 4))
        img = Z.zstd_compress(z, data, 1)
        try:
            fr = P.parse(img)
        except P.ParseError:
            continue
        parsed += 1
        with_sequences += any(b.get("nseq") for f in fr for b in f["blocks"])
        assert P.plain_of(fr) == data == Z.zstd_decompress(z, img, n + 16), it
    assert parsed >= 100, parsed
    print("libzstd level 1: %d of 400 images within the reader's features, %d of them with sequences" % (parsed, with_sequences))
