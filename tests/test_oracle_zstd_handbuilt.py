"""Hand-built Zstandard frames (tests/zstd_build.py: a frame WRITER from RFC 8878, no libzstd) against the image's
libzstd and the oracle.  The referee is ZSTD_decompressStream, the call the reference's filter makes, driven both with
the whole input at once and in small pieces (libzstd's one-shot shortcut inside the stream API is more lenient).

* valid cases: libzstd returns exactly the builder's plain bytes both ways (the builder's model is never its own
  judge), and the oracle agrees;
* invalid cases: the oracle refuses; libzstd's verdict (piece-wise drive) is recorded;
* name, sha256 of the image, sha256 of the plain bytes and libzstd's verdict are kept in tests/golden/zstd_handbuilt.json
  (our own recorded data): a regenerated case that differs from the file fails.  LA_ZSTD_REGEN_GOLDEN=1 rewrites it.

The census test counts the header features of the valid cases: every path that the compressor-made frames of
tests/test_gpu_zstd.py never or hardly ever take (direct weights, RLE literals, RLE / repeat table modes, 3-byte
sequence counts, 1-stream and treeless literals, window descriptors, 8-byte content sizes, checksums) is taken."""
import hashlib
import json
import os

import pytest

import zstd_build as B
import zstd_support as Z

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_handbuilt.json")


@pytest.fixture(scope="module")
def built():
    census = {}
    return B.handbuilt_cases(census), census


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_xxh64_in_python_known_answers():
    # the known answers of tests/test_oracle_zstd.py
    assert B.xxh64(b"") == 0xEF46DB3751D8E999
    assert B.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    assert B.xxh64(b"abc") == 0x44BC2CF5AD770999
    assert B.xxh64(b"Nobody inspects the spammish repetition") == 0xFBCEA83C8A378BF1
    o = Z.oracle_lib()
    for n in (31, 32, 33, 63, 64, 100, 4099):
        d = bytes((i * 131 + 7) & 0xFF for i in range(n))
        assert B.xxh64(d) == o.orc_xxh64(d, n, 0)


def test_every_case_against_libzstd_stream_and_the_oracle(built):
    cases, _ = built
    z = Z.libzstd()
    assert z is not None, "libzstd.so.1 is the referee of this test"
    o = Z.oracle_lib()
    records = []
    for c in cases:
        piece = 7 if len(c.image) < 5000 else 4093
        whole, pieces = Z.zstd_stream_decompress(z, c.image), Z.zstd_stream_decompress(z, c.image, piece)
        rc, out, msg = Z.oracle_decode(o, c.image, (len(c.plain) if c.valid else 1 << 18) + 16)
        if c.valid:
            assert whole == (c.plain, "ok") and pieces == (c.plain, "ok"), (c.name, whole[1], pieces[1])
            assert (rc, out, msg) == (0, c.plain, ""), c.name
        else:
            # the oracle refuses, and for the reason the case is built for: "Truncated zstd input" is status 12, every
            # other status is a format error; a cut frame is whichever of the two libzstd calls it
            assert rc == -30, c.name
            if c.status is None:
                assert pieces[1] != "ok", c.name
                want = "Truncated zstd input" if pieces[1] == "Truncated zstd input" else "Zstd decompression failed"
            else:
                want = "Truncated zstd input" if c.status == B.ST_TRUNCATED else "Zstd decompression failed"
            assert msg == want, (c.name, msg, pieces[1])
        records.append({"name": c.name, "image_sha256": _sha(c.image), "plain_sha256": _sha(c.plain) if c.valid else None,
                        "libzstd": pieces[1]})
    if os.environ.get("LA_ZSTD_REGEN_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(records, f, indent=0)
            f.write("\n")
    assert json.load(open(GOLDEN)) == records


def test_where_we_are_stricter_than_libzstd(built):
    """the divergence table of DESIGN.md: the only invalid-class cases libzstd 1.4.8 accepts"""
    gold = {r["name"]: r for r in json.load(open(GOLDEN))}
    accepted = sorted(n for n, r in gold.items() if r["plain_sha256"] is None and r["libzstd"] == "ok")
    assert accepted == ["bad-repeat-offset-1-minus-1", "bad-sequence-bits-left-over",
                        "bad-zero-sequences-in-2-byte-form-with-modes-byte"]


def test_header_feature_census(built):
    _, census = built
    print(sorted(census.items()))
    for key in ("huf_direct", "lit_rle_sf0", "lit_rle_sf1", "lit_rle_sf2", "lit_rle_sf3", "of_rle", "ll_rle", "ml_rle", "ll_repeat", "of_repeat",
                "ml_repeat", "nseq_form3", "huf_1stream", "lit_treeless", "window_descriptor", "fcs_8_bytes", "checksum",
                "huf_fse", "huf_4streams", "lit_huf_sf1", "lit_huf_sf2", "lit_huf_sf3", "ll_fse", "of_fse", "ml_fse"):
        assert census.get(key, 0) > 0, key
