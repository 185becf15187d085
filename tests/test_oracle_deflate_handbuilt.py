"""Hand-built deflate streams (tests/deflate_build.py: a raw-deflate WRITER from RFC 1951, no zlib) against the image's
libz and the oracle.  The referee is inflate() behind inflateInit2(-15), the call the reference's gzip filter makes,
driven with the whole input and one large output buffer, and with the input in 7-byte pieces and 64 KiB output buffers
(how the filter meets it); both drives must answer alike.

* valid cases: zlib says "ok" and returns exactly the builder's plain bytes (the builder's model is never its own
  judge); the oracle returns rc 0, the same bytes and consumed == zlib's total_in;
* refused cases: the oracle's rc class is the one the case names, zlib agrees with the class ("data" / "more"), and the
  bytes the oracle produced in front of the error are zlib's total_out bytes and the model's prefix;
* name, sha256 of the image, sha256 of the plain or prefix bytes, zlib's verdict and msg, and consumed are kept in
  tests/golden/deflate_handbuilt.json (our own recorded data): a regenerated case that differs from the file fails.
  LA_DEFLATE_REGEN_GOLDEN=1 rewrites it."""
import hashlib
import json
import os

import pytest

import deflate_build as B
import deflate_support as Z
import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_handbuilt.json")
RC_OF = {B.ST_DATA: 2, B.ST_TRUNCATED: 1}
VERDICT_OF = {B.ST_DATA: "data", B.ST_TRUNCATED: "more"}


@pytest.fixture(scope="module")
def built():
    census = {}
    return B.handbuilt_cases(census), census


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_the_referee_is_the_zlib_the_design_names():
    assert Z.zlib_version() == "1.2.11"


def test_every_case_against_zlib_both_ways_and_the_oracle(built):
    cases, _ = built
    records = []
    for c in cases:
        whole = Z.zlib_inflate(c.image)
        pieces = Z.zlib_inflate(c.image, 7, 65536)
        assert whole == pieces, c.name
        verdict, total_in, out, msg = whole
        rc, cons, oout = O.inflate_raw(c.image, len(c.plain) + 64)
        if c.valid:
            assert (verdict, out) == ("ok", c.plain), (c.name, verdict, msg)
            assert (rc, oout, cons) == (0, c.plain, total_in), (c.name, rc, cons, total_in)
        else:
            assert verdict == VERDICT_OF[c.status], (c.name, verdict, msg)
            assert rc == RC_OF[c.status], (c.name, rc, verdict, msg)
            assert oout == out == c.plain, (c.name, len(oout), len(out), len(c.plain))
        records.append({"name": c.name, "image_sha256": _sha(c.image), "plain_sha256": _sha(c.plain), "valid": c.valid,
                        "zlib": verdict, "msg": msg, "consumed": total_in if c.valid else None})
    if os.environ.get("LA_DEFLATE_REGEN_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(records, f, indent=0)
            f.write("\n")
    assert json.load(open(GOLDEN)) == records


def test_where_we_are_stricter_than_zlib(built):
    """the refused-class cases zlib 1.2.11 accepts: none"""
    gold = json.load(open(GOLDEN))
    assert sorted(r["name"] for r in gold if not r["valid"] and r["zlib"] == "ok") == []
    assert sum(1 for r in gold if not r["valid"]) > 40


def test_every_prefix_of_six_streams(built):
    """six streams of about 400 bytes cut at EVERY byte: the oracle's verdict and bytes are zlib's for each prefix"""
    for name, blocks in B.prefix_streams():
        image, plain, valid, _, _ = B.build(blocks)
        assert valid and 200 <= len(image) <= 700, (name, len(image))
        for n in range(len(image) + 1):
            verdict, total_in, out, msg = Z.zlib_inflate(image[:n])
            assert Z.zlib_inflate(image[:n], 7, 65536) == (verdict, total_in, out, msg), (name, n)
            rc, cons, oout = O.inflate_raw(image[:n], len(plain) + 64)
            assert (rc, oout) == ({"ok": 0, "more": 1, "data": 2}[verdict], out), (name, n, rc, verdict, len(oout), len(out))
            assert verdict == ("ok" if n == len(image) else "more"), (name, n)
            if verdict == "ok":
                assert cons == total_in == n


def test_feature_census(built):
    """every feature the catalogue names was taken by at least one case (valid ones; refused classes by name)"""
    _, census = built
    print(sorted(census.items()))
    for key in B.CENSUS_KEYS:
        assert census.get(key, 0) > 0, key
