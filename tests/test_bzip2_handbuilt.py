"""Hand-built bzip2 streams (tests/bzip2_build.py: a bzip2 WRITER from the format, no libbz2) against the image's libbz2
and the reference's read loop over it.  The referee is BZ2_bzDecompress behind BZ2_bzDecompressInit(0, 0), the calls the
reference's bzip2 filter makes, driven with the whole input and one output buffer larger than the plain, and with the
input in 7-byte pieces and 64 KiB output buffers; both drives must answer alike.

* valid cases: libbz2 says "ok" and returns exactly the builder's plain bytes (the builder's model is never its own
  judge);
* refused cases: libbz2's class is the one the case names ("data" for a data or CRC error, "more" for a cut stream) and
  the bytes it wrote in front of the error are the model's prefix;
* a block that ends on four equal bytes with no count: see the comment in the test;
* name, sha256 of the image, sha256 and length of libbz2's bytes (and of what it wrote unreported, for the missing count), its verdict, total_in for valid cases and what
  bzip2_support.reference_cat gives (length, sha256, rc, message) are kept in tests/golden/bzip2_handbuilt.json (our own
  recorded data): a regenerated case that differs from the file fails.  LA_BZIP2_REGEN_GOLDEN=1 rewrites it.
* every case through la_api.cat over the CPU stand-in for the device (mock_build.host_lib()) equals reference_cat.

libbz2 1.0.8 reads and drops the selectors beyond 18002; older versions refuse them.  The device decoder copies 1.0.8."""
import ctypes as C
import hashlib
import json
import os

import pytest

import bzip2_build as B
import bzip2_support as BS
import la_api
import mock_build

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bzip2_handbuilt.json")
VERDICT_OF = {"ok": "ok", "data": "data", "crc": "data", "truncated": "more"}
BZ_OK, BZ_STREAM_END = 0, 4


def libbz2_drive(image, in_piece=None, out_piece=None, out_cap=1 << 20, peek=None):
    """(verdict, total_in, bytes written): verdict "ok" at BZ_STREAM_END, "data" for every refusal, "more" when libbz2
    has taken all input and asks for more.  in_piece / out_piece None: the whole input, one buffer of out_cap bytes.
    peek (whole-input drive): the buffer's first `peek` bytes in place of what libbz2 reported as written."""
    lib = BS.libbz2()
    image = bytes(image)
    src = C.create_string_buffer(image, max(len(image), 1))
    osize = out_piece or out_cap
    obuf = C.create_string_buffer(osize)
    strm = BS._BzStream()
    assert lib.BZ2_bzDecompressInit(C.byref(strm), 0, 0) == BZ_OK
    out, pos, step = bytearray(), 0, in_piece or max(len(image), 1)
    try:
        while True:
            if strm.avail_in == 0 and pos < len(image):
                k = min(step, len(image) - pos)
                strm.next_in, strm.avail_in = C.addressof(src) + pos, k
                pos += k
            if strm.avail_out == 0:     # a buffer is handed on when it is full, as the reference's read loop does
                strm.next_out, strm.avail_out = C.addressof(obuf), osize
            ret = lib.BZ2_bzDecompress(C.byref(strm))
            if strm.avail_out == 0 or ret != BZ_OK or (strm.avail_in == 0 and pos == len(image)):
                out += obuf.raw[:osize - strm.avail_out]
            if ret == BZ_STREAM_END:
                verdict = "ok"
                break
            if ret != BZ_OK:
                verdict = "data"
                break
            if strm.avail_in == 0 and pos == len(image) and strm.avail_out > 0:
                verdict = "more"
                break
            if strm.avail_in == 0 and pos == len(image):
                strm.avail_out = 0      # (collected above: a fresh buffer for what libbz2 still holds)
            assert out_piece or strm.avail_out > 0, "the whole-input drive needs a larger output buffer"
        return verdict, strm.total_in_lo32, bytes(out) if peek is None else obuf.raw[:peek]
    finally:
        lib.BZ2_bzDecompressEnd(C.byref(strm))


@pytest.fixture(scope="module")
def built():
    census = {}
    return B.handbuilt_cases(census), census


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def test_the_referee_is_the_libbz2_the_design_names():
    assert BS.libbz2().BZ2_bzlibVersion().decode().split(",")[0] == "1.0.8"


def test_every_case_against_libbz2_both_ways_and_the_read_loop(built):
    cases, _ = built
    records = []
    for c in cases:
        whole = libbz2_drive(c.image, out_cap=len(c.plain) + (1 << 16))
        pieces = libbz2_drive(c.image, 7, 65536)
        verdict, total_in, out = whole
        assert verdict == VERDICT_OF[c.cls], (c.name, verdict)
        if c.end_run:
            # libbz2 writes the run it makes up behind four equal bytes and then returns the error WITHOUT updating
            # next_out / avail_out: the bytes are in the buffer, unreported, unless the buffer filled up inside the
            # run.  So the whole-input drive reports the blocks in front only, the other one up to its last full buffer,
            # and the model (which the device has to deliver, since the reference may hand the run out) is held to the
            # buffer's content.
            front = b"".join([c.plain])[:len(out)]
            assert out == front and len(out) < len(c.plain), c.name
            assert pieces[:2] == whole[:2] and pieces[2] == c.plain[:max(len(out), len(c.plain) & ~0xFFFF)], c.name
            written = libbz2_drive(c.image, out_cap=len(c.plain) + (1 << 16), peek=len(c.plain) + 8)[2]
            assert written == c.plain + bytes(8), c.name
        else:
            assert whole == pieces, c.name
            assert out == c.plain, (c.name, len(out), len(c.plain))
        if c.valid:
            assert total_in == len(c.image), c.name
        assert BS.find_magics(c.image)[0] == (32, 0) and set(c.marks) <= set(BS.find_magics(c.image)), c.name
        data, rc, msg = BS.reference_cat(c.image)
        if c.valid:
            assert (data, rc, msg) == (c.plain, 0, ""), c.name
        else:       # the read loop hands out whole 64 KiB blocks in front of an error
            want = "truncated bzip2 input" if c.cls == "truncated" else "bzip decompression failed"
            assert (rc, msg) == (BS.ARCHIVE_FATAL, want) and data == c.plain[:len(c.plain) & ~0xFFFF], c.name
        records.append({"name": c.name, "image_sha256": _sha(c.image), "out_sha256": _sha(out), "out_len": len(out), "valid": c.valid,
                        "libbz2": verdict, "total_in": total_in if c.valid else None, "reference_cat": [len(data), _sha(data), rc, msg],
                        "written_sha256": _sha(c.plain) if c.end_run else None})
    if os.environ.get("LA_BZIP2_REGEN_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(records, f, indent=0)
            f.write("\n")
    assert json.load(open(GOLDEN)) == records


def test_where_we_are_stricter_than_libbz2(built):
    """the refused-class cases libbz2 1.0.8 accepts: none"""
    gold = json.load(open(GOLDEN))
    assert sorted(r["name"] for r in gold if not r["valid"] and r["libbz2"] == "ok") == []
    assert len(gold) >= 70 and sum(1 for r in gold if not r["valid"]) >= 25


def test_the_made_up_run_is_handed_out(built):
    """the missing count behind a first block: the reference's first 64 KiB block ends inside the run libbz2 makes up"""
    cases, _ = built
    c = {c.name: c for c in cases}["missing-count-made-up-run-crosses-64k"]
    data, rc, msg = BS.reference_cat(c.image)
    assert len(data) == 65536 and data[65520:65527] == b"abcXXXX" and data[65527:] == b"X" * 9 and rc == BS.ARCHIVE_FATAL


def test_feature_census(built):
    """every feature the catalogue names was taken by at least one case: what the writer saw itself write in a valid
    stream, and what a case states for itself"""
    _, census = built
    print(sorted(census.items()))
    for key in B.CENSUS_KEYS:
        assert census.get(key, 0) > 0, key


def test_false_magics_are_listed(built):
    """the planted magics are real candidates: find_magics lists them beside the stream's own"""
    cases, _ = built
    n = 0
    for c in cases:
        if c.name.startswith("false-"):
            extra = [m for m in BS.find_magics(c.image) if m not in c.marks]
            assert len(extra) == (1 if "crc" in c.name else 2) and c.valid, c.name
            n += 1
            if "phase" in c.name:
                assert extra[0][1] == 0 and extra[1] == (extra[0][0] + 48, 1), c.name
    phases = {[m for m in BS.find_magics(c.image) if m not in c.marks][0][0] % 8 for c in cases if "block-follows" in c.name}
    assert n == 17 and phases == set(range(8))


def test_every_prefix_of_the_prefix_stream():
    image, plains, marks = B.prefix_stream()
    plain = b"".join(plains)
    assert 250 <= len(image) <= 500 and len(BS.find_magics(image)) == len(marks) + 1 == 4
    lengths = []
    for n in range(len(image) + 1):
        verdict, total_in, out = libbz2_drive(image[:n])
        assert libbz2_drive(image[:n], 7, 65536) == (verdict, total_in, out), n
        assert verdict == ("ok" if n == len(image) else "more") and total_in == n, n
        assert plain.startswith(out), n
        if n >= 14:     # what the device test expects of the filter: nothing in front of a cut, under 64 KiB as this is
            assert BS.reference_cat(image[:n]) == ((plain, 0, "") if n == len(image) else (b"", BS.ARCHIVE_FATAL, "truncated bzip2 input")), n
        lengths.append(len(out))
    # block by block: a block's bytes come when its last bit is there (the next magic starts behind it)
    assert lengths == [0 if 8 * n < marks[1][0] else len(plains[0]) if 8 * n < marks[2][0] else len(plain) for n in range(len(image) + 1)]


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_host_filter_over_the_mock(mock, built, read_size):
    """the host filter's handling of real false candidates, of the candidate table and of every refusal: la_api.cat over
    the CPU stand-in equals the reference's read loop, bytes, return code and message.  (Every cut case cuts a block that
    starts at a byte: the stand-in feeds libbz2 whole bytes, so the last, partial byte of a cut block that starts inside
    a byte is padded, and libbz2 may refuse the padding as data.  Cuts of such blocks are the device test's.)"""
    cases, _ = built
    for c in cases:
        ref = BS.reference_cat(c.image, read_size)
        got = la_api.as_reference_tuple(la_api.cat(c.image, read_size=read_size))
        assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2]), c.name
        assert got[0] == ref[0], c.name
