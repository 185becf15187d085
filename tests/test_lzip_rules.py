"""The lzip decode rules (libarchive_amd/csrc/la_lzip_dev.h over la_xz_dev.h's symbol loop, compiled for the host by
tests/mock_gpu/la_gpu_lzip_mock.c) against liblzma's raw LZMA1 decoder on hand-built streams: bytes, verdict and the bytes consumed
through the marker.  Then what the entry's tentative ends add: each has its own status."""
import zlib

import pytest

import lzip_support as LS
import mock_build

NAMES = {v: k for k, v in LS.ST.items()}


@pytest.fixture(scope="module")
def lib():
    return mock_build.gpu_lib()


def entry(raw, db, cap, src_end=LS.UNKNOWN, data_size=LS.UNKNOWN, crc=None, src_off=0, dst_off=0):
    return LS.Member(src_off, src_end, data_size, dst_off, cap, LS.dict_size(db), crc or 0, LS.HAS_CRC if crc is not None else 0, 0)


def test_the_cases_hold_what_their_names_say():
    cases = LS.stream_cases()
    verdict = lambda n: LS.expected_stream_result(*cases[n], 1 << 20)[0]      # noqa: E731
    assert len(LS.liblzma_raw(*cases["match_273"])[0]) == 3 + 273 + 2
    for n in ("match_273", "all_reps", "dict_4096_equal", "distance_equal_to_the_data", "marker_len_5", "marker_len_273", "empty", "good",
              "bytes_behind_the_marker"):
        assert verdict(n) == "OK", n
    for n in ("short_rep_at_0", "rep_at_0", "dict_4096_one_past", "distance_past_the_data", "first_init_byte_1", "first_init_byte_255",
              "marker_code_1", "marker_code_128"):
        assert verdict(n) == "DATA", n
    assert verdict("no_marker") == "TRUNCATED"
    assert LS.liblzma_raw(*cases["bytes_behind_the_marker"])[2] == len(cases["good"][0])
    cuts = [n for n in cases if n.startswith("cut_")]
    assert len(cuts) >= 20 and all(verdict(n) == "TRUNCATED" for n in cuts)
    assert {n.split("_")[1] for n in cuts} == {"literal", "match", "far", "rep", "short", "marker"}


@pytest.mark.parametrize("name", sorted(LS.stream_cases()))
def test_stream_against_liblzma(lib, name):
    raw, db = LS.stream_cases()[name]
    plain = LS.liblzma_raw(raw, db)[0]
    caps = {1 << 16, len(plain)} | ({len(plain) - 1, 1} if len(plain) > 1 else set())
    for cap in sorted(caps):
        exp = LS.expected_stream_result(raw, db, cap)
        (r, out), = LS.mock_decode(lib, raw, [entry(raw, db, cap)], cap)
        got = (NAMES[r.status], out, r.consumed if r.status == 0 else None)
        if cap == len(plain) and exp[0] == "TRUNCATED":
            # the output is full where the input ends: which of the two a decoder meets first is its own business
            assert got[0] in ("TRUNCATED", "OUT_FULL") and got[1] == exp[1], (name, cap)
            continue
        assert got == exp, (name, cap, got[0], exp[0])
        assert r.valid == r.out_len == len(out) and r.crc32 == zlib.crc32(out)


def test_tentative_ends_each_have_their_status(lib):
    raw, db = LS.stream_cases()["good"]
    plain, _, used = LS.liblzma_raw(raw, db)
    src = raw + bytes(40)
    run = lambda **kw: LS.mock_decode(lib, src, [entry(raw, db, kw.pop("cap", 100), **kw)], 100)[0]      # noqa: E731
    st = lambda r: NAMES[r[0].status]      # noqa: E731
    r = run(src_end=used, data_size=len(plain), cap=len(plain), crc=zlib.crc32(plain))
    assert st(r) == "OK" and r[1] == plain and r[0].consumed == used
    assert st(run(src_end=used - 1)) == "SRC_END"
    assert st(run(src_end=used + 1)) == "EARLY_END"
    assert st(run(src_end=5)) == "SRC_END" and st(run(src_end=0)) == "SRC_END"
    r = run(data_size=len(plain) - 1)
    assert st(r) == "SIZE_OVER" and r[1] == plain[:-1]
    r = run(data_size=len(plain) + 1)
    assert st(r) == "BAD_SIZE" and r[1] == plain
    r = run(cap=len(plain) - 1)
    assert st(r) == "OUT_FULL" and r[1] == plain[:-1]
    assert st(run()) == "OK" and st(run(cap=len(plain))) == "OK"
    r = run(crc=zlib.crc32(plain) ^ 1)
    assert st(r) == "BAD_CRC" and r[0].crc32 == zlib.crc32(plain) and r[1] == plain
    assert st(LS.mock_decode(lib, raw[:-1], [entry(raw, db, 100)], 100)[0]) == "TRUNCATED"
    # a match that meets the tentative size is copied up to it
    raw2, db2 = LS.stream_cases()["match_273"]
    plain2 = LS.liblzma_raw(raw2, db2)[0]
    r = LS.mock_decode(lib, raw2, [entry(raw2, db2, 300, data_size=100)], 300)[0]
    assert st(r) == "SIZE_OVER" and r[1] == plain2[:100]


def test_entries_outside_the_buffers_are_refused(lib):
    raw, db = LS.stream_cases()["good"]
    for kw in ({"src_off": len(raw) + 1}, {"dst_off": 101}, {"cap": 101}, {"dst_off": 60, "cap": 41}, {"src_end": len(raw) + 1},
               {"src_off": 4, "src_end": 3}, {"data_size": 101, "cap": 100}, {"cap": 0xFFFFFFC1}):
        m = entry(raw, db, kw.pop("cap", 100), **kw)
        (r, out), = LS.mock_decode(lib, raw, [m], 100 if m.dst_cap < 1 << 20 else 0xFFFFFFC1 + 64)
        assert NAMES[r.status] == "REFUSED" and r.out_len == 0, kw


def test_dictionary_sizes():
    assert [LS.dict_size(b) for b in (12, 0x2C, 13, 0x2D, 0xF4, 29, 0xFD)] == [4096, 4096, 8192, 8192 - 512, (1 << 20) - 7 * 65536, 1 << 29, (1 << 29) - 7 * (1 << 25)]
