"""The LZO1X rules.  Two statements of them exist, both written from the format description and neither from liblzo2:
lzop_support.decode() in Python and libarchive_amd/csrc/la_lzo_dev.h, which the kernel and the CPU stand-in
(tests/mock_gpu/la_gpu_lzop_mock.c) compile.  What pins the Python one is independent of both: every block of the reference's seven lzop
fixtures carries the Adler-32 of its decoded bytes.  The header then has to equal the Python decoder in bytes and
verdict on every instruction form, every length-run edge, the distances at which a form or a copy path changes, and the
four pinned verdicts; the expected bytes of the hand-built streams come from the emitter's own book-keeping."""
import hashlib
import zlib

import pytest

import lzop_support as L
import mock_build


@pytest.fixture(scope="module")
def mock():
    return mock_build.gpu_lib()


def header_decode(mock, streams):
    """[(status name, bytes, consumed)] of the rules header over [(stream, dst_len)]"""
    return [L.rules_decode(mock, s, n) for s, n in streams]


def test_the_python_decoder_reproduces_every_fixture_blocks_adler32():
    """the test that pins the oracle"""
    sizes = []
    for m, img in L.fixtures():
        seen = []
        data, rc, msg = L.reference_read(img, on_block=lambda plain, flags, word: seen.append((plain, flags, word)))
        assert (rc, msg) == (0, ""), m["file"]
        assert seen, m["file"]
        for plain, flags, word in seen:
            assert flags & L.ADLER32_UNCOMPRESSED and not flags & L.CRC32_UNCOMPRESSED
            assert zlib.adler32(plain) == word, m["file"]
        assert len(data) == m["decoded_size"] and hashlib.sha256(data).hexdigest() == m["sha256"], m["file"]
        sizes.append(len(data))
    assert sorted(sizes) == sorted([3072, 265728, 3072, 512, 3072, 4608, 265728])


def test_the_forms_the_fixtures_exercise_and_the_hand_built_cases_cover_the_rest():
    forms = set()
    for _, img in L.fixtures():
        L.reference_read(img, forms=forms)
    assert forms == L.FIXTURE_FORMS
    built = set()
    for stream, dst_len, verdict, _ in L.rules_cases().values():
        if verdict == "OK":
            L.decode(stream, dst_len, built)
    assert built == L.ALL_FORMS
    assert L.ALL_FORMS - L.FIXTURE_FORMS == {"first_byte_short", "first_byte_long", "m1_2byte", "m1_3byte", "m4_short", "m4_long"}


def test_the_cases_name_the_edges():
    names = set(L.rules_cases())
    assert {"literals_%d" % n for n in (18, 19, 273, 274, 528)} <= names
    assert {"m3_len_%d" % n for n in (33, 34, 288, 289)} <= names and {"m4_len_%d" % n for n in (9, 10, 264, 265)} <= names
    assert {"dist_%d_len_6" % d for d in (1, 2, 63, 64, 65, 2048, 2049, 3072, 16384, 16385, 32768, 49151)} <= names
    # the length-run edges stand where the run's byte count changes: 18 is the last short run, 273 the last with no zero byte
    e = L.rules_cases()
    assert e["literals_18"][0][0] == 15 and e["literals_19"][0][:2] == b"\x00\x01" and e["literals_273"][0][:2] == b"\x00\xff"
    assert e["literals_274"][0][:3] == b"\x00\x00\x01" and e["literals_528"][0][:3] == b"\x00\x00\xff"


def test_python_decoder_against_the_emitters_book_keeping():
    for name, (stream, dst_len, verdict, plain) in L.rules_cases().items():
        got = L.decode(stream, dst_len)
        assert got[0] == verdict, name
        assert got[1] == plain, name
        if verdict in ("OK", "SHORT_OUTPUT"):
            assert got[2] == len(stream), name


def test_rules_header_equals_the_python_decoder_on_every_case(mock):
    cases = L.rules_cases()
    got = header_decode(mock, [(c[0], c[1]) for c in cases.values()])
    for (name, (stream, dst_len, verdict, plain)), g in zip(cases.items(), got):
        ref = L.decode(stream, dst_len)
        assert g == ref, name
        assert g[0] == verdict and g[1] == plain, name


def test_the_four_pinned_verdicts_stand_alone(mock):
    """one violation per stream: the same stream without it decodes, and the violation is far from every other limit"""
    c = L.rules_cases()
    assert c["lookbehind_by_one"][2] == "LOOKBEHIND" and c["reaches_byte_0"][2] == "OK"
    assert c["output_overrun_match"][2] == "OUTPUT_OVERRUN" and L.decode(c["output_overrun_match"][0], 700)[0] == "OK"
    assert c["input_overrun_no_marker"][2] == "INPUT_OVERRUN" and L.decode(c["input_overrun_no_marker"][0] + b"\x11\x00\x00", 702)[0] == "OK"
    assert c["not_consumed"][2] == "NOT_CONSUMED" and L.decode(c["not_consumed"][0][:-40], 700)[0] == "OK"
    # a lookbehind is tested before the output room: a match that fails both is a lookbehind
    both = L.Emitter().first_literals(b"abcd").m3(100, 400, check=False).end()
    assert L.decode(both.stream(), 10)[0] == "LOOKBEHIND"
    assert header_decode(mock, [(both.stream(), 10)])[0][0] == "LOOKBEHIND"


def test_cut_at_every_byte(mock):
    stream, plain = L.cut_stream()
    assert 2048 <= len(stream) < 2400
    assert L.decode(stream, len(plain)) == ("OK", plain, len(stream))
    cuts = [(stream[:k], len(plain)) for k in range(len(stream))]
    got = header_decode(mock, cuts)
    kinds = set()
    for k, g in enumerate(got):
        ref = L.decode(stream[:k], len(plain))
        # the kind: the input ran out, or one of the pinned verdicts (a cut can leave a prefix that ends in 11 00 00 or asks
        # for more room); never OK, and the bytes in front are a prefix of the plain text
        assert g[0] in ("INPUT_OVERRUN", "OUTPUT_OVERRUN", "LOOKBEHIND", "NOT_CONSUMED", "SHORT_OUTPUT"), k
        assert g[0] == ref[0] and g[1] == ref[1] and plain.startswith(g[1]), k
        kinds.add(g[0])
    assert "INPUT_OVERRUN" in kinds


def test_compressor_round_trip(mock):
    inputs = [b"", b"a", b"abc", b"abcd", L.text(1, 5000), L.noise(2, 3000), L.noise(3, 70000, 4), bytes(100000), L.text(4, 60000) + L.noise(5, 300) + L.text(4, 60000)]
    streams = [(L.compress(p), len(p)) for p in inputs]
    forms = set()
    for p, (s, n) in zip(inputs, streams):
        assert L.decode(s, n, forms) == ("OK", p, len(s))
    assert {"m2", "m3_short", "m3_long", "m4_short", "first_byte_short", "literals_long"} <= forms
    for p, g in zip(inputs, header_decode(mock, streams)):
        assert g[0] == "OK" and g[1] == p


def test_sums_and_refusals_of_the_stand_in(mock):
    """what the kernel adds around the header, in the stand-in that the host tests run over"""
    p = L.text(9, 3000)
    s = L.compress(p)
    src, blocks, total = L.pack_table([(s, len(p))] * 6 + [(p, len(p))])
    for b, (flags, sc, su) in zip(blocks, ((L.C_ADLER32 | L.U_ADLER32, zlib.adler32(s), zlib.adler32(p)), (L.C_CRC32 | L.U_CRC32, zlib.crc32(s), zlib.crc32(p)),
                                           (15, zlib.crc32(s), zlib.crc32(p)), (L.C_ADLER32, 1, 0), (L.U_CRC32, 0, 1), (0, 5, 6),
                                           (L.U_ADLER32 | L.C_CRC32, zlib.crc32(p), 12345))):
        b.flags, b.sum_c, b.sum_u = flags, sc, su
    blocks.append(L.Block(len(src) - 2, 0, 3, 8, 0, 0, 0, 0))
    blocks.append(L.Block(0, 0, 9, 8, 0, 0, 0, 0))
    blocks.append(L.Block(0, 0, 8, (64 << 20) + 1, 0, 0, 0, 0))
    got = L.mock_decode(mock, src, blocks, total)
    assert [r.status for r, _ in got] == [0, 0, 0, L.ST["BAD_SUM_C"], L.ST["BAD_SUM_U"], 0, 0] + [L.ST["REFUSED"]] * 3
    assert all(d == p for (r, d) in got[:3] + got[4:7]) and got[3][1] == b""
