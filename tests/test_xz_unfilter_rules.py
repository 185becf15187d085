"""The inverse delta / BCJ transforms of libarchive_amd/csrc/la_xz_filters_dev.h, compiled for the host
(tests/mock_gpu/xz_rules_shim.c), against liblzma's raw decoder.  For a buffer X and a filter F, liblzma's verdict
is lzma.decompress(LZMA2(X), FORMAT_RAW, [F, LZMA2]): the F decoder run over X, whatever X holds.  Both the header's
serial routine and the kernels' parallel formulation (tiles and row groups for delta, segment cutting for x86, a map
for the others; the independent pieces in descending order) must give those bytes."""
import ctypes as C
import lzma
import random

import pytest

import mock_build
import xz_chains_support as XC

LZMA2, spec = XC.LZMA2, XC.spec
DELTA, X86, POWERPC, IA64, ARM, ARMTHUMB, SPARC = XC.DELTA, XC.X86, XC.POWERPC, XC.IA64, XC.ARM, XC.ARMTHUMB, XC.SPARC
TILE, SUB = XC.TILE, XC.SUB


@pytest.fixture(scope="module")
def rules():
    lib = C.CDLL(mock_build.rules("libxz_rules.so"))
    lib.rules_serial.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64]
    lib.rules_serial.restype = None
    lib.rules_parallel.argtypes = [C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]
    lib.rules_valid.argtypes = [C.c_uint32, C.c_uint32]
    return lib


def liblzma_unfilter(fid, prop, data):
    return XC.liblzma_unfilter([(fid, prop)], data)


def liblzma_filter(fid, prop, data):
    return XC.liblzma_filter([(fid, prop)], data)


def ours(lib, fid, prop, data, parallel=None):
    buf = C.create_string_buffer(bytes(data), max(len(data), 1))
    if parallel is None:
        lib.rules_serial(fid, prop, buf, len(data))
    else:
        tile, sub, parts = parallel
        assert lib.rules_parallel(fid, prop, buf, len(data), tile, sub, parts) == 0
    return buf.raw[:len(data)]


def check(lib, fid, prop, data, tilings=((TILE, SUB, 256), (64, 8, 3), (7, 5, 2))):
    want = liblzma_unfilter(fid, prop, data)
    assert ours(lib, fid, prop, data) == want, ("serial", fid, prop, len(data))
    for tl in tilings:
        assert ours(lib, fid, prop, data, tl) == want, ("parallel", tl, fid, prop, len(data))
    return want


def noise(seed, n):
    return random.Random(seed).randbytes(n)


@pytest.mark.parametrize("dist", [1, 2, 3, 4, 255, 256])
def test_delta(rules, dist):
    for n in sorted({0, 1, dist - 1, dist, dist + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1}):
        data = noise(dist * 1000 + n, n)
        got = check(rules, DELTA, dist, data, tilings=((TILE, SUB, 256 // dist), (TILE, SUB, 1), (64, 8, 3), (7, 5, 2)))
        assert liblzma_filter(DELTA, dist, got) == data


@pytest.mark.parametrize("start_offset", [0, 0x1000, 0xFFFFFFFB])
def test_x86(rules, start_offset):
    for name, data in XC.x86_buffers().items():
        try:
            got = check(rules, X86, start_offset, data)
        except AssertionError as e:
            raise AssertionError(name, *e.args)
        assert liblzma_filter(X86, start_offset, got) == data or name != "real_code"


@pytest.mark.parametrize("fid,align", [(POWERPC, 4), (IA64, 16), (ARM, 4), (ARMTHUMB, 2), (SPARC, 4)])
def test_map_filters(rules, fid, align):
    for start_offset in (0, 0x1000, (0xFFFFFFFF // align) * align - 4 * align):
        for n in (0, 1, 3, 4, 5, 15, 16, 17, 31, 4099, 16384 + align + 1):
            data = XC.dense(fid, fid * 100 + n, n)
            got = check(rules, fid, start_offset, data)
            assert liblzma_filter(fid, start_offset, got) == data
        assert check(rules, fid, start_offset, XC.dense(fid, 7, 40000)) != XC.dense(fid, 7, 40000)      # (something did convert)


def test_thumb_adjacent_units(rules):
    """F0xx F8xx F0xx F8xx: a unit that converts keeps (b[3] & 0xF8) == 0xF8, so the unit two bytes on cannot convert and
    liblzma's extra step skips nothing a map over all halfwords would have taken"""
    r = random.Random(8)
    for k in range(40):
        data = b"".join(bytes([r.randrange(256), (0xF0 if (i + k // 20) % 2 == 0 else 0xF8) | r.randrange(8)]) for i in range(200 + k))
        check(rules, ARMTHUMB, 2 * k, data)
    data = b"".join(bytes([r.randrange(256), r.choice((0xF0, 0xF8, 0xF0, 0xF8, 0x12)) | r.randrange(8)]) for _ in range(5000))
    check(rules, ARMTHUMB, 0, data + b"\x00")


def test_property_rules(rules):
    """alignment of start_offset and the range of the delta distance: liblzma's LZMA_OPTIONS_ERROR"""
    for fid, align in ((X86, 1), (POWERPC, 4), (IA64, 16), (ARM, 4), (ARMTHUMB, 2), (SPARC, 4)):
        for off in (0, 1, 2, 4, 8, 16, 0x1001, 0xFFFFFFF0):
            ok = True
            try:
                lzma.decompress(lzma.compress(b"abc", format=lzma.FORMAT_RAW, filters=[LZMA2]), format=lzma.FORMAT_RAW, filters=[spec(fid, off), LZMA2])
            except lzma.LZMAError:
                ok = False
            assert ok == (off % align == 0) and bool(rules.rules_valid(fid, off)) == ok, (fid, off)
    assert [bool(rules.rules_valid(DELTA, d)) for d in (0, 1, 256, 257)] == [False, True, True, False]
    assert not rules.rules_valid(0x0A, 0) and not rules.rules_valid(0x0B, 0) and not rules.rules_valid(0x21, 0)
