"""The gzip read filter's block-start mode (LA_GZIP_BLOCK_STARTS=1, la_filter_gzip.c) over a CPU stand-in for
la_gpu_gzip_decode with LA_GZ_OPT_BLOCK_STARTS (tests/mock_gpu/la_gpu_gz_blocks_mock.cpp: the kernels' rules header for the candidates, zlib
walked with Z_BLOCK for the pieces).  la_api.cat through the mock library must equal the reference filter over zlib
(oracle_lib.gzip_stream_decode) on bytes, return code and error string, at read sizes None, 1000 and 1, with the span of one
device call held to 40 000 bytes so that a stream takes several windows, windows begin in mid-byte, the history is carried
and spans that confirm nothing have to grow.  Without the switch the same streams go the way they went before."""

import pytest

import deflate_find_support as F
import la_api
import mock_build
import oracle_lib as O

ARCHIVE_FILTER_GZIP = 1
STREAMS = sorted(F.filter_streams())


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("LA_GZIP_BLOCK_STARTS", "1")
    monkeypatch.setenv("LA_GZ_TEST_BLOCKS_WINDOW", "40000")
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "16")
    monkeypatch.setenv("LA_GPU_BID", "auto")        # (the suite's default is "all": here the bid policy itself takes the member)


def reference(image):
    ref, res = O.gzip_stream_decode(image, 4 << 20)
    return ref.tobytes(), res.rc, res.errmsg.decode()


def same_as_reference(image, read_size=None):
    want = reference(image)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(want[0]), want[1], want[2])
    assert got[0] == want[0]
    return res


@pytest.mark.parametrize("name", STREAMS)
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_streams_with_the_switch(mock, switch_on, name, read_size):
    res = same_as_reference(F.filter_streams()[name], read_size)
    assert res.filters[0] == (ARCHIVE_FILTER_GZIP, "gzip")


@pytest.mark.parametrize("name", ["wrong-crc32", "wrong-isize"])
def test_trailer_is_compared_under_strict(mock, switch_on, monkeypatch, name):
    """the CRC32 folded over the windows and the byte count against the trailer, as for chains: with LA_GZIP_STRICT=1 the
    status's own message (the reference never looks, gzip.c:423)"""
    monkeypatch.setenv("LA_GZIP_STRICT", "1")
    image = F.filter_streams()[name]
    good = reference(F.filter_streams()["text-level-6"])
    res = la_api.cat(image)
    # (every byte in front of the unit that shows the mismatch: the windows before the last one, as for chains of pieces)
    assert res.rc == la_api.ARCHIVE_FATAL and 0 < len(res.data) < len(good[0]) and good[0].startswith(res.data)
    assert ("CRC" in res.error) if name == "wrong-crc32" else ("ISIZE" in res.error or "size" in res.error.lower())
    res = la_api.cat(F.filter_streams()["text-level-6"])
    assert (res.rc, res.data) == (la_api.ARCHIVE_EOF, good[0])


def test_a_run_of_stored_blocks_longer_than_the_window_limit_goes_the_ordinary_way(mock, switch_on, monkeypatch):
    """1.5 MiB of noise is one run of stored blocks; with the window limit at 1 MiB no span of it ever confirms a block
    start, and since nothing of the member is out yet it is decoded the ordinary way"""
    import random
    noise = random.Random(78).randbytes(3 << 19)
    image = F.gz_member(F.raw_deflate(noise, 6), noise)
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GZ_TEST_BLOCKS_WINDOW", "300000")
    res = same_as_reference(image, 65536)
    assert res.rc == la_api.ARCHIVE_EOF and res.data == noise


@pytest.mark.parametrize("name", ["text-level-6", "second-member-behind-the-first", "cut-inside-a-block", "flipped-bit-in-the-third-block"])
def test_without_the_switch_nothing_changes(mock, monkeypatch, name):
    image = F.filter_streams()[name]
    monkeypatch.delenv("LA_GZIP_BLOCK_STARTS", raising=False)
    monkeypatch.setenv("LA_GZ_TEST_BLOCKS_WINDOW", "40000")
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "16")
    monkeypatch.setenv("LA_GPU_BID", "auto")
    # the bid policy declines a lone member that is longer than the look-ahead: no gzip filter, the bytes pass as they are
    res = la_api.cat(image)
    if name == "second-member-behind-the-first":
        pass        # (whether a second header shows inside 16 KiB is the parent's rule, not this test's)
    else:
        assert res.filters[0][1] != "gzip" and res.data == image
    # taken by LA_GPU_BID=all it is decoded the ordinary way, as before
    monkeypatch.setenv("LA_GPU_BID", "all")
    res = same_as_reference(image)
    assert res.filters[0] == (ARCHIVE_FILTER_GZIP, "gzip")
