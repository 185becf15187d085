"""CPU-only: the gzip write filter's "single-member" option, as far as the CPU mock can show it.  The mock ignores
la_gzc_batch.framing (it writes a member per chunk whatever the field says), so nothing here writes data in that mode:
the option table and the empty stream are what the host code decides alone.  The data path is
tests/test_gpu_gzip_stream.py."""
import gzip
import struct
import time

import pytest

import la_api
import mock_build

ARCHIVE_OK, ARCHIVE_FAILED = 0, -25


@pytest.fixture(scope="module")
def mock_writer():
    import test_gpu_lz4_write as W
    mock = mock_build.host_lib()
    la_api.use_library(mock)
    saved = W._lib
    W._lib = lambda: W._lib_setup(mock)
    yield W
    W._lib = saved
    la_api.use_library(None)


def test_option_is_accepted_in_both_spellings(mock_writer):
    lib = mock_writer._lib()

    def set_option(module, key, value):
        a = lib.archive_write_new()
        assert lib.archive_write_add_filter_gzip(a) == ARCHIVE_OK
        rc = lib.archive_write_set_filter_option(a, module, key.encode(), None if value is None else value.encode())
        lib.archive_write_free(a)
        return rc

    for module in (b"gzip", None):
        assert set_option(module, "single-member", "1") == ARCHIVE_OK
        assert set_option(module, "single-member", None) == ARCHIVE_OK      # "!single-member"
    assert set_option(b"gzip", "single-members", "1") == ARCHIVE_FAILED
    # the lz4 filter has no such option
    a = lib.archive_write_new()
    assert lib.archive_write_add_filter_lz4(a) == ARCHIVE_OK
    assert lib.archive_write_set_filter_option(a, b"lz4", b"single-member", b"1") == ARCHIVE_FAILED
    lib.archive_write_free(a)


def test_empty_stream_is_the_twenty_bytes_of_today(mock_writer):
    W = mock_writer
    rc, today = W.write_lz4(b"", (("timestamp", None),), None, codec="gzip")
    assert rc == ARCHIVE_OK
    for options in ((("timestamp", None), ("single-member", "1")), (("single-member", "1"), ("timestamp", None)),
                    (("timestamp", None), ("compression-level", "6"), ("single-member", "1"))):
        rc, img = W.write_lz4(b"", options, None, codec="gzip")
        assert rc == ARCHIVE_OK and img == today
        # header with MTIME zero, XFL 0, OS 3; the empty final fixed block; CRC32 0; ISIZE 0
        assert img == b"\x1f\x8b\x08\x00" + bytes(4) + b"\x00\x03" + b"\x03\x00" + bytes(8)
        assert gzip.decompress(img) == b""
    # XFL follows the level as in the reference: 2 for level 9, 4 for level 1
    for level, xfl in (("9", 2), ("1", 4), ("0", 0), ("5", 0)):
        rc, img = W.write_lz4(b"", (("timestamp", None), ("compression-level", level), ("single-member", "1")), None, codec="gzip")
        assert rc == ARCHIVE_OK and len(img) == 20 and img[8] == xfl and img[:8] + img[9:] == today[:8] + today[9:]
    # without "!timestamp" the header carries the time
    t0 = int(time.time())
    rc, img = W.write_lz4(b"", (("single-member", "1"),), None, codec="gzip")
    assert rc == ARCHIVE_OK and len(img) == 20 and t0 <= struct.unpack_from("<I", img, 4)[0] <= int(time.time())
    assert img[:4] == today[:4] and img[8:] == today[8:] and gzip.decompress(img) == b""
    # off again: the many-member writer's empty stream, the same bytes
    rc, img = W.write_lz4(b"", (("timestamp", None), ("single-member", "1"), ("single-member", None)), None, codec="gzip")
    assert rc == ARCHIVE_OK and img == today
