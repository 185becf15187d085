"""The bzip2 write filter's HOST side (host/la_write_bzip2.c: options, windows of whole blocks, FIRST on the first
window, LAST on close()'s flush only, the device-resident stream state, the empty stream) over a CPU stand-in for
la_gpu_bzip2_compress (tests/mock_gpu/la_gpu_bzip2_comp_mock.c: the real libbz2, one block per cut).  Every image must be ONE stream that
libbz2 (bz2.decompress) and the reference's read loop over libbz2 (bzip2_support.reference_read) decode to the input.
A stand-alone program writes the same shapes under the address and undefined-behaviour sanitizers."""
import bz2
import ctypes as C
import os
import subprocess

import pytest

import bzip2_support as BS
import mock_build
from test_gpu_lz4_write import _lib_setup

ARCHIVE_OK, ARCHIVE_FAILED, ARCHIVE_FATAL = 0, -25, -30
BLOCK1 = 4 * ((100000 - 19) // 5)
WINDOW1 = (1 << 20) // BLOCK1 * BLOCK1        # LA_GPU_WRITE_WINDOW_MIB=1 at level 1: 13 whole blocks


@pytest.fixture(scope="module")
def lib():
    lib = _lib_setup(mock_build.host_lib())
    lib.archive_write_add_filter_bzip2.argtypes = [C.c_void_p]
    return lib


def write_bzip2(lib, data, options=(), piece=None, cap=None):
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_bzip2(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_raw(a) == ARCHIVE_OK
        for k, v in options:
            rc = lib.archive_write_set_filter_option(a, b"bzip2", k.encode(), None if v is None else v.encode())
            if rc != ARCHIVE_OK:
                return rc, lib.archive_error_string(a).decode()
        cap = cap if cap is not None else len(data) + len(data) // 50 + 65536
        buf = C.create_string_buffer(cap)
        used = C.c_size_t(0)
        assert lib.archive_write_open_memory(a, buf, cap, C.byref(used)) == ARCHIVE_OK
        assert lib.archive_write_header(a, None) == ARCHIVE_OK
        step = piece or max(len(data), 1)
        for i in range(0, len(data), step):
            chunk = data[i:i + step]
            if lib.archive_write_data(a, chunk, len(chunk)) != len(chunk):
                return ARCHIVE_FATAL, lib.archive_error_string(a).decode()
        rc = lib.archive_write_close(a)
        if rc != ARCHIVE_OK:
            return rc, lib.archive_error_string(a).decode()
        return rc, buf.raw[:used.value]
    finally:
        lib.archive_write_free(a)


def one_stream_of(img, data, level):
    assert img[:4] == b"BZh%d" % level
    dec = bz2.BZ2Decompressor()
    assert dec.decompress(img) == data and dec.eof and dec.unused_data == b""      # ONE stream, nothing behind it
    for read_size in (None, 4096):
        assert BS.reference_read(img, read_size) == (data, 0, "")
    magics = BS.find_magics(img)
    assert [k for _, k in magics].count(1) == 1 and magics[-1][1] == 1
    return magics


def test_options(lib):
    for value in ("10", "a", "", None, "-1"):
        rc, err = write_bzip2(lib, b"abc", (("compression-level", value),))
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, value
    rc, err = write_bzip2(lib, b"abc", (("no-such-option", "1"),))
    assert rc == ARCHIVE_FAILED and "Undefined option" in err
    for value, level in (("0", 1), ("1", 1), ("5", 5), ("9", 9)):
        rc, img = write_bzip2(lib, b"abc" * 100, (("compression-level", value),))
        assert rc == ARCHIVE_OK
        one_stream_of(img, b"abc" * 100, level)


def test_empty_and_one_byte(lib):
    for options, level in (((), 9), ((("compression-level", "1"),), 1)):
        rc, img = write_bzip2(lib, b"", options)
        assert rc == ARCHIVE_OK and len(img) == 14 and img == bz2.compress(b"", level)
        one_stream_of(img, b"", level)
        rc, img = write_bzip2(lib, b"x", options)
        assert rc == ARCHIVE_OK
        assert len(one_stream_of(img, b"x", level)) == 2


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_one_window_and_one_byte_more(lib, monkeypatch, extra):
    """the data ends on the window boundary: close() still makes a call, which writes the trailer alone"""
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = BS.letters(11, WINDOW1 + extra, 6)
    rc, img = write_bzip2(lib, data, (("compression-level", "1"),), piece=65536 + 17)
    assert rc == ARCHIVE_OK
    magics = one_stream_of(img, data, 1)
    assert len(magics) == WINDOW1 // BLOCK1 + extra + 1


def test_three_windows(lib, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = BS.noise(12, 3 * WINDOW1 - 7, 40)
    rc, img = write_bzip2(lib, data, (("compression-level", "1"),), piece=99991)
    assert rc == ARCHIVE_OK
    magics = one_stream_of(img, data, 1)
    assert len(magics) == -(-len(data) // BLOCK1) + 1
    assert any(bit % 8 for bit, _ in magics)        # blocks are joined at bit granularity, across windows too


def test_client_buffer_too_small(lib):
    rc, err = write_bzip2(lib, BS.noise(13, 200000), (("compression-level", "1"),), cap=100)
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"


def test_sanitizer_program():
    """host sources, mocks and a main of its own in one link under -fsanitize=address,undefined; nothing is preloaded"""
    exe = mock_build.program("bzip2_write_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "all shapes round-trip" in r.stdout
