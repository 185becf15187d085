"""The xz write filter's HOST side (host/la_write_xz.c: options, windows of whole blocks, the stream header on the first
window only, the index kept from the block headers that come back, index and footer at close(), the empty stream) over
the CPU stand-in for la_gpu_xz_compress (tests/mock_gpu/la_gpu_xz_comp_mock.c, which compiles the kernels' rules header).  Every image has
to pass xz_write_support.accept.  A stand-alone program writes the same shapes under the address and
undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

import xz_write_support as W
import mock_build
from test_gpu_lz4_write import _lib_setup

ARCHIVE_OK, ARCHIVE_FAILED, ARCHIVE_FATAL = 0, -25, -30
EMPTY = bytes.fromhex("fd377a585a000004e6d6b446" "000000001cdf4421" "1fb6f37d010000000004595a")
WINDOW = 1 << 20        # LA_GPU_WRITE_WINDOW_MIB=1: one block


@pytest.fixture(scope="module")
def lib():
    lib = _lib_setup(mock_build.host_lib())
    lib.archive_write_add_filter_xz.argtypes = [C.c_void_p]
    return lib


def write_xz(lib, data, options=(), piece=None, cap=None):
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_xz(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_raw(a) == ARCHIVE_OK
        for k, v in options:
            rc = lib.archive_write_set_filter_option(a, b"xz", k.encode(), None if v is None else v.encode())
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


def test_options(lib):
    data = W.filler(1, 3000)
    for value in ("10", "a", "", None):
        rc, err = write_xz(lib, data, (("compression-level", value),))
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, value
    for options in ((("threads", "x"),), (("threads", None),), (("threads", "4x"),), (("no-such-option", "1"),)):
        rc, err = write_xz(lib, data, options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    for options in ((("compression-level", "0"),), (("compression-level", "6"),), (("compression-level", "9"),), (("threads", "0"),),
                    (("threads", "4"),)):
        rc, img = write_xz(lib, data, options)
        assert rc == ARCHIVE_OK, options
        W.accept(img, data)


def test_empty_and_one_byte(lib):
    for options in ((), (("compression-level", "0"),)):
        rc, img = write_xz(lib, b"", options)
        assert rc == ARCHIVE_OK and img == EMPTY
        W.accept(img, b"")
        rc, img = write_xz(lib, b"x", options)
        assert rc == ARCHIVE_OK
        assert len(W.accept(img, b"x")["blocks"]) == 1


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_one_window_and_one_byte_more(lib, monkeypatch, extra):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["block_plus_1"][:WINDOW + extra]
    rc, img = write_xz(lib, data, (), piece=65536 + 17)
    assert rc == ARCHIVE_OK
    assert len(W.accept(img, data)["blocks"]) == 1 + extra


def test_three_windows_in_odd_pieces(lib, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["two_blocks_plus_1"] + W.noise(12, 70000) + W.filler(13, 9)
    rc, img = write_xz(lib, data, (("compression-level", "9"),), piece=99991)
    assert rc == ARCHIVE_OK
    w = W.accept(img, data)
    assert len(w["blocks"]) == 3 and [c[0] for c in w["blocks"][2]["chunks"]] == [0x01, 0x02]     # one byte of text, then noise: both stored


def test_client_buffer_too_small(lib):
    rc, err = write_xz(lib, W.noise(13, 200000), (), cap=100)
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"


def test_sanitizer_program():
    """host sources, mocks and a main of its own in one link under -fsanitize=address,undefined; nothing is preloaded"""
    exe = mock_build.program("xz_write_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "all shapes round-trip" in r.stdout
