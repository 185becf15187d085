"""The lzip write filter's HOST side (host/la_write_lzip.c: options, windows of whole members, nothing kept between
windows, the empty archive as one member of no data from the compress call) over the CPU stand-in for
la_gpu_lzip_compress (tests/mock_gpu/la_gpu_lzip_comp_mock.c, which compiles the kernels' rules header).  Every image has to pass
lzip_write_support.accept and comes back through the project's own lzip read filter over the decode stand-in, where
archive_filter_code and archive_filter_name name it.  A stand-alone program writes the same shapes under the address
and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

import la_api
import lzip_support as LS
import lzip_write_support as W
import mock_build
from test_gpu_lz4_write import _lib_setup

ARCHIVE_OK, ARCHIVE_FAILED, ARCHIVE_FATAL = 0, -25, -30
WINDOW = 1 << 20        # LA_GPU_WRITE_WINDOW_MIB=1: sixteen members, or four large ones


@pytest.fixture(scope="module")
def lib():
    lib = _lib_setup(mock_build.host_lib())
    lib.archive_write_add_filter_lzip.argtypes = [C.c_void_p]
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def write_lzip(lib, data, options=(), piece=None, cap=None):
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_lzip(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_raw(a) == ARCHIVE_OK
        for k, v in options:
            rc = lib.archive_write_set_filter_option(a, b"lzip", k.encode(), None if v is None else v.encode())
            if rc != ARCHIVE_OK:
                return rc, lib.archive_error_string(a).decode()
        cap = cap if cap is not None else len(data) + len(data) // 20 + 65536
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


def test_option_table(lib):
    """archive_compressor_xz_options: what it refuses is ARCHIVE_WARN, which set_filter_option turns into ARCHIVE_FAILED"""
    data = W.filler(1, 3000)
    for value in ("10", "a", "", "-1", "06", None):
        rc, err = write_lzip(lib, data, (("compression-level", value),))
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, value
    for options in ((("threads", "x"),), (("threads", None),), (("threads", "4x"),), (("threads", "4 "),),
                    (("no-such-option", "1"),), (("compression", "6"),)):
        rc, err = write_lzip(lib, data, options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    for level in "0123456789":
        rc, img = write_lzip(lib, data, (("compression-level", level),))
        assert rc == ARCHIVE_OK, level
        W.accept(img, data, int(level))
    for options in ((("threads", "0"),), (("threads", "4"),), (("threads", "4"), ("compression-level", "9"))):
        rc, img = write_lzip(lib, data, options)
        assert rc == ARCHIVE_OK, options
        W.accept(img, data, int(dict(options).get("compression-level", 6)))


def test_default_level_is_6(lib):
    data = W.inputs()["far_pair"]
    rc, img = write_lzip(lib, data)
    assert rc == ARCHIVE_OK and (rc, img) == write_lzip(lib, data, (("compression-level", "6"),))
    assert [m["dict_byte"] for m in W.accept(img, data, 6)] == [0x10] * 4
    rc, img9 = write_lzip(lib, data, (("compression-level", "9"),))
    assert [m["dict_byte"] for m in W.accept(img9, data, 9)] == [0x12] and len(img9) < len(img)


def test_empty_archive(lib):
    for options in ((), (("compression-level", "0"),), (("compression-level", "9"),)):
        rc, img = write_lzip(lib, b"", options)
        assert rc == ARCHIVE_OK
        (m,) = W.accept(img, b"", int(dict(options).get("compression-level", 6)))
        assert m["data_size"] == 0 and len(img) == 26 + len(m["stream"])


def test_three_windows_in_odd_pieces(lib, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["text_2mib"] + W.noise(12, 70000) + W.filler(13, 9)
    for level, members in ((6, 34), (9, 9)):
        rc, img = write_lzip(lib, data, (("compression-level", str(level)),), piece=99991)
        assert rc == ARCHIVE_OK
        assert len(W.accept(img, data, level)) == members


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_one_window_and_one_byte_more(lib, monkeypatch, extra):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["text_2mib"][:WINDOW + extra]
    rc, img = write_lzip(lib, data, (), piece=65536 + 17)
    assert rc == ARCHIVE_OK
    assert len(W.accept(img, data, 6)) == 16 + extra


def test_filter_code_and_name(lib):
    """the image names its filter to a reader: archive_filter_code / archive_filter_name over what the write filter wrote"""
    data = W.inputs()["m_plus_1"]
    rc, img = write_lzip(lib, data)
    assert rc == ARCHIVE_OK
    r = la_api.cat(img)
    assert r.filters[0] == (LS.ARCHIVE_FILTER_LZIP, "lzip") == (9, "lzip") and r.data == data and r.rc == la_api.ARCHIVE_EOF, r.error


def test_client_buffer_too_small(lib):
    rc, err = write_lzip(lib, W.noise(13, 200000), (), cap=100)
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"


def test_sanitizer_program():
    """host sources, mocks and a main of its own in one link under -fsanitize=address,undefined; nothing is preloaded"""
    exe = mock_build.program("lzip_write_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "all shapes round-trip" in r.stdout
