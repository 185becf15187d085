"""The lzop write filter's HOST side (host/la_write_lzop.c: options, the header written into the gap of the first
window's bytes, windows of whole blocks, nothing kept between windows, the closing word, the empty archive as header and
closing word) over the CPU stand-in for la_gpu_lzop_compress (tests/mock_gpu/la_gpu_lzop_comp_mock.c, which compiles the
kernel's rules header under a serial matcher of its own).  Every image has to pass lzop_write_support.accept and comes
back through the project's own lzop read filter over the decode stand-in, where archive_filter_code and
archive_filter_name name it.  A stand-alone program writes the same shapes under the address and undefined-behaviour
sanitizers."""
import ctypes as C
import os
import subprocess

import pytest

import la_api
import lzop_support as LS
import lzop_write_support as W
import mock_build
from test_gpu_lz4_write import _lib_setup

ARCHIVE_OK, ARCHIVE_FAILED, ARCHIVE_FATAL = 0, -25, -30
WINDOW = 1 << 20        # LA_GPU_WRITE_WINDOW_MIB=1: sixteen blocks


@pytest.fixture(scope="module")
def lib():
    lib = _lib_setup(mock_build.host_lib())
    lib.archive_write_add_filter_lzop.argtypes = [C.c_void_p]
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def write_lzop(lib, data, options=(), piece=None, cap=None):
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_lzop(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_raw(a) == ARCHIVE_OK
        for k, v in options:
            rc = lib.archive_write_set_filter_option(a, b"lzop", k.encode(), None if v is None else v.encode())
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


def blocks_only(img):
    """an image without its mtime, which is the clock's"""
    return img[:25] + img[29:34] + img[38:]


def test_option_table(lib):
    """archive_write_lzop_options: what it refuses is ARCHIVE_WARN, which set_filter_option turns into ARCHIVE_FAILED"""
    data = LS.text(1, 3000)
    for value in ("0", "10", "a", "", None, "-1", "05"):
        rc, err = write_lzop(lib, data, (("compression-level", value),))
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, value
    for options in ((("threads", "1"),), (("threads", None),), (("no-such-option", "1"),), (("compression", "6"),)):
        rc, err = write_lzop(lib, data, options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    images = set()
    for level in "123456789":
        rc, img = write_lzop(lib, data, (("compression-level", level),))
        assert rc == ARCHIVE_OK, level
        W.accept(img, data, int(level))
        images.add(img[38:])
    assert len(images) == 1         # one coder: every level writes the same block bytes


def test_default_level_is_5(lib):
    data = W.inputs()["block_plus_1"]
    rc, img = write_lzop(lib, data)
    rc5, img5 = write_lzop(lib, data, (("compression-level", "5"),))
    assert rc == rc5 == ARCHIVE_OK and blocks_only(img) == blocks_only(img5)
    assert [b["usize"] for b in W.accept(img, data, 5)] == [65536, 1]


@pytest.mark.parametrize("level", range(1, 10))
def test_header_method_and_level_bytes(lib, level):
    rc, img = write_lzop(lib, b"some bytes", (("compression-level", str(level)),))
    assert rc == ARCHIVE_OK and (img[15], img[16]) == W.LEVELS[level] == {1: (2, 1), 7: (3, 7), 8: (3, 8), 9: (3, 9)}.get(level, (1, 5))
    W.accept(img, b"some bytes", level)


def test_empty_archive(lib):
    for options in ((), (("compression-level", "1"),), (("compression-level", "9"),)):
        rc, img = write_lzop(lib, b"", options)
        assert rc == ARCHIVE_OK and len(img) == 42
        assert W.accept(img, b"", int(dict(options).get("compression-level", 5))) == []
        r = la_api.cat(img)
        assert r.data == b"" and r.rc == la_api.ARCHIVE_EOF, r.error


def test_three_windows_in_odd_pieces(lib, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = LS.text(11, 2 * WINDOW) + LS.randbytes(12, 70000) + LS.text(13, 9)
    rc, img = write_lzop(lib, data, (), piece=99991)
    assert rc == ARCHIVE_OK
    assert len(W.accept(img, data)) == 34
    assert img.count(LS.MAGIC) == 1         # one header, in front of the first window's blocks only


@pytest.mark.parametrize("extra", [0, 1])
def test_exactly_one_window_and_one_byte_more(lib, monkeypatch, extra):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = LS.text(14, WINDOW + extra)
    rc, img = write_lzop(lib, data, (), piece=65536 + 17)
    assert rc == ARCHIVE_OK
    assert len(W.accept(img, data)) == 16 + extra


@pytest.mark.parametrize("name", sorted(W.inputs()))
def test_named_inputs(lib, name):
    data = W.inputs()[name]
    rc, img = write_lzop(lib, data)
    assert rc == ARCHIVE_OK
    W.accept(img, data)


def test_filter_code_and_name(lib):
    """the image names its filter to a reader: archive_filter_code / archive_filter_name over what the write filter wrote"""
    data = W.inputs()["block_plus_1"]
    rc, img = write_lzop(lib, data)
    assert rc == ARCHIVE_OK
    r = la_api.cat(img)
    assert r.filters[0] == (LS.ARCHIVE_FILTER_LZOP, "lzop") == (11, "lzop") and r.data == data and r.rc == la_api.ARCHIVE_EOF, r.error


def test_client_buffer_too_small(lib):
    rc, err = write_lzop(lib, LS.randbytes(13, 200000), (), cap=100)
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"


def test_sanitizer_program():
    """host sources, mocks and a main of its own in one link under -fsanitize=address,undefined; nothing is preloaded"""
    exe = mock_build.program("lzop_write_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "all shapes round-trip" in r.stdout
