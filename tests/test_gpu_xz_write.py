"""The xz WRITE filter on the device data plane (host/la_write_xz.c) through the archive_write_* slice:
archive_write_new -> add_filter_xz -> set_format_raw -> open_memory -> header -> data (in pieces) -> close.  What it
writes must be ONE stream of the promised shape (xz_write_support.accept: liblzma, the reference's read loop, the walker)
that this repository's own xz read filter on the device (la_api.cat) returns as the input."""
import ctypes as C
import lzma

import pytest

import la_api
import libarchive_amd as la
import xz_write_support as W
from test_gpu_lz4_write import ARCHIVE_FAILED, ARCHIVE_FATAL, ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu


def write_xz(data, options=(), piece=None, cap=None):
    la.host_lib().archive_write_add_filter_xz.argtypes = [C.c_void_p]     # (write_lz4's setup does not list it)
    return write_lz4(data, options, piece, cap if cap is not None else len(data) + len(data) // 50 + 65536, codec="xz")


def reads_back(img, data):
    w = W.accept(img, data)
    r = la_api.cat(img)
    assert r.filters[0] == (6, "xz") and r.data == data and r.rc == la_api.ARCHIVE_EOF, r.error
    return w


@pytest.mark.parametrize("level", ["0", "6", "9"])
def test_one_window(gpu_ctx, level):
    data = W.inputs()["text_noise_text"] + W.inputs()["block_plus_1"]
    rc, img = write_xz(data, (("compression-level", level),), piece=65536 + 17)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    assert len(reads_back(img, data)["blocks"]) == 2


@pytest.mark.parametrize("level", ["0", "6", "9"])
def test_three_windows(gpu_ctx, monkeypatch, level):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["two_blocks_plus_1"] + W.filler(61, 70001)
    rc, img = write_xz(data, (("compression-level", level), ("threads", "4")), piece=99991)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    assert len(reads_back(img, data)["blocks"]) == 3


def test_data_ending_on_a_window_boundary(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = W.inputs()["block"]
    rc, img = write_xz(data)
    assert rc == ARCHIVE_OK
    assert len(reads_back(img, data)["blocks"]) == 1


def test_empty_archive(gpu_ctx):
    for options in ((), (("compression-level", "0"),)):
        rc, img = write_xz(b"", options)
        assert rc == ARCHIVE_OK and img == lzma.compress(b"", check=lzma.CHECK_CRC64) and len(img) == 32
        reads_back(img, b"")


def test_errors(gpu_ctx):
    for options in ((("no-such-option", "1"),), (("compression-level", "10"),), (("compression-level", "a"),), (("compression-level", None),),
                    (("threads", "x"),)):
        rc, err = write_xz(b"abc", options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    rc, err = write_xz(W.noise(1, 200000), (), None, cap=100)     # the client's buffer is too small
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"
