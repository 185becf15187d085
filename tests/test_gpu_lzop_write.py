"""The lzop WRITE filter on the device data plane (host/la_write_lzop.c) through the archive_write_* slice:
archive_write_new -> add_filter_lzop -> set_format_raw -> open_memory -> header -> data (in pieces) -> close.  What it
writes must be one part of the promised shape (lzop_write_support.accept: the template header, 64 KiB blocks, the closing
word, the reference's read loop over the Python decoder) that this repository's own lzop read filter on the device
(la_api.cat) returns as the input."""
import ctypes as C

import pytest

import la_api
import libarchive_amd as la
import lzop_support as LS
import lzop_write_support as W
from test_gpu_lz4_write import ARCHIVE_FAILED, ARCHIVE_FATAL, ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu


def write_lzop(data, options=(), piece=None, cap=None):
    la.host_lib().archive_write_add_filter_lzop.argtypes = [C.c_void_p]     # (write_lz4's setup does not list it)
    return write_lz4(data, options, piece, cap if cap is not None else len(data) + len(data) // 20 + 65536, codec="lzop")


def reads_back(img, data, level):
    blocks = W.accept(img, data, level)
    r = la_api.cat(img)
    assert r.data == data and r.rc == la_api.ARCHIVE_EOF, r.error
    if data:
        assert r.filters[0] == (11, "lzop")
    return blocks


@pytest.mark.parametrize("level", [None, "1", "9"])
def test_one_window(gpu_ctx, level):
    data = W.inputs()["text_noise_text"] + W.inputs()["pair_49151"] + W.inputs()["block_plus_1"]
    rc, img = write_lzop(data, (("compression-level", level),) if level else (), piece=65536 + 17)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    assert len(reads_back(img, data, int(level or 5))) == -(-len(data) // 65536)


def test_two_and_a_half_mib_under_a_window_of_one(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    data = LS.text(61, 2 << 20) + LS.randbytes(62, (1 << 19) + 1)
    rc, img = write_lzop(data, (("compression-level", "6"),), piece=99991)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    assert len(reads_back(img, data, 6)) == 41 and img.count(LS.MAGIC) == 1


def test_empty_archive(gpu_ctx):
    for options, level in (((), 5), ((("compression-level", "1"),), 1), ((("compression-level", "9"),), 9)):
        rc, img = write_lzop(b"", options)
        assert rc == ARCHIVE_OK and len(img) == 42
        assert reads_back(img, b"", level) == []


def test_errors(gpu_ctx):
    for options in ((("no-such-option", "1"),), (("compression-level", "0"),), (("compression-level", "10"),), (("compression-level", "a"),),
                    (("compression-level", ""),), (("compression-level", None),), (("threads", "1"),)):
        rc, err = write_lzop(b"abc", options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    rc, err = write_lzop(LS.randbytes(1, 200000), (), None, cap=100)     # the client's buffer is too small
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"
