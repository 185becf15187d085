"""The bzip2 WRITE filter on the device data plane (host/la_write_bzip2.c) through the archive_write_* slice:
archive_write_new -> add_filter_bzip2 -> set_format_raw -> open_memory -> header -> data (in pieces) -> close.  What it
writes must be ONE stream that reads back as the input through libbz2 (the library the reference's filter calls), the
reference's read loop over libbz2 and this repository's own read path (la_api.cat), and must stay within the recorded
margin of libbz2's own size."""
import bz2
import ctypes as C
import json
import os
import random

import pytest

import bzip2_support as BS
import la_api
import libarchive_amd as la
from test_gpu_lz4_write import ARCHIVE_FAILED, ARCHIVE_FATAL, ARCHIVE_OK, write_lz4

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bzip2_write_sizes.json")


def write_bzip2(data, options=(), piece=None, cap=None):
    la.host_lib().archive_write_add_filter_bzip2.argtypes = [C.c_void_p]     # (write_lz4's setup does not list it)
    return write_lz4(data, options, piece, cap if cap is not None else len(data) + len(data) // 50 + 65536, codec="bzip2")


def word_text(n):
    rnd = random.Random(14)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 10))) for _ in range(300)]
    return b" ".join(rnd.choice(words) for _ in range(n // 5))[:n]


def size_inputs():
    return {"word_text_1500000": word_text(1500000), "noise4_350000": BS.noise(350, 350000, 4),
            "random_300000": random.Random(300).randbytes(300000)}


def reads_back(img, data, level):
    assert img[:4] == b"BZh%d" % level
    dec = bz2.BZ2Decompressor()
    assert dec.decompress(img) == data and dec.eof and dec.unused_data == b""      # one stream
    magics = BS.find_magics(img)
    assert [k for _, k in magics] == [0] * -(-len(data) // (4 * ((100000 * level - 19) // 5))) + [1]
    for read_size in (1, 65536):
        assert BS.reference_read(img, read_size) == (data, 0, "")
    r = la_api.cat(img)
    assert r.filters[0] == (2, "bzip2") and r.data == data and r.rc == la_api.ARCHIVE_EOF, r.error


ROUND_TRIPS = {
    "empty": (lambda: b"", None), "one_byte": (lambda: b"x", None),
    "text": (lambda: word_text(4 * 1024 * 1024 + 333), 65536 + 17),
    "random": (lambda: random.Random(14).randbytes(2 * 1024 * 1024 + 5), 99991),
    "zeros": (lambda: bytes(3 << 20), 4096),
}


@pytest.mark.parametrize("options,level", [((), 9), ((("compression-level", "0"),), 1), ((("compression-level", "1"),), 1)],
                         ids=["default", "level0", "level1"])
@pytest.mark.parametrize("name", sorted(ROUND_TRIPS))
def test_bzip2_write_filter_round_trips(gpu_ctx, monkeypatch, name, options, level):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "2")      # several windows for a few MiB of input
    make, piece = ROUND_TRIPS[name]
    data = make()
    rc, img = write_bzip2(data, options, piece)
    assert rc == ARCHIVE_OK and isinstance(img, bytes), img
    reads_back(img, data, level)
    if not data:
        assert len(img) == 14


def test_data_ending_on_a_window_boundary(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    bb = 4 * ((100000 - 19) // 5)
    data = BS.letters(8, (1 << 20) // bb * bb, 12)
    rc, img = write_bzip2(data, (("compression-level", "1"),), 50000)
    assert rc == ARCHIVE_OK
    reads_back(img, data, 1)


def test_output_is_read_under_the_default_bid_policy(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_BID", "auto")
    data = word_text(1200000)
    rc, img = write_bzip2(data)
    assert rc == ARCHIVE_OK
    r = la_api.cat(img)
    assert r.filters[0] == (2, "bzip2") and r.data == data and r.rc == la_api.ARCHIVE_EOF


def test_bzip2_write_filter_errors(gpu_ctx):
    for options in ((("no-such-option", "1"),), (("compression-level", "10"),), (("compression-level", "a"),), (("compression-level", None),)):
        rc, err = write_bzip2(b"abc", options)
        assert rc == ARCHIVE_FAILED and "Undefined option" in err, options
    rc, err = write_bzip2(random.Random(1).randbytes(200000), (), None, cap=100)     # the client's buffer is too small
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("name", ["word_text_1500000", "noise4_350000", "random_300000"])
def test_size_against_libbz2(gpu_ctx, name, level):
    """len(ours) <= len(libbz2) * (1 + margin): the margin is the worst excess measured on the device when the golden
    file was written, rounded up to the next half percent; the output is deterministic, so it absorbs nothing and
    catches a later change that drops tables or refinement passes.  The golden file records libbz2's sizes too."""
    with open(GOLDEN) as f:
        golden = json.load(f)
    data = size_inputs()[name]
    ref = len(bz2.compress(data, level))
    assert ref == golden["cases"]["%s/%d" % (name, level)]["libbz2"]
    rc, img = write_bzip2(data, (("compression-level", str(level)),))
    assert rc == ARCHIVE_OK and bz2.decompress(img) == data
    print(name, level, "ours", len(img), "libbz2", ref, "ratio %.5f" % (len(img) / ref))
    assert len(img) <= ref * (1 + golden["margin"]), (len(img), ref, golden["margin"])
