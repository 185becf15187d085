"""The zstd WRITE filter on the device data plane (host/la_write_zstd.c) through the archive_write_* slice:
archive_write_new -> add_filter_zstd -> set_format_raw -> open_memory -> header -> data (in pieces) -> close.  What it
writes must read back as the input through the image's libzstd (the library the reference's filter calls), the
oracle's stream decoder and this repository's own read path (la_api.cat), and must have the frame shape it promises."""
import random

import pytest

import la_api
import zstd_support as Z
from test_gpu_lz4_write import ARCHIVE_FAILED, ARCHIVE_FATAL, ARCHIVE_OK, write_lz4
from test_gpu_zstd_compress import walk

pytestmark = pytest.mark.gpu


def write_zstd(data, options=(), piece=None, cap=None):
    return write_lz4(data, options, piece, cap, codec="zstd")


def test_zstd_write_filter_round_trips(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_WRITE_WINDOW_MIB", "2")      # several windows for a few MiB of input
    z, o = Z.libzstd(), Z.oracle_lib()
    assert z is not None
    rnd = random.Random(14)
    words = [bytes(rnd.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rnd.randint(2, 10))) for _ in range(300)]
    text = b" ".join(rnd.choice(words) for _ in range(700000))[:4 * 1024 * 1024 + 333]
    for data, piece in ((b"", None), (b"x", None), (text, 65536 + 17), (rnd.randbytes(2 * 1024 * 1024 + 5), 99991), (bytes(3 << 20), 4096)):
        for options in ((), (("compression-level", "0"),), (("max-frame-in", "64k"),)):
            rc, img = write_zstd(data, options, piece)
            assert rc == ARCHIVE_OK and isinstance(img, bytes), img
            assert Z.zstd_decompress(z, img, len(data) + 16) == data
            assert Z.oracle_decode(o, img, len(data) + 16) == (0, data, "")
            r = la_api.cat(img)
            assert r.filters[0] == (14, "zstd") and r.data == data, r.error
            frames = walk(img)
            assert all(f["csum"] == 1 and f["single"] == 1 for f in frames)
            limit = 65536 if ("max-frame-in", "64k") in options else 131072
            assert all(f["fcs"] <= limit for f in frames)
            assert len(frames) == max(1, -(-len(data) // limit))
            if data is text:
                literal_types = {b[2] for f in frames for b in f["blocks"] if b[0] == 2}
                assert literal_types == ({0} if ("compression-level", "0") in options else {2})


def test_default_output_is_read_under_the_default_bid_policy(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_BID", "auto")
    rnd = random.Random(15)
    data = b"".join(rnd.choice([b"alpha ", b"beta ", b"gamma ", b"delta "]) + rnd.randbytes(3) for _ in range(200000))
    assert len(data) > 1 << 20
    rc, img = write_zstd(data)
    assert rc == ARCHIVE_OK
    r = la_api.cat(img)
    assert r.filters[0] == (14, "zstd") and r.data == data and r.rc == la_api.ARCHIVE_EOF


def test_zstd_write_filter_errors(gpu_ctx):
    rc, err = write_zstd(b"abc", (("no-such-option", "1"),))
    assert rc == ARCHIVE_FAILED and "Undefined option" in err
    rc, err = write_zstd(b"abc", (("compression-level", "23"),))
    assert rc == ARCHIVE_FAILED and "Undefined option" in err
    rc, err = write_zstd(random.Random(1).randbytes(200000), (), None, cap=100)     # the client's buffer is too small
    assert rc == ARCHIVE_FATAL and err == "Buffer exhausted"
