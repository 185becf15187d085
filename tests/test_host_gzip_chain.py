"""CPU-only: the LA_GZIP_FLUSH_POINTS switch of the gzip read filter and its bid policy (la_bid_policy.c).  `1` and
`chain` both turn piece mode on, with the same bid evidence; `chain` alone says that the pieces may depend on each other
(the filter then decodes them with LA_GZ_OPT_CHAIN).

Checked here with zlib: the Z_SYNC_FLUSH stream below is one a decoder cannot enter at its second flush point ("invalid
distance too far back"), i.e. one that =1 takes on the same evidence and then has to give up on."""
import ctypes as C
import random
import zlib

import pytest

from libarchive_amd import _native as N

MARKER = b"\x00\x00\xff\xff"
HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03"


def _lib():
    lib = N.host_lib()
    lib.la_bid_gzip_parallel.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t]
    return lib


@pytest.mark.parametrize("value, on, chain", [(None, 0, 0), ("0", 0, 0), ("1", 1, 0), ("chain", 1, 1), ("", 0, 0),
                                              ("chained", 0, 0), ("c", 0, 0)])
def test_switch_values(monkeypatch, value, on, chain):
    if value is None:
        monkeypatch.delenv("LA_GZIP_FLUSH_POINTS", raising=False)
    else:
        monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", value)
    lib = _lib()
    assert (lib.la_gz_flush_points_enabled(), lib.la_gz_flush_points_chain()) == (on, chain)


def sync_flush_stream(size=2_400_000, step=30_000):
    r = random.Random(5)
    words = [b"window", b"piece", b"flush", b"marker", b"deflate", b"stored", b"lane", b"wave"]
    plain = b" ".join(r.choice(words) for _ in range(size // 4))
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    spans = [c.compress(plain[i:i + step]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(plain), step)]
    return HEADER + b"".join(spans) + c.flush(), spans


def test_bid_takes_a_sync_flush_stream_on_the_same_evidence(monkeypatch):
    img, spans = sync_flush_stream()
    look = 256 << 10
    assert len(img) > look and img[:look].count(MARKER) >= 4 and all(len(s) < (128 << 10) for s in spans)
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        zlib.decompressobj(-15).decompress(spans[1])
    lib = _lib()
    bid = lambda s: lib.la_bid_gzip_parallel(s, len(s), len(HEADER), look)
    few = HEADER + spans[0] + spans[1] + random.Random(6).randbytes(300 << 10).replace(b"\xff\xff", b"\xff\xfe").replace(b"\x1f\x8b", b"\x1f\x8c")
    assert few[:look].count(MARKER) == 2
    answers = {}
    for value in (None, "0", "1", "chain"):
        if value is None:
            monkeypatch.delenv("LA_GZIP_FLUSH_POINTS", raising=False)
        else:
            monkeypatch.setenv("LA_GZIP_FLUSH_POINTS", value)
        answers[value] = (bid(img[:look]), bid(few[:look]))
    assert answers[None] == answers["0"] == (0, 0)
    assert answers["1"] == answers["chain"] == (1, 0)     # four markers close together; two are not enough
