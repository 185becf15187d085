"""The gzip read filter's block-start mode on the device (LA_GZIP_BLOCK_STARTS=1: la_filter_gzip.c over la_inflate_find.hip
and the chain kernels) against the reference filter over zlib (oracle_lib.gzip_stream_decode): the streams of
tests/deflate_find_support.filter_streams() give its bytes, return code and error string, in one window and in many (the
span of one device call held to 40 000 bytes: windows that begin in mid-byte, the carried history, spans that have to
grow); la_cat takes a lone member under the product's own bid policy when the switch is on."""
import os
import subprocess

import pytest

import deflate_find_support as F
import la_api
import oracle_lib as O

pytestmark = pytest.mark.gpu

ARCHIVE_FILTER_GZIP = 1
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")
STREAMS = sorted(F.filter_streams())


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setenv("LA_GZIP_BLOCK_STARTS", "1")
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "16")
    monkeypatch.setenv("LA_GPU_BID", "auto")        # (the suite's default is "all": here the bid policy itself takes the member)


def reference(image):
    ref, res = O.gzip_stream_decode(image, 4 << 20)
    return ref.tobytes(), res.rc, res.errmsg.decode()


def same_as_reference(image, read_size=None):
    want = reference(image)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(want[0]), want[1], want[2])
    assert got[0] == want[0]
    assert res.filters[0] == (ARCHIVE_FILTER_GZIP, "gzip")
    return res


@pytest.mark.parametrize("name", STREAMS)
def test_streams_in_one_window(gpu_ctx, switch_on, name):
    same_as_reference(F.filter_streams()[name])


@pytest.mark.parametrize("name", STREAMS)
def test_streams_in_many_windows(gpu_ctx, switch_on, monkeypatch, name):
    monkeypatch.setenv("LA_GZ_TEST_BLOCKS_WINDOW", "40000")
    same_as_reference(F.filter_streams()[name], 1000 if name.startswith("text-level-6") else None)


@pytest.mark.parametrize("name", ["wrong-crc32", "wrong-isize"])
def test_trailer_is_compared_under_strict(gpu_ctx, switch_on, monkeypatch, name):
    monkeypatch.setenv("LA_GZIP_STRICT", "1")
    monkeypatch.setenv("LA_GZ_TEST_BLOCKS_WINDOW", "40000")
    good = reference(F.filter_streams()["text-level-6"])
    res = la_api.cat(F.filter_streams()[name])
    assert res.rc == la_api.ARCHIVE_FATAL and 0 < len(res.data) < len(good[0]) and good[0].startswith(res.data)
    assert ("CRC" in res.error) if name == "wrong-crc32" else ("ISIZE" in res.error or "size" in res.error.lower())
    res = la_api.cat(F.filter_streams()["text-level-6"])
    assert (res.rc, res.data) == (la_api.ARCHIVE_EOF, good[0])


def test_la_cat_takes_a_lone_member_when_the_switch_is_on(gpu_ctx, tmp_path):
    """a 1 MiB .gz of one member, LA_GPU_BID not set: with the switch the gzip filter bids and decodes it; without it the
    bid policy leaves it alone and the bytes pass as they are"""
    plain = F.word_text(9 << 19, seed=31)        # (4.5 MiB of this text: a little above 1 MiB compressed)
    image = F.gz_member(F.raw_deflate(plain, 6), plain)
    assert len(image) >= 1 << 20
    path = str(tmp_path / "lone.gz")
    with open(path, "wb") as f:
        f.write(image)
    env = {k: v for k, v in os.environ.items() if k not in ("LA_GPU_BID", "LA_GZIP_BLOCK_STARTS")}
    run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=dict(env, LA_GZIP_BLOCK_STARTS="1"), timeout=120)
    assert run.returncode == 0 and run.stdout == plain, run.stderr[-500:]
    run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
    assert run.returncode == 0 and run.stdout == image, run.stderr[-500:]
