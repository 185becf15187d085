"""The uu read filter on the device (la_filter_uu.c over la_uu.hip) against the oracle (uu_support.reference_cat):
verdict, message and delivered bytes for valid, multi-section, junk and damaged streams; the reference's two fixtures
through la_api.cat and la_cat; tarballs behind mail-style preambles through the tar reader."""
import gzip
import hashlib
import os
import subprocess

import pytest

import la_api
import uu_support as U
from test_host_uu_mock import tar_gz, windows_stream

pytestmark = pytest.mark.gpu

UU = (U.ARCHIVE_FILTER_UU, "uu")
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")
GROUPS = 4


def same_as_reference(image, read_size=None):
    ref = U.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:
        assert (res.filters[0] == UU) == (U.bid(image) > 0)
    return res


@pytest.mark.parametrize("read_size", [None, 1000])
@pytest.mark.parametrize("group", range(GROUPS))
def test_shapes(gpu_ctx, group, read_size):
    for name in sorted(U.filter_shapes())[group::GROUPS]:
        same_as_reference(U.filter_shapes()[name], read_size)


def test_fixtures(gpu_ctx):
    env = dict(os.environ)
    for m, img in U.fixtures():
        res = same_as_reference(img)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters == [UU, (0, "none")], m["file"]
        assert res.pathname == m["pathname"]
        assert len(res.data) == m["decoded_size"] and hashlib.sha256(res.data).hexdigest() == m["decoded_sha256"]
        run = subprocess.run([os.path.join(HOST, "la_cat"), os.path.join(U.FIXTURE_DIR, m["file"])], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0 and run.stdout == res.data, (m["file"], run.stderr[-500:])


@pytest.mark.parametrize("lead", [0, 1, 65536])
def test_tar_gz_behind_a_preamble(gpu_ctx, monkeypatch, lead):
    monkeypatch.setenv("LA_GPU_BID", "all")
    tgz, names = tar_gz()
    for img in (U.uu_section(tgz, name=b"x.tar.gz"), U.b64_section(tgz, name=b"x.tar.gz")):
        res = la_api.list_entries(U.preamble(lead) + img)
        assert res.open_rc == 0 and res.rc == la_api.ARCHIVE_EOF, res.error
        assert res.filters == [(1, "gzip"), UU, (0, "none")]
        assert [e[0] for e in res.entries] == names and res.entries[1][5] == U.randbytes(1, 2000)


def test_512_kib_of_preamble_is_not_bid_for(gpu_ctx):
    tgz, _ = tar_gz()
    res = la_api.list_entries(U.preamble(512 << 10) + U.uu_section(tgz, name=b"x.tar.gz"))
    assert res.open_rc != 0 and not res.entries


def test_3_mib_under_windows_of_1_mib(gpu_ctx, monkeypatch):
    """a line across every window edge, a '\\r' | '\\n' split on the first, a second header in the second window; then a
    damaged line in the third window: all bytes in front come out and then the message"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    img, plain = windows_stream()
    res = same_as_reference(img)
    assert res.data == plain and res.rc == la_api.ARCHIVE_EOF and res.filters[0] == UU
    at = img.index(b"\n", (2 << 20) + 300000) + 1
    res = same_as_reference(img[:at + 5] + b"*" + img[at + 6:])
    assert res.rc == la_api.ARCHIVE_FATAL and res.error == U.E_INSUFFICIENT and res.data == plain[:len(res.data)]
    assert len(res.data) > 45 * 18000 + 500000


def test_binary_junk_behind_end_is_ignored(gpu_ctx):
    data = U.randbytes(77, 5000)
    for img in (U.uu_section(data), U.b64_section(data)):
        res = same_as_reference(img + U.randbytes(78, 100000))
        assert res.rc == la_api.ARCHIVE_EOF and res.data == data


def test_look_ahead_over_another_filter(gpu_ctx, monkeypatch):
    """over another filter the bidder asks for no more than that filter has handed out: text in front of an lz4 content
    checksum error still comes out; a .uu inside a .gz is found behind 100 KiB of preamble"""
    import streams as S
    monkeypatch.setenv("LA_GPU_BID", "all")
    text = b"".join(b"line %d of a text that ends with its stream\n" % i for i in range(40))
    img, _ = S.lz4_frame([(text, S.lz4_block(text, stored=True))], bad_content=True)
    res = la_api.cat(img)
    assert la_api.as_reference_tuple(res) == (text, -30, "lz4 stream checksum error") and UU not in res.filters
    data = U.randbytes(5, 3000)
    for lead in (0, 100000):
        res = la_api.cat(gzip.compress(U.preamble(lead) + U.uu_section(data), mtime=0))
        assert res.filters == [UU, (1, "gzip"), (0, "none")] and res.data == data and res.rc == la_api.ARCHIVE_EOF
