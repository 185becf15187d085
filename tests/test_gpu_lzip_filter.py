"""The lzip read filter on the device (la_filter_lzip.c over la_lzip.hip) against the reference's read loop over liblzma
(lzip_support.reference_cat): verdict, message and delivered bytes are the reference's for valid, multi-member, cut and
damaged streams, hand-built LZMA streams included; the fixtures go through la_cat and la_tarwalk as well."""
import os
import subprocess

import pytest

import la_api
import lzip_support as LS

pytestmark = pytest.mark.gpu

LZIP = (LS.ARCHIVE_FILTER_LZIP, "lzip")
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")
FLIP_GROUPS = 4


def same_as_reference(image, read_size=None):
    ref = LS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == LZIP
    return res


@pytest.mark.parametrize("name", sorted(LS.filter_shapes()))
def test_shapes(gpu_ctx, name):
    same_as_reference(LS.filter_shapes()[name])


@pytest.mark.parametrize("read_size", [None, 1000])
def test_fixtures(gpu_ctx, read_size):
    for m, img in LS.fixtures():
        res = same_as_reference(img, read_size)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZIP, m["file"]


def test_la_cat_and_la_tarwalk(gpu_ctx):
    """the two programs over the fixture files: liblzma's bytes, and the entry names test_compat_lzip.c walks"""
    env = dict(os.environ, LA_GPU_BID="auto")
    for m, img in LS.fixtures():
        path = os.path.join(LS.FIXTURE_DIR, m["file"])
        if not m["entries"]:
            run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
            assert run.returncode == 0 and run.stdout == LS.reference_read(img)[0], (m["file"], run.stderr[-500:])
            continue
        run = subprocess.run([os.path.join(HOST, "la_tarwalk"), "-v", path], capture_output=True, text=True, env=env, timeout=120)
        assert run.returncode == 0, run.stderr[-500:]
        lines = run.stdout.splitlines()
        assert [ln.split("\t")[0] for ln in lines[:-1]] == m["entries"], run.stdout
        assert lines[-1].endswith("filter lzip")


def test_cuts(gpu_ctx):
    img = LS.member(LS.text(1, 5000)) + LS.member(LS.noise(2, 700, 16))
    for cut in range(6, len(img), 23):
        same_as_reference(img[:cut])


@pytest.mark.parametrize("group", range(FLIP_GROUPS))
def test_single_bit_flips(gpu_ctx, group):
    img = LS.three()[0]
    for bit in LS.flip_cases()[group::FLIP_GROUPS * 3]:
        same_as_reference(LS.flip(img, bit))


def test_small_windows(gpu_ctx, monkeypatch):
    """windows of 1 MiB over 2.4 MiB of noise in members of 300 000 bytes: a member straddles every window boundary"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    img = b"".join(LS.member(LS.noise(62 + i, 300000), preset=0, version=i % 3 != 2) for i in range(8))
    assert len(img) > 2 << 20
    same_as_reference(img)


def test_more_header_shapes_than_one_scan_keeps(gpu_ctx):
    """66 000 members of 0 and 1 bytes in one window: the scan's table of 65 536 candidates is filled and the rest is
    scanned in a second part; the launch table of 4096 is filled sixteen times"""
    one, none = LS.member(b"x"), LS.member(b"")
    res = same_as_reference(b"".join(none if i % 3 else one for i in range(66000)))
    assert len(res.data) == 22000


def test_bid_policy(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "4")
    t = LS.noise(80, 9000)
    two, one_long = LS.member(t[:3000]) + LS.member(t[3000:]), LS.member(t)
    monkeypatch.setenv("LA_GPU_BID", "auto")
    res = la_api.cat(two)
    assert res.filters[0] == LZIP and res.data == t
    declined = la_api.cat(one_long)
    assert LZIP not in declined.filters and declined.data == one_long
    monkeypatch.setenv("LA_GPU_BID", "all")
    for img in (two, one_long):
        res = la_api.cat(img)
        assert res.filters[0] == LZIP and res.data == t
