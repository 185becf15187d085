"""The xz read filter on the device (la_filter_xz.c over la_xz.hip) against the reference's read loop over liblzma
(xz_support.reference_cat): verdict, message and delivered bytes are the reference's for valid, concatenated, cut and
damaged streams, hand-built LZMA2 data included; the fixtures go through la_cat and la_tarwalk as well."""
import lzma
import os
import subprocess

import pytest

import la_api
import xz_build as XB
import xz_support as XS

pytestmark = pytest.mark.gpu

ARCHIVE_FILTER_XZ = 6
CUT_PARTS, FLIP_GROUPS = 8, 12
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")


def same_as_reference(image, read_size=None):
    ref = XS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz")
    return res


@pytest.mark.parametrize("name", sorted(XS.filter_shapes()))
def test_shapes(gpu_ctx, name):
    same_as_reference(XS.filter_shapes()[name])


@pytest.mark.parametrize("read_size", [None, 1000])
def test_fixtures(gpu_ctx, read_size):
    for m, img in XS.fixtures():
        res = same_as_reference(img, read_size)
        assert len(res.data) == m["decoded_size"] and res.filters[0] == (ARCHIVE_FILTER_XZ, "xz"), m["file"]


def test_la_cat_and_la_tarwalk(gpu_ctx):
    """the two programs over the fixture files: liblzma's bytes for the threaded writer's and the single-block file, the
    entry names test_compat_xz.c walks for the .txz"""
    env = dict(os.environ, LA_GPU_BID="auto")
    for m, img in XS.fixtures():
        path = os.path.join(XS.FIXTURE_DIR, m["file"])
        run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
        assert run.returncode == 0 and run.stdout == lzma.decompress(img), (m["file"], run.stderr[-500:])
    m = XS.fixtures()[0][0]
    run = subprocess.run([os.path.join(HOST, "la_tarwalk"), "-v", os.path.join(XS.FIXTURE_DIR, m["file"])], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0, run.stderr[-500:]
    lines = run.stdout.splitlines()
    assert [ln.split("\t")[0] for ln in lines[:-1]] == m["entries"], run.stdout
    assert "6 entries" in lines[-1] and lines[-1].endswith("filter xz")


def test_hand_built_data(gpu_ctx):
    for name, (raw, plain) in list(XS.packet_cases().items()) + list(XS.chunk_plans().items()):
        assert same_as_reference(XS.wrap(raw, plain, XB.CHECK_CRC64)).data == plain, name
    for name, (raw, valid, ok, dict_byte) in XS.beyond_cases().items():
        res = same_as_reference(XS.wrap(raw, valid if ok else b"", dict_byte=dict_byte))
        assert (res.rc == la_api.ARCHIVE_EOF) == ok, name
    for name, (raw, _) in XS.refusals().items():
        assert same_as_reference(XS.wrap(raw)).error == XS.DATA_ERROR, name


def test_unsupported_filters_are_named(gpu_ctx):
    t = XS.text(5, 300)
    img = XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, extra_filters=[(0x04, b"")])], XB.CHECK_CRC32)
    res = la_api.cat(img)
    assert res.rc == la_api.ARCHIVE_FATAL and "unsupported filter x86 BCJ" in res.error, res.error


def test_small_windows(gpu_ctx, monkeypatch):
    """windows of 1 MiB over 3.6 MiB of noise in blocks of 300 000 bytes: a block straddles every window boundary"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    parts = [XS.noise(60 + i, 300000) for i in range(12)]
    for sizes in (True, False):
        img = XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC32, comp=sizes, uncomp=sizes) for p in parts], XB.CHECK_CRC32)
        assert len(img) > 3 << 20
        same_as_reference(img)
        same_as_reference(img[:len(img) - 100000])


def test_tail_over_several_windows(gpu_ctx, monkeypatch):
    """windows of 1 MiB that decode 20 000 bytes each: the held-back tail takes the bytes of three windows before the
    fourth crosses 64 KiB, and an error in the fourth drops all of them"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    for name, img in XS.padded_streams().items():
        data, _, msg = la_api.as_reference_tuple(same_as_reference(img))
        assert (len(data), msg) == XS.PADDED_STREAMS_RESULT[name], name


@pytest.mark.parametrize("part", range(CUT_PARTS))
def test_cut_at_every_byte(gpu_ctx, part):
    img = XS.stream3000()
    for cut in range(6 + part, len(img), CUT_PARTS):
        same_as_reference(img[:cut])


@pytest.mark.parametrize("group", range(FLIP_GROUPS))
def test_single_bit_flips(gpu_ctx, group):
    img = XS.stream3000()
    for bit in XS.flip_cases()[group::FLIP_GROUPS]:
        same_as_reference(XS.flip(img, bit))


def test_bid_policy(gpu_ctx, monkeypatch):
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "4")
    t = XS.noise(80, 9000)
    threaded = XB.stream([XB.block(XB.lzma2(t[:4500]), t[:4500], XB.CHECK_CRC64), XB.block(XB.lzma2(t[4500:]), t[4500:], XB.CHECK_CRC64)], XB.CHECK_CRC64)
    plain_xz = lzma.compress(t)
    assert len(threaded) > 4096 and len(plain_xz) > 4096
    monkeypatch.setenv("LA_GPU_BID", "auto")
    res = la_api.cat(threaded)
    assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz") and res.data == t
    declined = la_api.cat(plain_xz)
    assert (ARCHIVE_FILTER_XZ, "xz") not in declined.filters and declined.data == plain_xz
    monkeypatch.setenv("LA_GPU_BID", "all")
    for img in (threaded, plain_xz):
        res = la_api.cat(img)
        assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz") and res.data == t
