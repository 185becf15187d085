"""The bzip2 read filter's HOST side (la_filter_bzip2.c: windows, carry of the unfinished unit and the stream state, the
decoded-bytes budget, the bytes held back in front of an error, verdicts and strings) over a CPU stand-in for
la_gpu_bzip2_scan / la_gpu_bzip2_decode (tests/mock_gpu/la_gpu_bzip2_mock.c: the real libbz2, one block at a time).  la_api.cat through
the mock library must equal the reference's read loop over libbz2 (bzip2_support.reference_read) on bytes, return
code, error string and filter code / name."""
import random

import pytest

import bzip2_support as BS
import la_api
import mock_build

ARCHIVE_FILTER_BZIP2 = 2


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def same_as_reference(image, read_size=None):
    ref = BS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == (ARCHIVE_FILTER_BZIP2, "bzip2")
    return res


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_fixtures(mock, read_size):
    for m, img in BS.fixtures():
        res = same_as_reference(img, read_size)
        # one filter's output is what the manifest records; test_expand.bz2 holds a second stream inside the first
        assert len(res.data) == (29 if m["file"] == "test_expand.bz2" else m["decoded_size"]), m["file"]


@pytest.mark.parametrize("name", sorted(BS.filter_shapes()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_shapes(mock, name, read_size):
    img = BS.filter_shapes()[name]
    res = same_as_reference(img, read_size)
    assert res.filters[0] == (ARCHIVE_FILTER_BZIP2, "bzip2")


def test_small_windows(mock, monkeypatch):
    """windows of 1 MiB: a stream of several MiB is taken in several windows, units carried from one to the next"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    img = b"".join(__import__("bz2").compress(BS.noise(40 + i, 700000), 1) for i in range(4))
    assert len(img) > 2 << 20
    same_as_reference(img)
    same_as_reference(img[:len(img) - 100000])


def test_budget_splits_a_window(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_OUT_BUDGET_MIB", "1")
    img = __import__("bz2").compress(bytes(3 << 20) + BS.letters(1, 2000), 1)
    same_as_reference(img)


def test_cut_at_every_byte(mock):
    img = BS.stream3000()
    for cut in range(14, len(img)):
        same_as_reference(img[:cut])


def test_cuts_of_the_long_stream(mock):
    img = BS.stream350k()
    r = random.Random(200)
    for _ in range(60):
        same_as_reference(img[:r.randrange(14, len(img))])


def test_single_bit_flips(mock):
    """the first 80 bits are the bidder's: a flip there and no bzip2 filter is created at all"""
    r = random.Random(2000)
    big, small = BS.stream350k(), BS.stream3000()
    for _ in range(150):
        same_as_reference(BS.flip(big, r.randrange(80, len(big) * 8)))
    for _ in range(350):
        same_as_reference(BS.flip(small, r.randrange(80, len(small) * 8)))


def test_randomised_block_is_a_data_error(mock):
    img = BS.stream3000()
    (bit,) = BS.randomised_bits(img)
    res = la_api.cat(BS.flip(img, bit))
    assert la_api.as_reference_tuple(res) == (b"", -30, "bzip decompression failed")


def test_tar_walk_over_the_fixtures(mock):
    """.tar.bz2 through the tar walker (the bsdtar -t shape): names, sizes and bodies as Python's tarfile reads them"""
    import io
    import tarfile
    for m, img in BS.fixtures():
        if not m["file"].endswith((".tbz", ".tar.bz2")):
            continue
        data, rc, _ = BS.reference_read(img)
        assert rc == 0
        want = [(t.name, t.size, tf.extractfile(t).read() if t.isfile() else None)
                for tf in [tarfile.open(fileobj=io.BytesIO(data))] for t in tf.getmembers()]
        res = la_api.list_entries(img)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == (ARCHIVE_FILTER_BZIP2, "bzip2"), (m["file"], res.error)
        got = [(e[0].rstrip("/"), e[1], e[5] if e[2] == 0o100000 else None) for e in res.entries]
        assert got == [(n.rstrip("/"), s, b) for n, s, b in want], m["file"]
