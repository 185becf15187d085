"""The bzip2 read filter on the device (la_filter_bzip2.c over la_bzip2.hip) against the reference's read loop over
libbz2 (bzip2_support.reference_cat): verdict, message and delivered bytes are the reference's for valid, concatenated,
cut and damaged streams.  The one exception is a flip of a block's randomised bit (libbz2 still decodes such blocks,
the device refuses them): those flips are told by position, counted, and only have to be a data error."""
import bz2
import random

import pytest

import bzip2_support as BS
import la_api

pytestmark = pytest.mark.gpu

ARCHIVE_FILTER_BZIP2 = 2
FLIP_GROUPS = 10


def same_as_reference(image, read_size=None):
    ref = BS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == (ARCHIVE_FILTER_BZIP2, "bzip2")
    return res


@pytest.mark.parametrize("read_size", [None, 1000])
def test_fixtures(gpu_ctx, read_size):
    for m, img in BS.fixtures():
        res = same_as_reference(img, read_size)
        assert len(res.data) == (29 if m["file"] == "test_expand.bz2" else m["decoded_size"]), m["file"]


@pytest.mark.parametrize("name", sorted(BS.filter_shapes()))
def test_shapes(gpu_ctx, name):
    res = same_as_reference(BS.filter_shapes()[name])
    assert res.filters[0] == (ARCHIVE_FILTER_BZIP2, "bzip2")


@pytest.mark.parametrize("serial", ["0", "1"])
def test_zeros_split_by_the_budget(gpu_ctx, monkeypatch, serial):
    """20 MB of zeros are four blocks of 5 MB at level 1: with a budget of 8 MiB of decoded bytes a window emits one
    block and carries the rest, stream state and bit offset included"""
    monkeypatch.setenv("LA_GPU_OUT_BUDGET_MIB", "8")
    monkeypatch.setenv("LA_BZIP2_SERIAL_CHASE", serial)
    img = bz2.compress(bytes(20000000), 1)
    assert len([1 for _, k in BS.find_magics(img) if k == 0]) == 4
    res = la_api.cat(img)
    assert la_api.as_reference_tuple(res) == (bytes(20000000), 0, "")
    assert max(res.block_sizes) <= 8 << 20


def test_level_9_block(gpu_ctx):
    same_as_reference(bz2.compress(BS.noise(9, 950000, 50), 9))


@pytest.mark.parametrize("part", range(6))
def test_cut_at_every_byte(gpu_ctx, part):
    img = BS.stream3000()
    for cut in range(14 + part, len(img), 6):
        same_as_reference(img[:cut])


@pytest.mark.parametrize("part", range(4))
def test_cuts_of_the_long_stream(gpu_ctx, part):
    img = BS.stream350k()
    r = random.Random(200)
    cuts = [r.randrange(14, len(img)) for _ in range(200)]
    for cut in cuts[part::4]:
        same_as_reference(img[:cut])


def flip_plan():
    """2 000 seeded flips spread over both streams (the first 80 bits are the bidder's: a flip there and no bzip2
    filter is created), plus the randomised bit of every block, so that the exception is met on purpose"""
    big, small = BS.stream350k(), BS.stream3000()
    r = random.Random(2000)
    flips = [("small", r.randrange(80, len(small) * 8)) for _ in range(1800)] + [("big", r.randrange(80, len(big) * 8)) for _ in range(200)]
    special = {("small", b) for b in BS.randomised_bits(small)} | {("big", b) for b in BS.randomised_bits(big)}
    assert len(special) == 5
    flips += sorted(special)
    r.shuffle(flips)
    return {"big": big, "small": small}, flips, special


@pytest.mark.parametrize("group", range(FLIP_GROUPS))
def test_single_bit_flips(gpu_ctx, group):
    images, flips, special = flip_plan()
    mine = flips[group::FLIP_GROUPS]
    skipped = 0
    for which, bit in mine:
        img = BS.flip(images[which], bit)
        if (which, bit) in special:
            skipped += 1
            res = la_api.cat(img)
            assert (res.rc, res.error) == (la_api.ARCHIVE_FATAL, "bzip decompression failed")
            continue
        same_as_reference(img)
    assert skipped == len([f for f in mine if f in special])


def test_the_exception_is_met(gpu_ctx):
    _, flips, special = flip_plan()
    assert len([f for f in flips if f in special]) >= 5


def test_tar_walk_over_the_fixtures(gpu_ctx):
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
