"""The lzop read filter's HOST side (la_filter_lzop.c: consume_header and consume_block_info restated, parts and junk,
the stale checksum, windows, the carry of the unfinished block, the blocks handed out in front of an error) over a CPU
stand-in for la_gpu_lzop_decode (tests/mock_gpu/la_gpu_lzop_mock.c: the kernel's own rules header, compiled for the host).  la_api.cat
through the mock library must equal the reference's read loop over the Python decoder (lzop_support.reference_read) on
bytes, return code, error string and filter code / name."""

import pytest

import la_api
import mock_build
import lzop_support as L

LZOP = (L.ARCHIVE_FILTER_LZOP, "lzop")


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def same_as_reference(image, read_size=None):
    ref = L.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == LZOP
    return res


@pytest.mark.parametrize("name", sorted(L.filter_shapes()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_shapes(mock, name, read_size):
    same_as_reference(L.filter_shapes()[name], read_size)


def test_the_shapes_end_as_their_names_say():
    """the reference's own verdicts on the shapes: the table the filter is held against above is not all one kind"""
    sh = L.filter_shapes()
    end = lambda n: L.reference_read(sh[n])[1:]      # noqa: E731
    assert end("empty_part_short") == (L.ARCHIVE_FAILED, L.E_TRUNCATED) and end("empty_part") == (0, "")
    assert end("required_version_08ff") == (L.ARCHIVE_FAILED, L.E_VERSION) and end("required_version_0900") == (0, "")
    assert end("method_0") == end("method_4") == (L.ARCHIVE_FAILED, L.E_METHOD) and end("method_3") == (0, "")
    assert end("level_10") == (L.ARCHIVE_FAILED, L.E_LEVEL) and end("level_9") == end("level_10_old_version") == (0, "")
    assert end("bad_header_checksum") == end("bad_header_crc32") == end("block_above_64_mib") == (L.ARCHIVE_FAILED, L.E_HEADER)
    assert end("compressed_above_uncompressed") == (L.ARCHIVE_FAILED, L.E_HEADER)
    assert end("block_truncated") == (L.ARCHIVE_FATAL, L.E_TRUNCATED) and end("no_closing_word") == (L.ARCHIVE_FAILED, L.E_TRUNCATED)
    assert end("extra_field_runs_off_the_stream") == (L.ARCHIVE_FAILED, L.E_TRUNCATED)
    assert end("stale_sum_fails") == end("stale_sum_first_block_is_compared_with_0") == end("stale_sum_crc32_fails") == (L.ARCHIVE_FATAL, L.E_DATA)
    assert end("stale_sum_of_the_block_in_front_passes") == end("stale_sum_carries_over_a_part") == (0, "")
    assert len(L.reference_read(sh["stale_sum_fails"])[0]) == 900       # the block in front of the stored one is out
    for f in L.SUM_FLAGS:
        # (a stored block carries one word at most, of the *_UNCOMPRESSED kind; where the *_COMPRESSED flag asks for none or
        # for the other kind, a writer's stream fails at its first stored block: the stale checksum)
        ckind = "crc" if f & L.CC else "adler" if f & L.AC else None
        ukind = "crc" if f & L.CU else "adler" if f & L.AU else None
        stale = ckind is not None and ckind != ukind
        assert end("flags_%04x" % f) == (0, "") and end("stored_flags_%04x" % f) == ((L.ARCHIVE_FATAL, L.E_DATA) if stale else (0, ""))
    for name, code in (("lookbehind_by_one", -6), ("output_overrun_match", -5), ("input_overrun_no_marker", -4), ("not_consumed", -8)):
        assert end("handbuilt_" + name) == end("handbuilt_first_" + name) == (L.ARCHIVE_FATAL, L.E_LZO % code)
        assert len(L.reference_read(sh["handbuilt_" + name])[0]) == 5000 and L.reference_read(sh["handbuilt_first_" + name])[0] == b""
    assert end("handbuilt_short_output") == (L.ARCHIVE_FATAL, L.E_DATA)
    assert end("bad_sum_u_flags_0001_block_0") == end("bad_sum_c_flags_0200_block_2") == (L.ARCHIVE_FATAL, L.E_DATA)
    assert end("bad_sum_u_flags_0001_block_1") == (0, "")       # a stored block's word is not looked at without a *_COMPRESSED flag
    assert end("bad_sum_u_flags_0303_block_1") == (L.ARCHIVE_FATAL, L.E_DATA)     # with one it is, as the compressed sum
    assert end("junk_is_a_bare_magic") == (L.ARCHIVE_FAILED, L.E_TRUNCATED) and end("junk_is_most_of_a_magic") == (0, "")
    assert L.reference_cat(sh["nested"])[0] == L.text(1, 5000)


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_fixtures(mock, read_size):
    for m, img in L.fixtures():
        res = same_as_reference(img, read_size)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZOP, m["file"]
        assert len(res.data) == m["decoded_size"], m["file"]


def test_tar_walk_over_the_fixtures(mock):
    for m, img in L.fixtures():
        if m["entries"]:
            res = la_api.list_entries(img)
            assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZOP, res.error
            assert [e[0] for e in res.entries] == m["entries"]


def test_cut_at_every_byte(mock):
    img = L.part(L.text(1, 3000), block_size=1200, flags=L.AU | L.AC, name=b"a name") + L.part(L.noise(2, 300, 16), flags=L.CC | L.EXTRA_FIELD, version=0x0930)
    assert 1500 < len(img) < 3000
    for cut in range(9, len(img)):
        same_as_reference(img[:cut])


def test_single_bit_flips(mock):
    img = L.header(flags=L.AU | L.AC, name=b"nm") + L.block(L.text(1, 1500), L.AU | L.AC) + L.block(L.noise(2, 200), L.AU | L.AC) + L.block(L.text(3, 1000), L.AU | L.AC) + bytes(4)
    for bit in L.flip_cases(img, 29 + 2 + 4 + 16):
        same_as_reference(L.flip(img, bit))
    # without checksums a flipped bit reaches the decoder: every verdict of the rules has to come out as the reference words it
    img = L.header(flags=0) + L.block(L.text(1, 1500), 0) + L.block(L.text(3, 1000), 0) + bytes(4)
    for bit in L.flip_cases(img, 40):
        same_as_reference(L.flip(img, bit))


def stored_block_to(total, seed):
    """a stored block whose image (8 bytes of sizes, one checksum word, the data) is `total` bytes long"""
    data = L.randbytes(seed, total - 12)
    b = L.block(data, L.AU, stored=True)
    assert len(b) == total
    return b


def test_window_edges(mock, monkeypatch):
    """windows of 1 MiB: a block that ends exactly at the first window's edge, then blocks that straddle every edge; cut
    and damaged copies"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    head = L.header() + L.block(L.text(1, 200000), L.AU)
    img = head + stored_block_to((1 << 20) - len(head), 61)
    assert len(img) == 1 << 20
    img += b"".join(stored_block_to(300000 + 7 * i, 62 + i) if i % 3 else L.block(L.text(i, 400000), L.AU) for i in range(9))
    img += bytes(4)
    assert len(img) > 3 << 20
    same_as_reference(img)
    same_as_reference(img[:1 << 20])
    same_as_reference(img[:(1 << 20) + 3])
    same_as_reference(img[:(1 << 20) + 9])
    same_as_reference(img[:len(img) - 100000])
    same_as_reference(L.flip(img, (2 << 20) * 8 + 5))
    same_as_reference(img[:-4] + L.part(b"a second part behind the windows"))


def test_more_blocks_than_one_launch_takes(mock):
    img = L.part(L.text(9, 9000), block_size=1)
    res = same_as_reference(img)
    assert len(res.data) == 9000
    same_as_reference(L.flip(img, (len(img) - 30) * 8))        # a damaged block in the third launch


def test_a_block_larger_than_the_window_limit_is_refused_by_name(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    res = la_api.cat(L.header() + stored_block_to(1200000, 70) + L.block(b"x") + bytes(4))
    assert res.rc == la_api.ARCHIVE_FATAL and "lzop block too large for the GPU data plane" in res.error, res.error


def test_bid_policy(mock, monkeypatch):
    """auto: taken when the look-ahead holds the whole stream or the first block ends inside it; a first block longer
    than the look-ahead is declined.  all: everything with the magic."""
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "4")
    t = L.noise(80, 9000)
    two = L.header() + L.block(t[:3000], stored=True) + L.block(t[3000:], stored=True) + bytes(4)
    long_first = L.header() + L.block(t[:6000], stored=True) + L.block(t[6000:], stored=True) + bytes(4)
    one_long = L.header() + L.block(t, stored=True) + bytes(4)
    small = L.part(t[:1000])
    extra = L.header(flags=L.AU | L.EXTRA_FIELD | L.FILTER, extra=bytes(100)) + L.block(t[:3000], stored=True) + L.block(t[3000:], stored=True) + bytes(4)
    assert len(small) < 4096 < len(two)
    monkeypatch.setenv("LA_GPU_BID", "auto")
    for img, plain in ((two, t), (small, t[:1000]), (extra, t)):
        res = la_api.cat(img)
        assert res.filters[0] == LZOP and res.data == plain
    for img in (long_first, one_long):
        declined = la_api.cat(img)
        assert LZOP not in declined.filters and declined.data == img
    monkeypatch.setenv("LA_GPU_BID", "all")
    for img in (two, long_first, one_long, small, extra):
        res = la_api.cat(img)
        assert res.filters[0] == LZOP and res.rc == la_api.ARCHIVE_EOF and res.data == t[:len(res.data)]
