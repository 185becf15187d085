"""The lzip read filter's HOST side (la_filter_lzip.c: the chain of members by their trailers, members decoded alone,
windows, the carry of the unfinished member, the bytes held back in front of an error, lzip_tail's verdicts) over CPU
stand-ins for la_gpu_lzip_scan / la_gpu_lzip_decode (tests/mock_gpu/la_gpu_lzip_mock.c: the kernel's own rules headers, compiled for the
host).  la_api.cat through the mock library must equal the reference's read loop over liblzma
(lzip_support.reference_read) on bytes, error string and filter code / name."""

import pytest

import la_api
import mock_build
import lzip_support as LS

LZIP = (LS.ARCHIVE_FILTER_LZIP, "lzip")


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def same_as_reference(image, read_size=None):
    ref = LS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == LZIP
    return res


# the member's bytes are a multiple of 64 KiB there and the error sits behind them: with 1-byte reads the reference sees
# it in a call of its own (la_filter_lzip.c's head comment names the assumption)
WHOLE_READS_ONLY = {"bad_crc_at_64k", "bad_crc_at_128k"}


@pytest.mark.parametrize("name", sorted(LS.filter_shapes()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_shapes(mock, name, read_size):
    if read_size == 1 and name in WHOLE_READS_ONLY:
        read_size = 65536
    same_as_reference(LS.filter_shapes()[name], read_size)


def test_the_shapes_end_as_their_names_say():
    """the reference's own verdicts on the shapes: the table the filter is held against above is not all one kind"""
    sh = LS.filter_shapes()
    end = lambda n: LS.reference_read(sh[n])[1:]      # noqa: E731
    a, b, c = LS.three()[2]
    for k in range(3):
        assert end("patched_crc_member_%d" % k) == (LS.ARCHIVE_FAILED, LS.E_CRC)
        assert end("patched_data_size_member_%d" % k) == (LS.ARCHIVE_FAILED, LS.E_SIZE)
        assert end("patched_member_size_member_%d" % k) == (LS.ARCHIVE_FAILED, LS.E_MEMBER)
        assert end("patched_member_size_small_member_%d" % k) == (LS.ARCHIVE_FAILED, LS.E_MEMBER)
    assert end("member_1_size_reaches_back") == (LS.ARCHIVE_FAILED, LS.E_MEMBER)
    assert LS.reference_read(sh["member_1_size_reaches_back"])[0] == a
    assert LS.reference_read(sh["version_0_between"]) == (a + b + c, 0, "")
    assert LS.reference_read(sh["junk_contains_a_header_shape"]) == (LS.text(5, 20000), 0, "")
    assert end("junk_begins_with_a_header")[0] == LS.ARCHIVE_FATAL and end("junk_is_a_bare_header") == (LS.ARCHIVE_FATAL, LS.BUF_ERROR)
    assert end("handbuilt_distance_past_the_data") == (LS.ARCHIVE_FATAL, LS.DATA_ERROR)
    assert end("handbuilt_no_marker")[0] == LS.ARCHIVE_FATAL


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_fixtures(mock, read_size):
    for m, img in LS.fixtures():
        res = same_as_reference(img, read_size)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZIP, m["file"]
        if not m["entries"]:
            assert len(res.data) == m["decoded_size"], m["file"]


def test_tar_walk_over_the_fixtures(mock):
    for m, img in LS.fixtures():
        if m["entries"]:
            res = la_api.list_entries(img)
            assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZIP, res.error
            assert [e[0] for e in res.entries] == m["entries"]


def test_cut_at_every_byte(mock):
    img = LS.member(LS.text(1, 5000)) + LS.member(LS.noise(2, 700, 16))
    for cut in range(6, len(img)):
        same_as_reference(img[:cut])
    v0 = LS.member(LS.text(1, 900), version=0) + LS.member(LS.noise(2, 300, 16))
    for cut in range(6, len(v0), 3):
        same_as_reference(v0[:cut])


def test_single_bit_flips(mock):
    img = LS.three()[0]
    for bit in LS.flip_cases():
        same_as_reference(LS.flip(img, bit))


def exact_member(target, seed):
    """a member of noise whose image is exactly `target` bytes long"""
    n = target - 26 - target // 60
    for _ in range(200):
        m = LS.member(LS.noise(seed, n), preset=0)
        if len(m) == target:
            return m
        n += target - len(m)
    raise AssertionError("no member of %d bytes found" % target)


def test_window_edges(mock, monkeypatch):
    """windows of 1 MiB: a member that ends exactly at the first window's edge, then members that straddle every edge;
    cut and damaged copies"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    first = LS.member(LS.noise(60, 300000), preset=0)
    img = first + exact_member((1 << 20) - len(first), 61)
    assert len(img) == 1 << 20
    img += b"".join(LS.member(LS.noise(62 + i, 300000), preset=0, version=i % 3 != 2) for i in range(8))
    assert len(img) > 3 << 20
    same_as_reference(img)
    same_as_reference(img[:1 << 20])
    same_as_reference(img[:(1 << 20) + 3])
    same_as_reference(img[:len(img) - 100000])
    same_as_reference(LS.flip(img, (2 << 20) * 8 + 5))


def test_one_member_more_than_a_launch_takes(mock):
    img = b"".join(LS.member(b"" if i % 2 else bytes([i & 0xFF])) for i in range(4097))
    res = same_as_reference(img)
    assert len(res.data) == 2049


def test_more_header_shapes_than_one_scan_keeps(mock):
    """66 000 members in one window: the scan's table of 65 536 candidates is filled and the rest is scanned in a second
    part; the launch table of 4096 is filled sixteen times"""
    one, none = LS.member(b"x"), LS.member(b"")
    img = b"".join(none if i % 3 else one for i in range(66000))
    res = same_as_reference(img)
    assert len(res.data) == 22000


def test_a_member_larger_than_the_window_limit_is_refused_by_name(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    res = la_api.cat(LS.member(LS.noise(70, 1200000), preset=0) + LS.member(b"x"))
    assert res.rc == la_api.ARCHIVE_FATAL and "lzip member too large for the GPU data plane" in res.error
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "2048")
    monkeypatch.setenv("LA_GPU_OUT_BUDGET_MIB", "2")
    p = bytes(3 << 20)
    for img in (LS.member(p, preset=0), LS.member(p, preset=0, version=0)):
        res = la_api.cat(img)
        assert res.rc == la_api.ARCHIVE_FATAL and "lzip member too large for the GPU data plane" in res.error, res.error


def test_budget_grows_for_a_member_decoded_alone(mock):
    p = bytes(40 << 20)         # 40 MiB of zeros are 6 KB of LZMA: the first budget (1 MiB) is doubled until it holds them
    res = la_api.cat(LS.member(p, preset=0, version=0))
    assert la_api.as_reference_tuple(res) == (p, 0, "")


def test_bid_policy(mock, monkeypatch):
    """auto: taken when the look-ahead shows a confirmed second member or the whole stream; a first member longer than
    the look-ahead is declined.  all: everything with the header shape."""
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "4")
    t = LS.noise(80, 9000)
    two = LS.member(t[:3000]) + LS.member(t[3000:])
    long_first, one_long, small = LS.member(t[:6000]) + LS.member(t[6000:]), LS.member(t), LS.member(t[:1000])
    fake = LS.member(t[:1000], member_size=7) + b"LZIP\x01\x14" + t[:5000]           # a header shape that no member size confirms
    v0 = LS.member(t[:1000], version=0) + LS.member(t[1000:], version=0)
    assert len(LS.member(t[:3000])) < 4096 < len(two) and len(LS.member(t[:6000])) > 4096 > len(small)
    monkeypatch.setenv("LA_GPU_BID", "auto")
    for img, plain in ((two, t), (small, t[:1000])):
        res = la_api.cat(img)
        assert res.filters[0] == LZIP and res.data == plain
    for img in (long_first, one_long, fake, v0):
        declined = la_api.cat(img)
        assert LZIP not in declined.filters and declined.data == img
    monkeypatch.setenv("LA_GPU_BID", "all")
    for img in (two, long_first, one_long, small, v0):
        res = la_api.cat(img)
        assert res.filters[0] == LZIP and res.rc == la_api.ARCHIVE_EOF
