"""The xz read filter's HOST side (la_filter_xz.c: the container walk, windows, the carry of the unfinished unit, blocks
with and without sizes, the bytes held back in front of an error, verdicts and strings) over a CPU stand-in for
la_gpu_xz_decode (tests/mock_gpu/la_gpu_xz_chains_mock.c: the kernel's own rules header, compiled for the host).  la_api.cat through the mock
library must equal the reference's read loop over liblzma (xz_support.reference_read) on bytes, return code, error
string and filter code / name.  The same shapes go through a stand-alone ASan/UBSan program of the same sources."""
import lzma
import os
import subprocess

import pytest

import la_api
import mock_build
import xz_build as XB
import xz_support as XS

ARCHIVE_FILTER_XZ = 6


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def same_as_reference(image, read_size=None):
    ref = XS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz")
    return res


# T is a multiple of 64 KiB there and the error sits in the next header: with 1-byte reads the reference sees the error
# in a call of its own (la_filter_xz.c's head comment names the assumption)
WHOLE_READS_ONLY = {"error_behind_64k_boundary"}


@pytest.mark.parametrize("name", sorted(XS.filter_shapes()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_shapes(mock, name, read_size):
    if read_size == 1 and name in WHOLE_READS_ONLY:
        read_size = 65536
    same_as_reference(XS.filter_shapes()[name], read_size)


@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_fixtures(mock, read_size):
    for m, img in XS.fixtures():
        res = same_as_reference(img, read_size)
        assert len(res.data) == m["decoded_size"] and res.filters[0] == (ARCHIVE_FILTER_XZ, "xz"), m["file"]


def test_hand_built_data(mock):
    for name, (raw, plain) in list(XS.packet_cases().items()) + list(XS.chunk_plans().items()):
        assert same_as_reference(XS.wrap(raw, plain, XB.CHECK_CRC64)).data == plain, name
    for name, (raw, valid, ok, dict_byte) in XS.beyond_cases().items():
        res = same_as_reference(XS.wrap(raw, valid if ok else b"", dict_byte=dict_byte))
        assert (res.rc == la_api.ARCHIVE_EOF) == ok, name
    for name, (raw, _) in XS.refusals().items():
        res = same_as_reference(XS.wrap(raw))
        assert res.error == XS.DATA_ERROR, name


def test_unsupported_filters_are_named(mock):
    t = XS.text(5, 300)
    for fid, props, word in ((0x03, b"\x00", "delta"), (0x04, b"", "x86 BCJ"), (0x07, b"", "ARM BCJ"), (0x0A, b"", "ARM64 BCJ"), (0x0B, b"", "RISC-V BCJ")):
        img = XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, extra_filters=[(fid, props)])], XB.CHECK_CRC32)
        assert XS.reference_read(img)[1] == 0 or fid in (0x03, 0x0A, 0x0B)     # (liblzma runs the chain; delta changes the bytes, a liblzma from before 5.4 does not know the last two)
        res = la_api.cat(img)
        assert res.rc == la_api.ARCHIVE_FATAL and "unsupported filter " + word in res.error, res.error


def test_small_windows(mock, monkeypatch):
    """windows of 1 MiB over 3.6 MiB of noise in blocks of 300 000 bytes: every window boundary cuts a block, sized
    blocks are carried whole, size-less ones are tried, found short and carried"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    parts = [XS.noise(60 + i, 300000) for i in range(12)]
    for sizes in (True, False):
        img = XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC32, comp=sizes, uncomp=sizes) for p in parts], XB.CHECK_CRC32)
        assert len(img) > 3 << 20
        same_as_reference(img)
        same_as_reference(img[:len(img) - 100000])
        same_as_reference(XS.flip(img, (2 << 20) * 8 + 5))


@pytest.mark.parametrize("read_size", [None, 1000])
def test_tail_over_several_windows(mock, monkeypatch, read_size):
    """windows of 1 MiB that decode 20 000 bytes each: the held-back tail takes the bytes of three windows before the
    fourth crosses 64 KiB, and an error in the fourth drops all of them"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    for name, img in XS.padded_streams().items():
        data, _, msg = la_api.as_reference_tuple(same_as_reference(img, read_size))
        assert (len(data), msg) == XS.PADDED_STREAMS_RESULT[name], name


def test_a_block_larger_than_the_window_limit_is_refused_by_name(mock, monkeypatch):
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_MAX_BATCH_MIB", "1")
    p = XS.noise(70, 1200000)
    for sizes in (True, False):
        res = la_api.cat(XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC32, comp=sizes, uncomp=sizes)], XB.CHECK_CRC32))
        assert res.rc == la_api.ARCHIVE_FATAL and "xz block too large for the GPU data plane" in res.error


def test_budget_grows_for_a_block_without_sizes(mock):
    p = bytes(40 << 20)         # 40 MiB of zeros are 6 KB of LZMA2: the first budget (1 MiB) is doubled until it holds them
    img = XB.stream([XB.block(XB.lzma2(p, preset=0), p, XB.CHECK_CRC32, comp=False, uncomp=False)], XB.CHECK_CRC32)
    res = la_api.cat(img)
    assert la_api.as_reference_tuple(res) == (p, 0, "")


def test_cut_at_every_byte(mock):
    img = XS.stream3000()
    for cut in range(6, len(img)):
        same_as_reference(img[:cut])
    bare = XS.filter_shapes()["mixed_sized_and_bare"]
    for cut in range(6, len(bare), 3):
        same_as_reference(bare[:cut])


def test_single_bit_flips(mock):
    img = XS.stream3000()
    for bit in XS.flip_cases():
        same_as_reference(XS.flip(img, bit))


def test_bid_policy(mock, monkeypatch):
    """auto: a stream whose first block carries its compressed size is taken whatever its length; one that opens with a
    size-less block is taken only when the look-ahead holds all of it.  all: everything with the magic."""
    monkeypatch.setenv("LA_GPU_BID_LOOKAHEAD_KIB", "4")
    t = XS.noise(80, 9000)
    threaded = XB.stream([XB.block(XB.lzma2(t[:4500]), t[:4500], XB.CHECK_CRC64), XB.block(XB.lzma2(t[4500:]), t[4500:], XB.CHECK_CRC64)], XB.CHECK_CRC64)
    plain_xz, small = lzma.compress(t), lzma.compress(t[:1000])
    assert len(threaded) > 4096 and len(plain_xz) > 4096 > len(small)
    monkeypatch.setenv("LA_GPU_BID", "auto")
    assert la_api.cat(threaded).filters[0] == (ARCHIVE_FILTER_XZ, "xz") and la_api.cat(threaded).data == t
    assert la_api.cat(small).filters[0] == (ARCHIVE_FILTER_XZ, "xz")
    declined = la_api.cat(plain_xz)
    assert (ARCHIVE_FILTER_XZ, "xz") not in declined.filters and declined.data == plain_xz
    assert la_api.cat(lzma.compress(b"")).filters[0] == (ARCHIVE_FILTER_XZ, "xz")
    monkeypatch.setenv("LA_GPU_BID", "all")
    for img in (threaded, plain_xz, small):
        res = la_api.cat(img)
        assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz") and res.rc == la_api.ARCHIVE_EOF


def test_tar_walk_over_the_fixture(mock):
    m, img = XS.fixtures()[0]
    res = la_api.list_entries(img)
    assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == (ARCHIVE_FILTER_XZ, "xz"), res.error
    assert [e[0] for e in res.entries] == m["entries"]


def test_sanitizer_program(mock, tmp_path):
    """the C filter and the mock as one ASan/UBSan program of their own, over the shapes, the hand-built data, cuts and flips"""
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    images = list(XS.filter_shapes().values()) + [img for _, img in XS.fixtures()]
    images += [XS.wrap(raw, plain, XB.CHECK_CRC64) for raw, plain in list(XS.packet_cases().values()) + list(XS.chunk_plans().values())]
    images += [XS.wrap(raw) for raw, _ in XS.refusals().values()] + [XS.wrap(c[0], dict_byte=c[3]) for c in XS.beyond_cases().values()]
    img = XS.stream3000()
    images += [img[:cut] for cut in range(6, len(img), 5)] + [XS.flip(img, b) for b in XS.flip_cases()[::4]]
    env = dict(os.environ, LA_GPU_BID="all", ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)

    def run_over(images, tag, env):
        paths = []
        for i, im in enumerate(images):
            paths.append(os.path.join(out, "%s%04d.xz" % (tag, i)))
            with open(paths[-1], "wb") as f:
                f.write(im)
        for k in range(0, len(paths), 400):
            run = subprocess.run([exe] + paths[k:k + 400], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
            assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
            lines = run.stdout.splitlines()
            assert len(lines) == len(paths[k:k + 400])
            for line, im in zip(lines, images[k:k + 400]):
                data, rc, msg = XS.reference_cat(im)
                assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(im))
        return lines

    run_over(images, "case", env)
    # the tail that takes several windows' bytes (test_tail_over_several_windows), in a run of its own with windows of 1 MiB
    held = XS.padded_streams()
    lines = run_over(list(held.values()), "held", dict(env, LA_GPU_BATCH_MIB="1"))
    for name, line in zip(held, lines):
        assert (int(line.split()[1]), line.split(" ", 3)[3]) == XS.PADDED_STREAMS_RESULT[name], (name, line)
