"""The xz read filter's host side with LA_XZ_CHAINS=1 (la_filter_xz.c: chains parsed and judged as liblzma judges them,
the chain table carried to the device call) over a CPU stand-in for la_gpu_xz_decode that compiles both rules headers
of the kernels (tests/mock_gpu/la_gpu_xz_chains_mock.c).  la_api.cat through the mock library must equal the reference's read loop over
liblzma (xz_support.reference_cat) on bytes, return code and error string.  Without the variable the same streams end
in today's refusal.  The same shapes go through a stand-alone ASan/UBSan program of the same sources."""
import os
import subprocess

import pytest

import la_api
import mock_build
import xz_build as XB
import xz_chains_support as XC
import xz_support as XS

ARCHIVE_FILTER_XZ = 6


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


@pytest.fixture
def chains_on(monkeypatch):
    monkeypatch.setenv("LA_XZ_CHAINS", "1")


def same_as_reference(image, read_size=None):
    ref = XS.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:
        assert res.filters[0] == (ARCHIVE_FILTER_XZ, "xz")
    return res


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


@pytest.mark.parametrize("name", sorted(XC.good_streams()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_good_streams(mock, chains_on, name, read_size):
    res = same_as_reference(XC.good_streams()[name], read_size)
    assert res.rc == la_api.ARCHIVE_EOF and len(res.data) > 0


@pytest.mark.parametrize("name", sorted(XC.bad_streams()))
@pytest.mark.parametrize("read_size", [None, 1000, 1])
def test_bad_streams(mock, chains_on, name, read_size):
    res = same_as_reference(XC.bad_streams()[name], read_size)
    assert res.rc == la_api.ARCHIVE_FATAL
    if name.startswith("lzma_error"):
        assert len(res.data) == 65536       # T = 74 008: the first 64 KiB block is out, unfiltered


def test_an_error_next_to_a_64k_boundary_leaves_a_prefix_of_the_plain_data(mock, chains_on):
    """there the count of 64 KiB blocks may be one below the reference's (la_filter_xz.c's head comment), never above it,
    and what is handed out is plain data; code and message are the reference's"""
    fewer = 0
    for name, (img, plain) in XC.near_boundary_streams().items():
        ref = XS.reference_cat(img)
        got = la_api.as_reference_tuple(la_api.cat(img))
        assert got[1:] == ref[1:] and ref[1] == la_api.ARCHIVE_FATAL, name
        assert ref[0] == plain[:len(ref[0])] and got[0] == plain[:len(got[0])], name
        assert len(got[0]) in (len(ref[0]), len(ref[0]) - 65536), (name, len(got[0]), len(ref[0]))
        fewer += len(got[0]) < len(ref[0])
    assert fewer <= 3 * 16        # (T in [65536, 65536 + hold) only)


def test_small_windows(mock, chains_on, monkeypatch):
    """windows of 1 MiB over 3.6 MB of blocks with chains: every window boundary cuts a block"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    img = XC.window_stream()
    assert len(img) > 3 << 20
    same_as_reference(img)
    same_as_reference(img[:len(img) - 100000])
    same_as_reference(XS.flip(img, (2 << 20) * 8 + 5))


def test_newer_filters_stay_refused_by_name(mock, chains_on):
    t = XS.text(5, 300)
    for extra, word in (([(0x0A, b"")], "ARM64 BCJ"), ([(0x0B, b"")], "RISC-V BCJ"), ([(0x04, b""), (0x0A, b"")], "ARM64 BCJ")):
        img = XB.stream([XB.block(XB.lzma2(t), t, XB.CHECK_CRC32, extra_filters=extra)], XB.CHECK_CRC32)
        res = la_api.cat(img)
        assert res.rc == la_api.ARCHIVE_FATAL and "unsupported filter " + word in res.error, res.error


def test_without_the_variable_chains_are_refused_as_before(mock, monkeypatch):
    monkeypatch.delenv("LA_XZ_CHAINS", raising=False)
    names = {XC.DELTA: "delta", XC.X86: "x86 BCJ", XC.POWERPC: "PowerPC BCJ", XC.IA64: "IA-64 BCJ", XC.ARM: "ARM BCJ", XC.ARMTHUMB: "ARM-Thumb BCJ",
             XC.SPARC: "SPARC BCJ"}
    for fid, _ in XC.ALONE:
        res = la_api.cat(XC.good_streams()["alone_%02x" % fid])
        assert res.rc == la_api.ARCHIVE_FATAL and res.data == b""
        assert res.error == "xz GPU data plane: unsupported filter %s in a block's filter chain (only LZMA2 is decoded)" % names[fid]
    for name in ("delta4_x86", "sixteen_mixed", "without_sizes"):
        res = la_api.cat(XC.good_streams()[name])
        assert res.rc == la_api.ARCHIVE_FATAL and "unsupported filter" in res.error
    for value in ("0", "", "yes"):      # only 1 switches it on
        monkeypatch.setenv("LA_XZ_CHAINS", value)
        assert "unsupported filter x86 BCJ" in la_api.cat(XC.good_streams()["alone_04"]).error


def test_sanitizer_program(mock, tmp_path):
    """the C filter and the stand-in as one ASan/UBSan program of their own over the same streams"""
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    images = list(XC.good_streams().values()) + list(XC.bad_streams().values())
    img = XC.good_streams()["sized_and_bare"]
    images += [img[:cut] for cut in range(6, len(img), 211)]
    env = dict(os.environ, LA_GPU_BID="all", LA_XZ_CHAINS="1", ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    paths = []
    for i, im in enumerate(images):
        paths.append(os.path.join(out, "case%04d.xz" % i))
        with open(paths[-1], "wb") as f:
            f.write(im)
    run = subprocess.run([exe] + paths, capture_output=True, text=True, env=env, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(paths)
    for line, im in zip(lines, images):
        data, rc, msg = XS.reference_cat(im)
        assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(im))
