"""The failure paths of the bzip2, xz, lzip and lzop read filters: what they do when a device call fails.  The CPU mock of
the device ABI (tests/mock_gpu/la_gpu_mock.c) fails the k-th call of one kind when LA_MOCK_FAIL=<call>:<k> is set; for
every filter and every kind of call, k runs from 1 until a read completes with no call failed.  A failed read has to end
with ARCHIVE_FATAL and the data plane's own words for that call, hand out nothing but a prefix of the plain data, and
leave the process able to read the same stream in full.  The same cases run in the stand-alone ASan / UBSan program of
the readers (tests/mock_gpu/la_read_main.c), where a leak or a double free in the cleanup would show: the sanitizer runtimes
are linked into that program statically, and nothing is loaded into Python."""
import bz2
import ctypes as C
import os
import re
import subprocess

import pytest

import bzip2_support as BS
import la_api
import mock_build
import lzip_support as LS
import lzop_support as L
import xz_build as XB
import xz_support as XS

CALLS = ("la_gpu_open", "la_gpu_malloc", "la_gpu_malloc_host", "la_gpu_memcpy_h2d", "la_gpu_memcpy_d2h")
# the label la_window_fail is given for each call; a pinned allocation is the stage's (the gather) or the output's
LABELS = {"la_gpu_malloc": ("la_gpu_malloc",), "la_gpu_malloc_host": ("la_gpu_malloc_host", "pinned staging allocation"),
          "la_gpu_memcpy_h2d": ("la_gpu_memcpy_h2d",), "la_gpu_memcpy_d2h": ("la_gpu_memcpy_d2h",)}
K_CAP = 10000


def bzip2_stream():
    """three streams of 0.5 MB each: two windows of 1 MiB"""
    return b"".join(bz2.compress(BS.noise(40 + i, 500000), 1) for i in range(3))


def xz_stream():
    """five blocks of 0.3 MB, both sizes in their headers: two windows of 1 MiB"""
    parts = [XS.noise(60 + i, 300000) for i in range(5)]
    return XB.stream([XB.block(XB.lzma2(p), p, XB.CHECK_CRC32) for p in parts], XB.CHECK_CRC32)


def lzip_stream():
    """five members of 0.3 MB, the last of version 0 (decoded alone): two windows of 1 MiB"""
    return b"".join(LS.member(LS.noise(62 + i, 300000), preset=0, version=i != 4) for i in range(5))


def lzop_stream():
    """9000 blocks of one byte: three launches in one window"""
    return L.part(L.text(9, 9000), block_size=1)


# filter name -> stream
FILTERS = {"bzip2": bzip2_stream, "xz": xz_stream, "lzip": lzip_stream, "lzop": lzop_stream}


@pytest.fixture(scope="module", params=sorted(FILTERS))
def reader(request, tmp_path_factory):
    """(filter name, mock library, directory for files, stream, its plain bytes) with la_api routed to the mock library"""
    name = request.param
    stream = FILTERS[name]
    out = str(tmp_path_factory.mktemp("fail_" + name))
    lib = mock_build.host_lib()
    lib.la_gpu_mock_failed.restype = C.c_ulong
    la_api.use_library(lib)
    env = {"LA_GPU_BATCH_MIB": "1", "LA_GPU_BID": "all"}
    old = {k: os.environ.get(k) for k in list(env) + ["LA_MOCK_FAIL"]}
    os.environ.update(env)
    os.environ.pop("LA_MOCK_FAIL", None)
    image = stream()
    whole = la_api.cat(image)
    assert whole.rc == la_api.ARCHIVE_EOF and whole.filters[0][1] == name and len(whole.data) > 0, whole.error
    yield name, lib, out, image, whole.data
    la_api.use_library(None)
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.mark.parametrize("call", CALLS)
def test_every_failing_call(reader, call, monkeypatch):
    name, lib, _, image, plain = reader
    failed_runs = 0
    for k in range(1, K_CAP + 1):
        monkeypatch.setenv("LA_MOCK_FAIL", "%s:%d" % (call, k))
        before = lib.la_gpu_mock_failed()
        res = la_api.cat(image)
        failed = lib.la_gpu_mock_failed() - before
        if not failed:
            assert res.rc == la_api.ARCHIVE_EOF and res.data == plain, (k, res.error)
            break
        assert failed == 1
        failed_runs += 1
        assert res.rc == la_api.ARCHIVE_FATAL, (k, res.rc, res.error)
        if call == "la_gpu_open":
            assert res.error.startswith("Can't initialize %s GPU data plane (la_gpu_open: " % name), (k, res.error)
        else:
            assert res.error in ["%s GPU data plane: %s failed: mock failure" % (name, what) for what in LABELS[call]], (k, res.error)
        assert plain.startswith(res.data), k
        # the same process reads the stream in full once nothing fails
        monkeypatch.delenv("LA_MOCK_FAIL")
        again = la_api.cat(image)
        assert again.rc == la_api.ARCHIVE_EOF and again.data == plain, (k, again.error)
    else:
        raise AssertionError("%s still fails at call %d: the hook never lets a read complete" % (call, K_CAP))
    # every filter opens the device, allocates device and pinned memory and copies both ways
    assert failed_runs >= 1, "no %s was failed" % call
    if call == "la_gpu_open":
        assert failed_runs == 1


def test_failing_calls_under_asan_ubsan(reader):
    """each call's first three failures in the filter's sanitizer program: exit status 0 (the three read sizes agree),
    nothing reported, no leak"""
    name, _, out, image, plain = reader
    prog = mock_build.program("la_read_asan")
    path = os.path.join(out, "stream." + name)
    with open(path, "wb") as f:
        f.write(image)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LA_MOCK_FAIL", None)
    run = subprocess.run([prog, path], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and re.match(r"0 %d [0-9a-f]{16} $" % len(plain), run.stdout), run.stdout + run.stderr[-3000:]
    for call in CALLS:
        for k in (1, 2, 3):
            run = subprocess.run([prog, path], env=dict(env, LA_MOCK_FAIL="%s:%d" % (call, k)),
                                 capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, (call, k, (run.stdout + run.stderr)[-3000:])
            assert "AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, (call, k, run.stderr[-3000:])
            if k == 1:      # (a later one may never be made: the device is opened once per read)
                assert run.stdout.startswith("%d " % la_api.ARCHIVE_FATAL) and "GPU data plane" in run.stdout, (call, k, run.stdout)
