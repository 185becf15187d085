"""CPU-only: the host side of LA_ZSTD_BLOCKS=1 (one Zstandard frame decoded block-parallel on the device): the bid
policy takes a frame longer than the look-ahead, the filter sets LA_ZSTD_OPT_BLOCK_PARALLEL on windows of large
frames -- tests/mock_gpu ignores the bit and decodes whole frames, so the stream still comes out right -- and the
header's new names lie where ctypes and numpy put them."""
import ctypes as C
import os
import random
import subprocess

import pytest

import la_api
import mock_build
from test_gpu_bid_policy import ARCHIVE_FILTER_ZSTD, _codes, _zstd_raw_frame

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def mock():
    lib = mock_build.host_lib()
    la_api.use_library(lib)
    yield lib
    la_api.use_library(None)


@pytest.fixture(scope="module")
def lone():
    plain = random.Random(11).randbytes(1_500_000)
    return _zstd_raw_frame(plain), plain


def test_the_bidder_takes_a_long_frame_only_with_the_variable(mock, lone, monkeypatch):
    img, _ = lone
    la = 1 << 20
    mock.la_bid_zstd_parallel.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
    monkeypatch.delenv("LA_GPU_BID", raising=False)
    monkeypatch.delenv("LA_ZSTD_BLOCKS", raising=False)
    assert mock.la_bid_zstd_parallel(img[:la], la, la) == 0
    assert mock.la_bid_zstd_parallel(img[:1000], 1000, la) == 1          # a stream shorter than the look-ahead
    monkeypatch.setenv("LA_ZSTD_BLOCKS", "0")
    assert mock.la_bid_zstd_parallel(img[:la], la, la) == 0
    monkeypatch.setenv("LA_ZSTD_BLOCKS", "1")
    assert mock.la_bid_zstd_parallel(img[:la], la, la) == 1


def test_a_lone_frame_through_the_filter_on_the_mock(mock, lone, monkeypatch):
    img, plain = lone
    monkeypatch.delenv("LA_GPU_BID", raising=False)
    monkeypatch.delenv("LA_ZSTD_BLOCKS", raising=False)
    r = la_api.cat(img)
    assert ARCHIVE_FILTER_ZSTD not in _codes(r) and r.data == img
    monkeypatch.setenv("LA_ZSTD_BLOCKS", "1")
    r = la_api.cat(img)
    assert ARCHIVE_FILTER_ZSTD in _codes(r)
    assert la_api.as_reference_tuple(r) == (plain, 0, "")


def test_header_names_match_ctypes_and_numpy(tmp_path):
    from libarchive_amd import _native as N
    from libarchive_amd import zstd
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "la_gpu.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %u\\n", sizeof(la_zstd_result), offsetof(la_zstd_result, path),\n'
                   '    offsetof(la_zstd_result, reserved), offsetof(la_zstd_result, out_len), LA_ZSTD_OPT_BLOCK_PARALLEL); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_path, off_res, off_len, opt = map(int, subprocess.check_output([str(exe)]).split())
    dt = zstd.ZSTD_RESULT_DTYPE
    assert (size, off_path, off_res, off_len) == (dt.itemsize, dt.fields["path"][1], dt.fields["reserved"][1], dt.fields["out_len"][1])
    assert (size, off_path, off_res, off_len) == (16, 4, 4, 8)
    assert opt == N.LA_ZSTD_OPT_BLOCK_PARALLEL == zstd.LA_ZSTD_OPT_BLOCK_PARALLEL == 4
    assert C.sizeof(zstd._ZstdBatchC) == 56 and zstd._ZstdBatchC.options.offset == 28     # the batch struct did not change
