"""The xz read filter on the device with LA_XZ_CHAINS=1 (la_filter_xz.c over la_xz.hip and la_xz_filters.hip) against the
reference's read loop over liblzma (xz_support.reference_cat): blocks whose chains hold delta and BCJ filters give
liblzma's bytes, verdicts and messages; la_cat reads a file the xz tool wrote with --x86 --lzma2."""
import lzma
import os
import shutil
import subprocess

import pytest

import la_api
import xz_chains_support as XC
import xz_support as XS

pytestmark = pytest.mark.gpu

ARCHIVE_FILTER_XZ = 6
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")


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


@pytest.mark.parametrize("name", sorted(XC.good_streams()))
def test_good_streams(gpu_ctx, chains_on, name):
    res = same_as_reference(XC.good_streams()[name], 1000 if name == "sixteen_mixed" else None)
    assert res.rc == la_api.ARCHIVE_EOF and len(res.data) > 0


@pytest.mark.parametrize("name", sorted(XC.bad_streams()))
def test_bad_streams(gpu_ctx, chains_on, name):
    res = same_as_reference(XC.bad_streams()[name])
    assert res.rc == la_api.ARCHIVE_FATAL
    if name.startswith("lzma_error"):
        assert len(res.data) == 65536


def test_an_error_next_to_a_64k_boundary_leaves_a_prefix_of_the_plain_data(gpu_ctx, chains_on):
    """x86, T from 65533 to 65553: the reference's code and message, plain bytes, at most one 64 KiB block fewer"""
    for name, (img, plain) in XC.near_boundary_streams().items():
        if name.startswith("04_"):
            ref = XS.reference_cat(img)
            got = la_api.as_reference_tuple(la_api.cat(img))
            assert got[1:] == ref[1:] and got[0] == plain[:len(got[0])], name
            assert len(got[0]) in (len(ref[0]), len(ref[0]) - 65536), (name, len(got[0]), len(ref[0]))


def test_small_windows(gpu_ctx, chains_on, monkeypatch):
    """windows of 1 MiB over 3.6 MB of blocks with chains: a block straddles every window boundary"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    img = XC.window_stream()
    same_as_reference(img)
    same_as_reference(img[:len(img) - 100000])


def test_without_the_variable_the_chain_is_refused(gpu_ctx, monkeypatch):
    monkeypatch.delenv("LA_XZ_CHAINS", raising=False)
    res = la_api.cat(XC.good_streams()["alone_04"])
    assert res.rc == la_api.ARCHIVE_FATAL
    assert res.error == "xz GPU data plane: unsupported filter x86 BCJ in a block's filter chain (only LZMA2 is decoded)"


def test_la_cat_on_a_file_from_the_xz_tool(gpu_ctx, tmp_path):
    plain = XC.real_code(150000)
    path = str(tmp_path / "code.xz")
    if shutil.which("xz"):
        image = subprocess.run(["xz", "-c", "--x86", "--lzma2=preset=1", "--block-size=65536"], input=plain, capture_output=True, check=True).stdout
    else:       # (the same encoder through Python's binding)
        image = lzma.compress(plain, format=lzma.FORMAT_XZ, filters=[{"id": lzma.FILTER_X86}, {"id": lzma.FILTER_LZMA2, "preset": 1}])
    with open(path, "wb") as f:
        f.write(image)
    env = dict(os.environ, LA_GPU_BID="auto", LA_XZ_CHAINS="1")
    run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
    assert run.returncode == 0 and run.stdout == plain, run.stderr[-500:]
    env.pop("LA_XZ_CHAINS")
    run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
    assert run.returncode != 0 and b"unsupported filter x86 BCJ" in run.stderr
