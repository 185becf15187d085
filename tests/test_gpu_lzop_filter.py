"""The lzop read filter on the device (la_filter_lzop.c over la_lzo.hip) against the reference's read loop over the
Python decoder (lzop_support.reference_cat): verdict, message and delivered bytes are the reference's for valid,
multi-part, junk and damaged streams; the fixtures go through la_cat and la_tarwalk as well."""
import os
import subprocess

import pytest

import la_api
import lzop_support as L

pytestmark = pytest.mark.gpu

LZOP = (L.ARCHIVE_FILTER_LZOP, "lzop")
HOST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "libarchive_amd", "host")
GROUPS = 4


def same_as_reference(image, read_size=None):
    ref = L.reference_cat(image, read_size)
    res = la_api.cat(image, read_size=read_size)
    got = la_api.as_reference_tuple(res)
    assert (len(got[0]), got[1], got[2]) == (len(ref[0]), ref[1], ref[2])
    assert got[0] == ref[0]
    if res.filters:     # (an error in the first block ends archive_read_open, before the filters can be listed)
        assert res.filters[0] == LZOP
    return res


@pytest.mark.parametrize("group", range(GROUPS))
def test_shapes(gpu_ctx, group):
    """every shape of the host tests: header variants and refusals, parts, junk, stored blocks, the stale checksum, damaged
    and hand-built blocks"""
    for name in sorted(L.filter_shapes())[group::GROUPS]:
        same_as_reference(L.filter_shapes()[name])


@pytest.mark.parametrize("read_size", [None, 1000])
def test_fixtures(gpu_ctx, read_size):
    for m, img in L.fixtures():
        res = same_as_reference(img, read_size)
        assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZOP, m["file"]
        assert len(res.data) == m["decoded_size"]


def test_tar_listing(gpu_ctx):
    for m, img in L.fixtures():
        if m["entries"]:
            res = la_api.list_entries(img)
            assert res.rc == la_api.ARCHIVE_EOF and res.filters[0] == LZOP, res.error
            assert [e[0] for e in res.entries] == m["entries"]


def test_la_cat_and_la_tarwalk(gpu_ctx):
    """the two programs over the fixture files: the oracle's bytes, and the entry names the reference's tests walk"""
    env = dict(os.environ, LA_GPU_BID="auto")
    for m, img in L.fixtures():
        path = os.path.join(L.FIXTURE_DIR, m["file"])
        if not m["entries"]:
            run = subprocess.run([os.path.join(HOST, "la_cat"), path], capture_output=True, env=env, timeout=120)
            assert run.returncode == 0 and run.stdout == L.reference_read(img)[0], (m["file"], run.stderr[-500:])
            continue
        run = subprocess.run([os.path.join(HOST, "la_tarwalk"), "-v", path], capture_output=True, text=True, env=env, timeout=120)
        assert run.returncode == 0, run.stderr[-500:]
        lines = run.stdout.splitlines()
        assert [ln.split("\t")[0] for ln in lines[:-1]] == m["entries"], run.stdout
        assert lines[-1].endswith("filter lzop")


def test_cuts_and_flips(gpu_ctx):
    img = L.part(L.text(1, 3000), block_size=1200, flags=L.AU | L.AC, name=b"a name") + L.part(L.noise(2, 300, 16), flags=L.CC | L.EXTRA_FIELD, version=0x0930)
    for cut in range(9, len(img), 23):
        same_as_reference(img[:cut])
    bare = L.header(flags=0) + L.block(L.text(1, 1500), 0) + L.block(L.text(3, 1000), 0) + bytes(4)
    for bit in L.flip_cases(bare, 40)[::9]:
        same_as_reference(L.flip(bare, bit))


def test_3_mib_of_4_kib_blocks_under_small_windows(gpu_ctx, monkeypatch):
    """windows of 1 MiB over a 3 MiB stream in blocks of 4 KiB: 768 blocks, some stored, a block across every window edge;
    then the same with a damaged block in the third window"""
    monkeypatch.setenv("LA_GPU_BATCH_MIB", "1")
    monkeypatch.setenv("LA_GPU_BID", "all")
    unit = L.text(7, 40960) + L.randbytes(8, 8192)
    plain = unit * 64
    assert len(plain) == 3 << 20
    blocks = [L.block(unit[i:i + 4096], L.AU | L.AC) for i in range(0, len(unit), 4096)]
    img = L.header(flags=L.AU | L.AC) + b"".join(blocks) * 64 + bytes(4)
    assert len(img) > 1 << 20
    res = same_as_reference(img)
    assert res.data == plain
    same_as_reference(L.flip(img, (len(img) - 5000) * 8))
