"""The ZIP write format on the device data plane, through the archive_write_* slice (host/la_write_zip.c):
archive_write_new -> set_format_zip -> options -> open_memory -> header / data / finish_entry ... -> close, with
windows of 1 MiB so that entries split across la_gpu_zip_compress calls.  What it writes must read with Python's
zipfile and with this repository's own ZIP reader, and every field of every record must be what the cited lines of
libarchive/archive_write_set_format_zip.c prescribe (tests/zip_write_support.py).  The same shapes run against a CPU
stand-in for the device call in tests/test_host_zip_write.py."""
import gzip
import random
import zlib

import pytest

import la_api
import libarchive_amd as la
import zip_write_support as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(gpu_ctx):
    mp = pytest.MonkeyPatch()
    mp.setenv("LA_GPU_WRITE_WINDOW_MIB", "1")
    la_api.use_library(None)
    yield Z.setup(la.host_lib())
    mp.undo()


@pytest.fixture(scope="module")
def main_archive(lib):
    rc, img = Z.write_zip(lib, Z.main_entries())
    assert rc == Z.ARCHIVE_OK, img
    return img


def test_main_archive_records(main_archive):
    locals_, central, end = Z.check_records(main_archive, Z.main_entries())
    # the device's streams: random bytes do not shrink and cost 5 bytes per 48 KiB chunk and window piece; text shrinks
    by_name = {c["name"]: c for c in central}
    assert 300000 < by_name[b"random.bin"]["comp"] <= 300000 + 5 * (300000 // 49152 + 2) + 2
    assert by_name[b"a/dir/text"]["comp"] < (3 << 20) // 2
    assert by_name[b"empty.txt"]["comp"] == 2


def test_main_archive_reads_with_zipfile(main_archive):
    Z.check_with_zipfile(main_archive, Z.main_entries())


def test_main_archive_reads_with_own_reader(lib, main_archive):
    res = la_api.list_entries(main_archive)
    assert res.rc == la_api.ARCHIVE_EOF and res.error is None and res.format_name.startswith("ZIP")
    assert [(n.encode(), body) for n, _, _, _, _, body in res.entries] == [(e.stored_name, e.kept) for e in Z.main_entries()]
    for e, (_, size, ftype, perm, mtime, _) in zip(Z.main_entries(), res.entries):
        assert (ftype, perm) == (e.type, e.perm)
        if e.mtime is not None:
            assert 0 <= e.mtime - mtime < 2  # the reader goes by the DOS time, which counts every two seconds


@pytest.mark.parametrize("options,kw", [
    ((("compression", "store"),), dict(method=0)),
    ((("compression-level", "0"),), dict(method=0)),
    ((("compression-level", "1"),), dict(level=1)),
    ((("compression-level", "9"),), dict(level=9)),
    ((("zip64", "1"),), dict(force_zip64=True)),
    ((("fakecrc32", "1"),), dict(fake_crc=True)),
], ids=["store", "level0", "level1", "level9", "zip64", "fakecrc32"])
def test_option_archives(lib, options, kw):
    entries = [e for e in Z.main_entries() if len(e.data) <= 300000] + [Z.Entry("two-windows", Z.word_text(12, Z.WINDOW + 4321), piece=100001)]
    rc, img = Z.write_zip(lib, entries, options)
    assert rc == Z.ARCHIVE_OK, img
    locals_, central, end = Z.check_records(img, entries, **kw)
    if kw.get("force_zip64"):
        assert all(c["need"] == 45 for e, c in zip(entries, central) if e.type == Z.AE_IFREG) and end["zip64"] is not None
    if not kw.get("fake_crc"):      # (zipfile would reject the zero CRCs)
        Z.check_with_zipfile(img, entries, kw.get("method", 8))


def test_level_one_is_fixed_codes_and_level_nine_is_not_larger(lib):
    entries = [Z.Entry("text", Z.word_text(13, 200000))]
    sizes = {}
    for level in ("1", "9"):
        rc, img = Z.write_zip(lib, entries, (("compression-level", level),))
        assert rc == Z.ARCHIVE_OK, img
        locals_, central, _ = Z.parse(img)
        sizes[level] = central[0]["comp"]
        assert (locals_[0]["data"][0] >> 1) & 3 == (1 if level == "1" else 2)   # BTYPE of the first block: fixed / dynamic codes
    assert sizes["9"] <= sizes["1"]


@pytest.mark.parametrize("key,value,rc,message", Z.OPTION_TABLE, ids=["%s=%s" % (k, v) for k, v, _, _ in Z.OPTION_TABLE])
def test_option_table(lib, key, value, rc, message):
    got, err = Z.set_option(lib, key, value)
    assert got == rc, err
    if message is not None:
        assert err == message


def test_many_entries_get_the_zip64_end_record(lib):
    rnd = random.Random(41)
    entries = [Z.Entry("f%05d" % i, rnd.randbytes(rnd.randint(0, 8)), mtime=1700000000 + i) for i in range(66000)]
    rc, img = Z.write_zip(lib, entries, finish_every=0)
    assert rc == Z.ARCHIVE_OK, img
    locals_, central, end = Z.parse(img)
    assert end["n"] == 0xFFFF and end["zip64"] is not None and end["zip64"]["n"] == 66000 and end["zip64"]["need"] == 45
    assert [c["name"] for c in central] == [e.name for e in entries]
    for i in [0, 65535, 65536, 65999] + rnd.sample(range(66000), 200):
        z = zlib.decompressobj(-15)
        assert z.decompress(locals_[i]["data"]) == entries[i].data and z.eof
        assert locals_[i]["desc"]["crc"] == zlib.crc32(entries[i].data) == central[i]["crc"]


def test_through_the_gzip_write_filter(lib):
    entries = [e for e in Z.main_entries() if len(e.data) <= 300000]
    rc, gz = Z.write_zip(lib, entries, gzip_filter=True)
    assert rc == Z.ARCHIVE_OK, gz
    img = gzip.decompress(gz)
    Z.check_records(img, entries)
    Z.check_with_zipfile(img, entries)
