"""CPU-only: the ZIP write format (host/la_write_zip.c) and the format hooks of the write core, against a CPU stand-in
for la_gpu_zip_compress (tests/mock_gpu/la_gpu_zip_mock.c: zlib, one Z_SYNC_FLUSH per chunk, then 03 00).  Everything the host decides
-- segments and gaps per window, headers and descriptors patched into the gaps, entries chained over windows, the
central directory and the end records, the options, the failure paths -- is what is checked here, field by field
against the lines of libarchive/archive_write_set_format_zip.c that la_write_zip.c restates.  The device's side of the
same call is tests/test_gpu_zip_compress.py, the two together tests/test_gpu_zip_write.py."""
import ctypes as C
import gzip
import os
import random

import pytest

import la_api
import mock_build
import zip_write_support as Z


@pytest.fixture(scope="module")
def lib():
    mock = mock_build.host_lib()
    mock._gpu_mock = mock_build.gpu_lib()
    saved = os.environ.get("LA_GPU_WRITE_WINDOW_MIB")
    os.environ["LA_GPU_WRITE_WINDOW_MIB"] = "1"     # entries split across windows
    la_api.use_library(mock)
    yield Z.setup(mock)
    la_api.use_library(None)
    if saved is None:
        del os.environ["LA_GPU_WRITE_WINDOW_MIB"]
    else:
        os.environ["LA_GPU_WRITE_WINDOW_MIB"] = saved


@pytest.fixture(scope="module")
def main_archive(lib):
    rc, img = Z.write_zip(lib, Z.main_entries())
    assert rc == Z.ARCHIVE_OK, img
    return img


def test_main_archive_records(main_archive):
    Z.check_records(main_archive, Z.main_entries())


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
    ((("compression-level", "3"), ("threads", "8")), dict(level=3)),
    ((("zip64", "1"),), dict(force_zip64=True)),
    ((("fakecrc32", "1"),), dict(fake_crc=True)),
    # level 0 asks for "store" (:412-414); a method named after it stands: method 8 of stored blocks, zlib's level 0
    ((("compression-level", "0"), ("compression", "deflate")), dict(level=0)),
], ids=["store", "level0", "level1", "level9", "level3_threads", "zip64", "fakecrc32", "deflate_level0"])
def test_option_archives(lib, options, kw):
    entries = [e for e in Z.main_entries() if len(e.data) <= 300000]
    rc, img = Z.write_zip(lib, entries, options)
    assert rc == Z.ARCHIVE_OK, img
    locals_, central, end = Z.check_records(img, entries, **kw)
    if kw.get("force_zip64"):
        assert all(c["need"] == 45 for e, c in zip(entries, central) if e.type == Z.AE_IFREG) and end["zip64"] is not None
    if not kw.get("fake_crc"):      # (zipfile would reject the zero CRCs)
        Z.check_with_zipfile(img, entries, kw.get("method", 8))


@pytest.mark.parametrize("key,value,rc,message", Z.OPTION_TABLE, ids=["%s=%s" % (k, v) for k, v, _, _ in Z.OPTION_TABLE])
def test_option_table(lib, key, value, rc, message):
    got, err = Z.set_option(lib, key, value)
    assert got == rc, err
    if message is not None:
        assert err == message
    # without a module name the format is still asked
    got, _ = Z.set_option(lib, key, value, module=None)
    assert got == rc


def test_option_module_names(lib):
    assert Z.set_option(lib, "compression", "store", module=b"tar") == (Z.ARCHIVE_FAILED, "Unknown module name: `tar'")
    assert Z.set_option(lib, "", "x") == (Z.ARCHIVE_FAILED, "Empty option")
    assert Z.set_option(lib, "", None)[0] == Z.ARCHIVE_OK
    # the raw format has no options
    a = lib.archive_write_new()
    assert lib.archive_write_set_format_raw(a) == Z.ARCHIVE_OK
    assert lib.archive_write_set_format_option(a, b"raw", b"compression", b"store") == Z.ARCHIVE_FAILED
    assert lib.archive_error_string(a) == b"Undefined option: `raw:compression=store'"
    lib.archive_write_free(a)


def test_names_that_are_not_ascii(lib):
    entries = [Z.Entry("grüße.txt".encode("utf-8"), b"hallo"), Z.Entry("plain.txt", b"x")]
    rc, img = Z.write_zip(lib, entries, (("hdrcharset", "UTF-8"),))
    assert rc == Z.ARCHIVE_OK, img
    Z.check_records(img, entries, utf8=True)
    Z.check_with_zipfile(img, entries)


def test_unsupported_types_fail_and_write_nothing(lib):
    good = Z.Entry("before", b"data")
    for bad, what in ((Z.AE_IFLNK, "symbolic links"), (Z.AE_IFIFO, "named pipes"), (0o020000, "character devices")):
        rc, err = Z.write_zip(lib, [good, Z.Entry("odd", type=bad)])
        assert rc == Z.ARCHIVE_FAILED and err == "odd: zip format cannot archive " + what
    rc, err = Z.write_zip(lib, [Z.Entry("odd", type=0, perm=0o644)])
    assert rc == Z.ARCHIVE_FAILED and err == "odd: zip format cannot archive files with mode 0644"
    # the archive goes on without the refused entry
    lib_ = Z.setup(lib)
    a, ent = lib_.archive_write_new(), lib_.archive_entry_new()
    buf, used = C.create_string_buffer(1 << 16), C.c_size_t(0)
    assert lib_.archive_write_set_format_zip(a) == Z.ARCHIVE_OK
    assert lib_.archive_write_open_memory(a, buf, len(buf), C.byref(used)) == Z.ARCHIVE_OK
    for name, ftype in ((b"one", Z.AE_IFREG), (b"link", Z.AE_IFLNK), (b"two", Z.AE_IFREG)):
        lib_.archive_entry_clear(ent)
        lib_.archive_entry_set_pathname(ent, name)
        lib_.archive_entry_set_filetype(ent, ftype)
        lib_.archive_entry_set_perm(ent, 0o644)
        lib_.archive_entry_set_mtime(ent, 1700000000, 0)
        rc = lib_.archive_write_header(a, ent)
        assert rc == (Z.ARCHIVE_FAILED if ftype == Z.AE_IFLNK else Z.ARCHIVE_OK)
        if rc == Z.ARCHIVE_OK:
            assert lib_.archive_write_data(a, name, len(name)) == len(name)
    assert lib_.archive_write_close(a) == Z.ARCHIVE_OK
    img = buf.raw[:used.value]
    lib_.archive_entry_free(ent)
    lib_.archive_write_free(a)
    entries = [Z.Entry("one", b"one", size=None), Z.Entry("two", b"two", size=None)]
    Z.check_records(img, entries)


def test_empty_archive(lib):
    rc, img = Z.write_zip(lib, [])
    assert rc == Z.ARCHIVE_OK and img == b"PK\x05\x06" + bytes(18)


def test_many_entries_get_the_zip64_end_record(lib):
    rnd = random.Random(41)
    entries = [Z.Entry("f%05d" % i, rnd.randbytes(rnd.randint(0, 8)), mtime=1700000000 + i) for i in range(66000)]
    rc, img = Z.write_zip(lib, entries, finish_every=0)
    assert rc == Z.ARCHIVE_OK, img
    locals_, central, end = Z.parse(img)
    assert end["n"] == 0xFFFF and end["zip64"] is not None and end["zip64"]["n"] == 66000 and end["zip64"]["need"] == 45
    assert [c["name"] for c in central] == [e.name for e in entries]
    for i in [0, 65535, 65536, 65999] + rnd.sample(range(66000), 200):
        assert Z.zlib.decompressobj(-15).decompress(locals_[i]["data"]) == entries[i].data
        assert locals_[i]["desc"]["crc"] == Z.zlib.crc32(entries[i].data) == central[i]["crc"]


def test_through_the_gzip_write_filter(lib):
    entries = [e for e in Z.main_entries() if len(e.data) <= 300000]
    rc, gz = Z.write_zip(lib, entries, gzip_filter=True)
    assert rc == Z.ARCHIVE_OK, gz
    img = gzip.decompress(gz)
    Z.check_records(img, entries)
    Z.check_with_zipfile(img, entries)


def test_memory_sink_too_small(lib):
    entries = Z.main_entries()
    for cap in (100, 200000, 1 << 20):
        rc, err = Z.write_zip(lib, entries, (("compression", "store"),), cap=cap)
        assert rc == Z.ARCHIVE_FATAL and err == "Buffer exhausted", (cap, rc, err)


def test_device_error_on_the_second_window(lib, monkeypatch):
    lib._gpu_mock.la_gpu_zip_mock_reset()
    monkeypatch.setenv("LA_MOCK_ZIP_FAIL_CALL", "2")
    rc, err = Z.write_zip(lib, Z.main_entries())
    assert rc == Z.ARCHIVE_FATAL
    assert err == "zip GPU data plane: compress failed: mock: injected failure of call 2"
