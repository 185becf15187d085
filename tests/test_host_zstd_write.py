"""The zstd write filter's registration and options (host/la_write_zstd.c) on the product library, without a device:
nothing before archive_write_open touches the GPU.  The option table is the one of the reference's
libarchive/test/test_write_filter_zstd.c (the archive_write_set_filter_option assertions after its round trip), for
the filter built without libzstd's own bounds, plus every option the filter documents."""
import ctypes as C

import pytest

import libarchive_amd as la

ARCHIVE_OK, ARCHIVE_FAILED = 0, -25

REFERENCE_TABLE = [
    ("nonexistent-option", "0", ARCHIVE_FAILED),
    ("compression-level", "abc", ARCHIVE_FAILED),
    ("compression-level", "25", ARCHIVE_FAILED),
    ("compression-level", "9", ARCHIVE_OK),
    ("compression-level", "7", ARCHIVE_OK),
    ("threads", "-1", ARCHIVE_FAILED),
    ("threads", "4", ARCHIVE_OK),
    ("frame-per-file", "", ARCHIVE_OK),
    ("min-frame-out", "", ARCHIVE_FAILED),
    ("min-frame-out", "-1", ARCHIVE_FAILED),
] + [(k, v, ARCHIVE_OK) for k in ("min-frame-out", "min-frame-in")
     for v in ("0", "1048576", "1k", "1kB", "1M", "1MB", "1G", "1GB")] + [
    ("min-frame-in", "", ARCHIVE_FAILED),
    ("min-frame-in", "-1", ARCHIVE_FAILED),
] + [(k, v, ARCHIVE_FAILED) for k in ("max-frame-in", "max-frame-out") for v in ("", "-1", "0", "1023")] + [
    (k, v, ARCHIVE_OK) for k in ("max-frame-in", "max-frame-out")
    for v in ("1024", "1048576", "1k", "1kB", "1M", "1MB", "1G", "1GB")] + [
    ("long", "23", ARCHIVE_OK),
    ("long", "-1", ARCHIVE_FAILED),
]

FILTER_TABLE = [
    ("compression-level", "-99", ARCHIVE_OK), ("compression-level", "-100", ARCHIVE_FAILED),
    ("compression-level", "0", ARCHIVE_OK), ("compression-level", "22", ARCHIVE_OK),
    ("compression-level", "23", ARCHIVE_FAILED), ("compression-level", None, ARCHIVE_FAILED),
    ("compression-level", "3x", ARCHIVE_FAILED),
    ("threads", "0", ARCHIVE_OK), ("threads", "x", ARCHIVE_FAILED),
    ("frame-per-file", None, ARCHIVE_OK),
    ("min-frame-size", "5k", ARCHIVE_OK), ("min-frame-size", "-5", ARCHIVE_FAILED),
    ("min-frame-in", "12T", ARCHIVE_FAILED), ("min-frame-in", "1kBB", ARCHIVE_FAILED),
    ("max-frame-size", "64k", ARCHIVE_OK), ("max-frame-size", "1000", ARCHIVE_FAILED),
    ("max-frame-in", "128k", ARCHIVE_OK), ("max-frame-in", "+5", ARCHIVE_FAILED),
    ("long", "10", ARCHIVE_OK), ("long", "31", ARCHIVE_OK), ("long", "9", ARCHIVE_FAILED), ("long", "32", ARCHIVE_FAILED),
    ("long", None, ARCHIVE_FAILED),
    ("block-size", "4", ARCHIVE_FAILED),
]


def _lib():
    lib = la.host_lib()
    lib.archive_write_new.restype = C.c_void_p
    for f in ("archive_write_add_filter_zstd", "archive_write_set_format_raw", "archive_write_free"):
        getattr(lib, f).argtypes = [C.c_void_p]
    lib.archive_write_set_filter_option.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p]
    lib.archive_error_string.argtypes = [C.c_void_p]
    lib.archive_error_string.restype = C.c_char_p
    return lib


@pytest.mark.parametrize("table", [REFERENCE_TABLE, FILTER_TABLE], ids=["reference", "filter"])
@pytest.mark.parametrize("module", [None, "zstd"])
def test_option_table(table, module):
    lib = _lib()
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_zstd(a) == ARCHIVE_OK
        assert lib.archive_write_set_format_raw(a) == ARCHIVE_OK
        for key, value, want in table:
            rc = lib.archive_write_set_filter_option(a, module and module.encode(), key.encode(),
                                                     None if value is None else value.encode())
            assert rc == want, (key, value, rc)
            if rc == ARCHIVE_FAILED:
                assert b"Undefined option" in lib.archive_error_string(a)
    finally:
        lib.archive_write_free(a)


def test_options_of_other_filters_do_not_reach_it():
    lib = _lib()
    a = lib.archive_write_new()
    try:
        assert lib.archive_write_add_filter_zstd(a) == ARCHIVE_OK
        assert lib.archive_write_set_filter_option(a, b"lz4", b"compression-level", b"3") == ARCHIVE_FAILED
        assert lib.archive_write_set_filter_option(a, b"zstd", b"compression-level", b"3") == ARCHIVE_OK
    finally:
        lib.archive_write_free(a)
