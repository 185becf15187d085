"""The lzip filter source compiles unchanged against libarchive's REAL private headers (-DLA_IN_LIBARCHIVE), as
tests/test_dropin_boundary.py checks for the other filters, and the core registers it through a weak reference so that
libraries that leave the file out still load."""
import os
import subprocess

import la_api
from test_dropin_boundary import REF_FLAGS, ROOT, needs_ref


@needs_ref
def test_lzip_filter_compiles_against_the_real_private_headers():
    cmd = ["gcc", "-fsyntax-only", "-Wall", "-Werror=implicit-function-declaration", "-DLA_IN_LIBARCHIVE",
           "-I" + ROOT + "/include", os.path.join(ROOT, "libarchive_amd", "host", "la_filter_lzip.c")] + REF_FLAGS
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]


def test_registration_is_weak_in_the_core_and_strong_in_the_library():
    import libarchive_amd as la
    lib = la.host_lib()
    assert hasattr(lib, "archive_read_support_filter_lzip")
    src = open(os.path.join(ROOT, "libarchive_amd", "host", "la_read_core.c")).read()
    assert "archive_read_support_filter_lzip(struct archive *) __attribute__((weak))" in src
    header = open(os.path.join(ROOT, "include", "la_archive.h")).read()
    assert "archive_read_support_filter_lzip" in header and "#define ARCHIVE_FILTER_LZIP 9" in header
    assert la_api.ARCHIVE_OK == 0
    gpu = la.gpu_lib()
    assert all(hasattr(gpu, n) for n in ("la_gpu_lzip_scan", "la_gpu_lzip_decode", "la_gpu_lzip_workspace_bytes"))
