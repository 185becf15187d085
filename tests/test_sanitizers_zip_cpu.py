"""ASan + UBSan over the ZIP write path on the CPU: tests/mock_gpu/zip_write_main.c is a program of its own that links
the host sources (write core, la_write_zip.c), the CPU mock of the device ABI and the zlib stand-in for
la_gpu_zip_compress, all compiled with -fsanitize=address,undefined.  It writes a 3 000-entry archive to memory
(directories, entries with and without a size, entries written past their size, a refused symbolic link, windows of
1 MiB) and has to exit 0 with nothing reported.  The sanitizer runtimes are linked into the program statically; the
test preloads nothing, changes nothing about what its environment preloads, and loads nothing into Python."""
import os
import subprocess

import mock_build


def test_zip_writer_under_asan_ubsan():
    exe = mock_build.program("zip_write_asan")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    run = subprocess.run([exe, "3000"], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.startswith("ok 3000 "), run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
