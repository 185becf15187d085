"""ASan + UBSan over the bzip2 read path on the CPU: tests/mock_gpu/la_read_main.c is a program of its own that
links the host sources (read core, la_filter_bzip2.c), the CPU mock of the device ABI and the libbz2 stand-in for
la_gpu_bzip2_scan / la_gpu_bzip2_decode, all compiled with -fsanitize=address,undefined.  It reads valid, concatenated,
cut and damaged streams, each in one piece, 1000 bytes and 1 byte at a time, and has to exit 0 with nothing reported
and the reference's verdicts.  The sanitizer runtimes are linked into the program statically; the test preloads
nothing, changes nothing about what its environment preloads, and loads nothing into Python."""
import os
import random
import subprocess

import bzip2_support as BS
import mock_build


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_bzip2_reader_under_asan_ubsan(tmp_path):
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    big, small = BS.stream350k(), BS.stream3000()
    r = random.Random(77)
    images = list(BS.filter_shapes().values()) + [img for _, img in BS.fixtures()]
    images += [small[:c] for c in range(14, len(small), 97)] + [big[:r.randrange(14, len(big))] for _ in range(6)]
    images += [BS.flip(small, r.randrange(80, len(small) * 8)) for _ in range(40)]
    images += [BS.flip(big, r.randrange(80, len(big) * 8)) for _ in range(10)]
    paths = []
    for i, img in enumerate(images):
        paths.append(os.path.join(out, "img%03d.bz2" % i))
        with open(paths[-1], "wb") as f:
            f.write(img)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    run = subprocess.run([exe] + paths, env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(images)
    for img, line in zip(images, lines):
        data, rc, msg = BS.reference_cat(img)
        assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(img))
