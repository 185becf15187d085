"""ASan + UBSan over the lzip read path on the CPU: tests/mock_gpu/la_read_main.c is a program of its own that links
the host sources (read core, la_filter_lzip.c, la_bid_policy.c), the CPU mock of the device ABI and the stand-ins for
la_gpu_lzip_scan / la_gpu_lzip_decode (the kernel's rules headers), all compiled with -fsanitize=address,undefined.  It
reads valid, multi-member, cut and damaged streams, each in one piece, 1000 bytes and 1 byte at a time, and has to exit
0 with nothing reported and the reference's verdicts.  The sanitizer runtimes are linked into the program statically;
the test preloads nothing, changes nothing about what its environment preloads, and loads nothing into Python."""
import os
import subprocess

import lzip_support as LS
import mock_build

# (read 1 byte at a time the reference meets these errors in a call of its own: la_filter_lzip.c's head comment)
WHOLE_READS_ONLY = {"bad_crc_at_64k", "bad_crc_at_128k"}


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_lzip_reader_under_asan_ubsan(tmp_path):
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    images = [img for name, img in sorted(LS.filter_shapes().items()) if name not in WHOLE_READS_ONLY and len(img) < 1 << 17]
    images += [img for _, img in LS.fixtures()]
    two = LS.member(LS.text(1, 5000)) + LS.member(LS.noise(2, 700, 16))
    images += [two[:cut] for cut in range(6, len(two), 5)]
    images += [LS.flip(LS.three()[0], b) for b in LS.flip_cases()[::4]]
    paths = []
    for i, img in enumerate(images):
        paths.append(os.path.join(out, "img%04d.lz" % i))
        with open(paths[-1], "wb") as f:
            f.write(img)
    env = dict(os.environ, LA_GPU_BID="all", ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")     # (the environment is otherwise the caller's)
    for k in range(0, len(paths), 400):
        run = subprocess.run([exe] + paths[k:k + 400], env=env, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
        assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
        lines = run.stdout.splitlines()
        assert len(lines) == len(paths[k:k + 400])
        for img, line in zip(images[k:k + 400], lines):
            data, rc, msg = LS.reference_cat(img)
            assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(img))
    # the bid policy's look-ahead walk under the sanitizers too: a look-ahead of 4 KiB over streams longer than that
    run = subprocess.run([exe] + paths[:40], env=dict(env, LA_GPU_BID="auto", LA_GPU_BID_LOOKAHEAD_KIB="4"),
                         capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
