"""ASan + UBSan over the lzop read path on the CPU: tests/mock_gpu/la_read_main.c is a program of its own that links
the host sources (read core, la_filter_lzop.c, la_bid_policy.c), the CPU mock of the device ABI and the stand-in for
la_gpu_lzop_decode (the kernel's rules header), all compiled with -fsanitize=address,undefined.  It reads valid,
multi-part, cut and damaged streams, each in one piece, 1000 bytes and 1 byte at a time, and has to exit 0 with nothing
reported and the reference's verdicts.  The sanitizer runtimes are linked into the program statically; the test
preloads nothing, changes nothing about what its environment preloads, and loads nothing into Python."""
import os
import subprocess

import lzop_support as L
import mock_build


def fnv1a(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_lzop_reader_under_asan_ubsan(tmp_path):
    out = str(tmp_path)
    exe = mock_build.program("la_read_asan")
    images = [img for _, img in sorted(L.filter_shapes().items())]
    images += [img for _, img in L.fixtures()]
    two = L.part(L.text(1, 3000), block_size=1200, flags=L.AU | L.AC, name=b"a name") + L.part(L.noise(2, 300, 16), flags=L.CC | L.EXTRA_FIELD)
    images += [two[:cut] for cut in range(9, len(two), 5)]
    bare = L.header(flags=0) + L.block(L.text(1, 1500), 0) + L.block(L.text(3, 1000), 0) + bytes(4)
    images += [L.flip(bare, b) for b in L.flip_cases(bare, 40)[::3]]
    # the rules cases, each as the only block of a stream without checksums: every verdict under the sanitizers
    images += [L.header(flags=0) + L.block(bytes(c[1]), 0, comp=c[0], stored=False) + bytes(4) for c in L.rules_cases().values() if 0 < c[1] and len(c[0]) < c[1]]
    paths = []
    for i, img in enumerate(images):
        paths.append(os.path.join(out, "img%04d.lzo" % i))
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
            data, rc, msg = L.reference_cat(img)
            assert line == ("%d %d %016x %s" % (rc, len(data), fnv1a(data), msg)), (line, len(img))
    # the bid policy's header walk under the sanitizers too: a look-ahead of 4 KiB over streams longer than that
    run = subprocess.run([exe] + paths[:60], env=dict(env, LA_GPU_BID="auto", LA_GPU_BID_LOOKAHEAD_KIB="4"),
                         capture_output=True, text=True, timeout=600)
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
