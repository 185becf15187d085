#!/usr/bin/env python3
"""ONE gzip member written by this project's own gzip:single-member filter (the 32 MiB shape of
tools/measure_single_member_gz.py, and larger), read back through la_cat in piece mode (LA_GZIP_FLUSH_POINTS=1), beside
the whole-member decode of the same file (LA_GPU_BID=all without the switch; --baseline-cat names another build's
la_cat for that, e.g. the parent commit's) and Python's zlib on one core.
usage (GPU box): python tools/measure_gzip_flush_points.py [--baseline-cat PATH] [--baseline-max-mib N] [MiB ...]"""
import os, subprocess, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("LA_GPU_BID", "all")
import numpy as np
from test_gpu_lz4_write import ARCHIVE_OK, write_lz4

args = sys.argv[1:]
base_cat, base_max = None, 32
while args and args[0].startswith("--"):
    if args[0] == "--baseline-cat":
        base_cat = args[1]
    elif args[0] == "--baseline-max-mib":
        base_max = int(args[1])
    args = args[2:]
cat = os.path.join(ROOT, "libarchive_amd", "host", "la_cat")


def timed(exe, path, env, want, repeat):
    best = None
    for _ in range(repeat):
        t0 = time.time()
        r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=dict(os.environ, **env))
        dt = time.time() - t0
        assert r.returncode == 0 and r.stdout == want, r.stderr[-500:]
        best = dt if best is None else min(best, dt)
    return best


for mib in [int(x) for x in args] or [32]:
    rs = np.random.RandomState(mib)
    words = rs.randint(0, 256, size=(4096, 8), dtype=np.uint8)
    data = words[rs.randint(0, 4096, size=(mib << 20) // 8)].tobytes()
    rc, gz = write_lz4(data, (("single-member", "1"),), 1 << 20, codec="gzip")
    assert rc == ARCHIVE_OK
    t0 = time.time(); ok = zlib.decompress(gz, 31) == data; t_cpu = time.time() - t0
    assert ok
    path = "/dev/shm/la_flush_points.gz"
    open(path, "wb").write(gz)
    t_piece = timed(cat, path, {"LA_GZIP_FLUSH_POINTS": "1", "LA_GPU_BID": "auto"}, data, 3)
    line = "single member, %d MiB decoded (%d MiB compressed, %d markers): piece mode %.3f s -> %.1f MiB/s; zlib on one core %.2f s -> %.0f MiB/s" % (
        mib, len(gz) >> 20, gz.count(b"\x00\x00\xff\xff"), t_piece, mib / t_piece, t_cpu, mib / t_cpu)
    if mib <= base_max:
        t_whole = timed(base_cat or cat, path, {"LA_GPU_BID": "all", "LA_GZIP_FLUSH_POINTS": "0"}, data, 1)
        line += "; whole-member decode (%s) %.2f s -> %.1f MiB/s: piece mode is %.0f x" % (
            "baseline build" if base_cat else "this build, switch off", t_whole, mib / t_whole, t_whole / t_piece)
    print(line, flush=True)
    os.unlink(path)
