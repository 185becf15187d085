#!/usr/bin/env python3
"""ONE gzip member whose pieces DEPEND on each other -- written by Python's zlib with Z_SYNC_FLUSH every 128 KiB, which is
the shape pigz writes without -i -- read back through la_cat with LA_GZIP_FLUSH_POINTS=chain (LA_GZ_OPT_CHAIN on the
device), beside
  - the whole-member decode of the same file (LA_GPU_BID=all, switch unset: the path the parent commit has for such a
    stream; --baseline-cat names another build's la_cat for it, e.g. the parent commit's; only up to --baseline-max-mib,
    it runs at a few MiB/s),
  - Python's zlib on one host core,
  - and, for a file of the same plain bytes written by this project's gzip:single-member filter (independent pieces),
    the =1 path and the chain path over it.
--keep PATH leaves the sync-flushed file there.  The per-kernel split comes from a run of its own under the profiler:
    rocprofv3 --kernel-trace --stats -d OUT -- libarchive_amd/host/la_cat FILE > /dev/null   (LA_GZIP_FLUSH_POINTS=chain)
usage (GPU box): python tools/measure_gzip_chain.py [--baseline-cat PATH] [--baseline-max-mib N] [--keep PATH] [MiB ...]"""
import os, subprocess, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("LA_GPU_BID", "all")
import numpy as np

args = sys.argv[1:]
base_cat, base_max, keep = None, 32, None
while args and args[0].startswith("--"):
    if args[0] == "--baseline-cat":
        base_cat = args[1]
    elif args[0] == "--baseline-max-mib":
        base_max = int(args[1])
    elif args[0] == "--keep":
        keep = args[1]
    args = args[2:]
cat = os.path.join(ROOT, "libarchive_amd", "host", "la_cat")
STEP = 128 << 10


def timed(exe, path, env, want, repeat):
    best = None
    for _ in range(repeat):
        t0 = time.time()
        r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, env=dict(os.environ, **env))
        dt = time.time() - t0
        assert r.returncode == 0 and r.stdout == want, r.stderr[-500:]
        best = dt if best is None else min(best, dt)
    return best


def sync_flushed(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    out = [c.compress(data[i:i + STEP]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(data), STEP)]
    return b"".join(out) + c.flush()


for mib in [int(x) for x in args] or [32]:
    rs = np.random.RandomState(mib)
    words = rs.randint(0, 256, size=(4096, 8), dtype=np.uint8)
    data = words[rs.randint(0, 4096, size=(mib << 20) // 8)].tobytes()
    gz = sync_flushed(data)
    t0 = time.time(); ok = zlib.decompress(gz, 31) == data; t_cpu = time.time() - t0
    assert ok
    path = keep or "/dev/shm/la_chain.gz"
    open(path, "wb").write(gz)
    chain_env = {"LA_GZIP_FLUSH_POINTS": "chain", "LA_GPU_BID": "auto"}
    t_chain = timed(cat, path, chain_env, data, 3)
    line = "sync-flushed member, %d MiB decoded (%d MiB compressed, %d markers): chain %.3f s -> %.1f MiB/s; zlib on one core %.2f s -> %.0f MiB/s" % (
        mib, len(gz) >> 20, gz.count(b"\x00\x00\xff\xff"), t_chain, mib / t_chain, t_cpu, mib / t_cpu)
    if mib <= base_max:
        t_whole = timed(base_cat or cat, path, {"LA_GPU_BID": "all", "LA_GZIP_FLUSH_POINTS": "0"}, data, 1)
        line += "; whole-member decode (%s) %.2f s -> %.1f MiB/s: chain is %.0f x" % (
            "baseline build" if base_cat else "this build, switch off", t_whole, mib / t_whole, t_whole / t_chain)
    print(line, flush=True)
    if not keep:
        os.unlink(path)
    # the independent pieces of this project's own writer: today's =1 path beside the chain path over the same file
    from test_gpu_lz4_write import ARCHIVE_OK, write_lz4
    rc, own = write_lz4(data, (("single-member", "1"),), 1 << 20, codec="gzip")
    assert rc == ARCHIVE_OK
    path2 = "/dev/shm/la_chain_own.gz"
    open(path2, "wb").write(own)
    t_one = timed(cat, path2, {"LA_GZIP_FLUSH_POINTS": "1", "LA_GPU_BID": "auto"}, data, 3)
    t_two = timed(cat, path2, chain_env, data, 3)
    print("gzip:single-member file, %d MiB decoded (%d MiB compressed): =1 %.3f s -> %.1f MiB/s; =chain %.3f s -> %.1f MiB/s" % (
        mib, len(own) >> 20, t_one, mib / t_one, t_two, mib / t_two), flush=True)
    os.unlink(path2)
