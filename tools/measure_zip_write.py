#!/usr/bin/env python3
"""Measurement: la_gpu_zip_compress (a write window of ZIP entries per call) on C2-like data resident in HBM, against
la_gpu_gzip_compress with LA_GZC_FRAME_STREAM on the same buffer -- the same kernels over an even chunk grid -- and
the archive path end to end (archive_write_set_format_zip, host copies and Python's calls included).
  shapes: the buffer as ONE segment; as entries of 64 KiB; as entries of 1 KiB (each entry LAST, gaps 46 + 16)
usage: python tools/measure_zip_write.py [MiB of input, default 1024] [--reps N, default 3] [--modes 0,1]
Every repetition prints its own line (stream-ordered HIP events around the one call, buffers allocated before)."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import libarchive_amd as la
from libarchive_amd import _native as N
import streams as S

argv = sys.argv[1:]


def opt(name, default):
    return argv[argv.index(name) + 1] if name in argv else default


reps = int(opt("--reps", "3"))
modes = [int(m) for m in opt("--modes", "0,1").split(",")]
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--modes", "--reps"))]
mib = int(pos[0]) if pos else 1024
CHUNK = 49152
NAMES = {0: "fixed", 1: "dynamic", 2: "stored"}
ctx = la.GpuContext(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
lib = N.gpu_lib()

_, plain = S.synth_lz4_stream(0x5A535444, 0, mib, 16, 65536, nthreads=16)
d_src = torch.from_numpy(plain).cuda()
n = int(d_src.numel())
d_len = torch.zeros(1, dtype=torch.int64, device="cuda")


def time_call(call):
    call()
    ctx.sync()
    out = []
    for _ in range(reps):
        ctx.timer_start()
        call()
        out.append(ctx.timer_stop())
    return out


def stream_call(mode):
    cap = int(lib.la_gpu_gzip_compress_bound(n, CHUNK))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    b = N._GzcBatchC()
    b.d_src, b.src_bytes, b.chunk_bytes, b.mtime, b.options, b.framing = d_src.data_ptr(), n, CHUNK, 0, mode, N.LA_GZC_FRAME_STREAM
    b.d_out, b.out_cap, b.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
    return (lambda: ctx.gzip_compress(b)), d_out


def zip_call(mode, entry):
    k = (n + entry - 1) // entry
    t = np.zeros(k, dtype=N.ZIPC_SEG_DTYPE)
    t["src_off"] = np.arange(k, dtype=np.uint64) * entry
    t["src_len"] = np.minimum(entry, n - t["src_off"].astype(np.int64))
    t["gap_before"], t["gap_after"], t["flags"] = 46, 16, N.LA_ZIPC_LAST
    cap = int(lib.la_gpu_zip_compress_bound(n, k, CHUNK, 62 * k))
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    d_segs = torch.from_numpy(t.view(np.uint8).reshape(-1).copy()).cuda()
    d_res = torch.zeros(k * N.ZIPC_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    b = N._ZipcBatchC()
    b.d_src, b.src_bytes, b.d_segs, b.n_segs, b.chunk_bytes, b.options = d_src.data_ptr(), n, d_segs.data_ptr(), k, CHUNK, mode
    b.d_out, b.out_cap, b.d_results, b.d_out_bytes = d_out.data_ptr(), cap, d_res.data_ptr(), d_len.data_ptr()

    def call():
        assert ctx.zip_compress(b) == N.LA_OK
    return call, (d_out, d_segs, d_res), k


for mode in modes:
    call, keep = stream_call(mode)
    base = time_call(call)
    size = int(d_len.cpu()[0])
    for ms in base:
        print("%4d MiB %-7s gzip_compress stream framing      %8.2f ms = %6.1f GB/s; %d bytes out" % (mib, NAMES[mode], ms, n / ms / 1e6, size), flush=True)
    del keep
    for label, entry in (("one segment", n), ("64 KiB entries", 65536), ("1 KiB entries", 1024)):
        call, keep, k = zip_call(mode, entry)
        ts = time_call(call)
        size = int(d_len.cpu()[0])
        for ms in ts:
            print("%4d MiB %-7s zip_compress %8d x %-14s %8.2f ms = %6.1f GB/s; %d bytes out; x%.3f of the stream framing's median"
                  % (mib, NAMES[mode], k, label, ms, n / ms / 1e6, size, ms / sorted(base)[len(base) // 2]), flush=True)
        del keep
        torch.cuda.empty_cache()

# the archive path end to end: entries of 64 KiB through archive_write_*, default window
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zip_write_support as Z
host = Z.setup(la.host_lib())
data = plain.tobytes()
for _ in range(reps):
    a, ent = host.archive_write_new(), host.archive_entry_new()
    cap = n + n // 8 + (n // 65536 + 1) * 200 + (1 << 20)
    buf, used = C.create_string_buffer(cap), C.c_size_t(0)
    assert host.archive_write_set_format_zip(a) == 0 and host.archive_write_open_memory(a, buf, cap, C.byref(used)) == 0
    t0 = time.time()
    for i in range(0, n, 65536):
        part = data[i:i + 65536]
        host.archive_entry_clear(ent)
        host.archive_entry_set_pathname(ent, b"dir/entry%07d" % (i >> 16))
        host.archive_entry_set_filetype(ent, Z.AE_IFREG)
        host.archive_entry_set_perm(ent, 0o644)
        host.archive_entry_set_mtime(ent, 1700000000, 0)
        host.archive_entry_set_size(ent, len(part))
        assert host.archive_write_header(a, ent) == 0 and host.archive_write_data(a, part, len(part)) == len(part)
    assert host.archive_write_close(a) == 0
    dt = time.time() - t0
    print("%4d MiB archive path, %d entries of 64 KiB, dynamic: %.1f ms = %.2f GB/s; %d bytes out"
          % (mib, (n + 65535) // 65536, dt * 1e3, n / dt / 1e9, used.value), flush=True)
    host.archive_entry_free(ent)
    host.archive_write_free(a)
ctx.close()
