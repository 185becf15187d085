#!/usr/bin/env python3
"""Measurement: la_gpu_gzip_compress (device gzip compression, the write filter's data plane), resident in HBM, in its
three block modes (LA_GZC_FIXED, LA_GZC_DYNAMIC, LA_GZC_STORED).  Input GB/s and ratio on C2-like data (the plain bytes
of streams.synth_lz4_stream) and on ASCII word text; zlib levels 1 and 6 on a 16 MiB host sample next to them; the
device read side's decode speed on the stream the dynamic mode wrote.  Every mode is measured in both framings
(LA_GZC_FRAME_MEMBERS, LA_GZC_FRAME_STREAM): a line each, with the output size.
usage: python tools/measure_gzip_compress.py [GiB of C2-like input, default 4] [--once] [--modes 0,1,2] [--reps N]
           [--framings 0,1]
  --once: one compression of each input in each mode and nothing else (for a rocprofv3 --kernel-trace --stats run)
  --reps: timed repetitions of the whole measurement per mode (each prints its own line; default 1)"""
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import libarchive_amd as la
from libarchive_amd import gzip as LG
import la_api
import streams as S

argv = sys.argv[1:]


def opt(name, default):
    return argv[argv.index(name) + 1] if name in argv else default


once = "--once" in argv
modes = [int(m) for m in opt("--modes", "0,1,2").split(",")]
reps = int(opt("--reps", "1"))
framings = [int(f) for f in opt("--framings", "0,1").split(",")]
pos = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] not in ("--modes", "--reps", "--framings"))]
gib = int(pos[0]) if pos else 4
NAMES = {0: "fixed", 1: "dynamic", 2: "stored"}
FRAMES = {0: "members", 1: "stream"}
ctx = la.GpuContext(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

_, c2 = S.synth_lz4_stream(0x5A535444, 0, gib * 1024, 16, 65536, nthreads=16)
rng = np.random.default_rng(7)
letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
words = [bytes(rng.choice(letters, rng.integers(2, 10))) + b" " for _ in range(2000)]
text16 = b"".join(words[i] for i in rng.integers(0, len(words), 3 << 20))[:16 << 20]
text = np.tile(np.frombuffer(text16, dtype=np.uint8), gib * 64 // 4)        # a quarter of the C2 size
inputs = [("c2_like", c2), ("text", text)]


def timed(fn, n=3):
    fn()
    ctx.sync()
    t0 = time.time()
    for _ in range(n):
        fn()
    ctx.sync()
    return (time.time() - t0) / n


for name, plain in inputs:
    d_plain = torch.from_numpy(plain).cuda()
    n = int(d_plain.numel())
    if once:
        for m in modes:
            for fr in framings:
                LG.compress_to_members(ctx, d_plain, options=m, framing=fr)
        ctx.sync()
        continue
    sample = plain[:16 << 20].tobytes()
    z1, z6 = len(sample) / len(zlib.compress(sample, 1)), len(sample) / len(zlib.compress(sample, 6))
    for m in modes:
        for fr in framings:
            img = LG.compress_to_members(ctx, d_plain, options=m, framing=fr)
            size = int(img.numel())
            del img
            for _ in range(reps):
                dt = timed(lambda: LG.compress_to_members(ctx, d_plain, options=m, framing=fr))
                print("%-8s %5.2f GiB in: gzip_compress %-7s %-7s %7.1f ms = %5.1f GB/s; %d bytes out, ratio %.3f "
                      "(zlib -1 %.3f, -6 %.3f on 16 MiB)" % (name, n / 2**30, NAMES[m], FRAMES[fr], dt * 1e3, n / dt / 1e9,
                                                            size, n / size, z1, z6), flush=True)
    if 1 in modes:
        # the device read side on what the dynamic mode wrote, through the filter (a 256 MiB piece)
        piece = d_plain[:256 << 20]
        img = LG.compress_to_members(ctx, piece, options=1).cpu().numpy().tobytes()
        t0 = time.time()
        r = la_api.cat(img)
        dt = time.time() - t0
        assert r.data == piece.cpu().numpy().tobytes()
        print("%-8s read path (la_api.cat, host copies included) on %d MiB of the dynamic stream: %.1f ms = %.2f GB/s"
              % (name, int(piece.numel()) >> 20, dt * 1e3, int(piece.numel()) / dt / 1e9), flush=True)
    del d_plain
    torch.cuda.empty_cache()
ctx.close()
