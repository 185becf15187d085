#!/usr/bin/env python3
"""Measurement: la_gpu_zstd_compress (device zstd compression, the write filter's data plane), resident in HBM.
Input GB/s on C2-like data (the plain bytes of streams.synth_lz4_stream) and on ASCII word text; the compression
ratio next to libzstd levels 1 and 3 on the host (ZSTD_compress through ctypes, on a 64 MiB sample) and next to the
device lz4 and gzip writers; the device read side's decode speed on the written stream.
usage: python tools/measure_zstd_compress.py [GiB of C2-like input, default 4] [--once]
  --once: one compression of each input and nothing else (for a rocprofv3 --kernel-trace --stats run)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import libarchive_amd as la
from libarchive_amd import gzip as LG
from libarchive_amd import lz4 as LL
from libarchive_amd import zstd as LZ
import streams as S
import zstd_support as Z

args = [a for a in sys.argv[1:] if not a.startswith("--")]
once = "--once" in sys.argv
gib = int(args[0]) if args else 4
ctx = la.GpuContext(0)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)

_, c2 = S.synth_lz4_stream(0x5A535444, 0, gib * 1024, 16, 65536, nthreads=16)
rng = np.random.default_rng(7)
letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
words = [bytes(rng.choice(letters, rng.integers(2, 10))) + b" " for _ in range(2000)]
text16 = b"".join(words[i] for i in rng.integers(0, len(words), 3 << 20))[:16 << 20]
text = np.tile(np.frombuffer(text16, dtype=np.uint8), gib * 64 // 4)        # a quarter of the C2 size
inputs = [("c2_like", c2), ("text", text)]


def timed(fn, reps=3):
    fn()
    ctx.sync()
    t0 = time.time()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.time() - t0) / reps


for name, plain in inputs:
    d_plain = torch.from_numpy(plain).cuda()
    n = int(d_plain.numel())
    if once:
        LZ.compress_to_frames(ctx, d_plain)
        ctx.sync()
        continue
    img = LZ.compress_to_frames(ctx, d_plain)
    dt = timed(lambda: LZ.compress_to_frames(ctx, d_plain))
    dt_raw = timed(lambda: LZ.compress_to_frames(ctx, d_plain, flags=1 | 2))
    ratio = n / int(img.numel())
    lz4_ratio = n / int(LL.compress_to_frames(ctx, d_plain).numel())
    gz_ratio = n / int(LG.compress_to_members(ctx, d_plain).numel())
    # the device read side on the written stream
    host_img = img.cpu().numpy()
    frames, end_kind, consumed, dst_bytes = LZ.index_image(host_img, cap=(n >> 17) + 16)
    plan = LZ.ZstdDevicePlan(ctx, img, frames, dst_bytes)
    plan.run()
    res = plan.results()
    assert (res["status"] == 0).all() and int(res["out_len"].sum()) == n
    dt_dec = timed(plan.run)
    # libzstd on the host, on a 64 MiB sample
    z = Z.libzstd()
    sample = plain[:64 << 20].tobytes()
    z1 = len(sample) / len(Z.zstd_compress(z, sample, 1))
    z3 = len(sample) / len(Z.zstd_compress(z, sample, 3))
    dev_sample = LZ.compress_to_frames(ctx, d_plain[:64 << 20])
    assert Z.zstd_decompress(z, dev_sample.cpu().numpy().tobytes(), len(sample)) == sample
    print("%-8s %5.2f GiB in: zstd_compress %.1f ms = %.1f GB/s (raw literals %.1f GB/s); ratio %.3f "
          "(device lz4 %.3f, device gzip %.3f, libzstd -1 %.3f, -3 %.3f on 64 MiB); "
          "device decode of the written stream %.1f ms = %.1f GB/s"
          % (name, n / 2**30, dt * 1e3, n / dt / 1e9, n / dt_raw / 1e9, ratio, lz4_ratio, gz_ratio, z1, z3,
             dt_dec * 1e3, n / dt_dec / 1e9), flush=True)
    del plan, img, d_plain
    torch.cuda.empty_cache()
ctx.close()
