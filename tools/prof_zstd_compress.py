#!/usr/bin/env python3
"""One input shape through la_gpu_zstd_compress a few times and nothing else: the program of a
`rocprofv3 --kernel-trace --stats` run that times zstd_compress_blocks_kernel.
usage: python tools/prof_zstd_compress.py text|skewed FLAGS [MiB, default 1024] [launches, default 4]
The input is 16 MiB of the shape (seeded), tiled on the device; blocks are compressed independently, so tiling changes
nothing a block sees.  LA_GPU_LIB selects another build of the data plane (the parent's, for an A/B in one session)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import libarchive_amd as la
from libarchive_amd import zstd as LZ


def shape_bytes(kind, n, seed=7):
    """n bytes of `text` (words of 2..9 lower-case letters from a list of 2 000) or `skewed` (i.i.d. bytes
    min(255, floor(Exp(0.03))): all 256 values occur, order-0 entropy about 6.5 bits)"""
    rng = np.random.default_rng(seed)
    if kind == "skewed":
        return np.minimum(255, rng.exponential(1 / 0.03, n)).astype(np.uint8)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    words = [bytes(rng.choice(letters, rng.integers(2, 10))) + b" " for _ in range(2000)]
    return np.frombuffer(b"".join(words[i] for i in rng.integers(0, len(words), n // 4 + 16))[:n], dtype=np.uint8).copy()


if __name__ == "__main__":
    kind, flags = sys.argv[1], int(sys.argv[2])
    mib = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    launches = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    unit = torch.from_numpy(shape_bytes(kind, 16 << 20)).cuda()
    d_plain = unit.repeat(max(1, mib // 16))[:mib << 20].contiguous()
    total = 0
    for _ in range(launches):
        total = int(LZ.compress_to_frames(ctx, d_plain, flags=flags).numel())
    ctx.sync()
    print("%s flags %d: %d MiB in, %d bytes out, %d launches" % (kind, flags, mib, total, launches), flush=True)
    ctx.close()
