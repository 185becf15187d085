#!/usr/bin/env python3
"""Measurement: what the entropy flags of la_gpu_zstd_compress buy.  For every input of the entropy tests
(tests/test_gpu_zstd_compress_entropy.INPUTS) and for the first 64 MiB of a real binary -- torch's libtorch_hip.so, or
the file given -- the stream bytes at flags 0, LA_ZSTDC_FULL_ALPHABET, LA_ZSTDC_FIT_TABLES and both (frames of one
128 KiB block, no checksum), and beside them libzstd at levels 1 and 3 on the same independent 128 KiB frames.
usage: python tools/measure_zstd_entropy.py [binary file]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import libarchive_amd as la
from libarchive_amd import zstd as LZ
import zstd_support as Z
import test_gpu_zstd_compress_entropy as T

BS = 131072


def libzstd_frames(z, data, level):
    return sum(len(Z.zstd_compress(z, data[i:i + BS], level)) for i in range(0, max(len(data), 1), BS))


if __name__ == "__main__":
    binary = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(torch.__file__), "lib", "libtorch_hip.so")
    with open(binary, "rb") as f:
        blob = f.read(64 << 20)
    inputs = list(T.INPUTS) + [("%s[:%d MiB]" % (os.path.basename(binary), len(blob) >> 20), blob)]
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    z = Z.libzstd()
    print("%-28s %10s %10s %10s %10s %10s %10s %10s" % ("input", "bytes", "flags 0", "FULL", "FIT", "FULL|FIT", "libzstd -1", "libzstd -3"))
    for name, data in inputs:
        d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda() if data else torch.empty(0, dtype=torch.uint8, device="cuda")
        sizes = []
        for flags in (0, LZ.LA_ZSTDC_FULL_ALPHABET, LZ.LA_ZSTDC_FIT_TABLES, LZ.LA_ZSTDC_FULL_ALPHABET | LZ.LA_ZSTDC_FIT_TABLES):
            img = LZ.compress_to_frames(ctx, d, BS, 1, flags)
            sizes.append(int(img.numel()))
            if flags == 12:
                assert Z.zstd_decompress(z, img.cpu().numpy().tobytes(), len(data) + 16) == data, name
        print("%-28s %10d %10d %10d %10d %10d %10d %10d" % ((name, len(data)) + tuple(sizes) + (libzstd_frames(z, data, 1), libzstd_frames(z, data, 3))), flush=True)
    ctx.close()
