#!/usr/bin/env python3
"""Recorder of tests/golden/zstd_compress_entropy_parent.json: the SHA-256 of every image that
tests/test_gpu_zstd_compress_entropy.pinned_entropy_images names (key name/block size/blocks per frame/flags), written
by the data plane that LA_GPU_LIB selects -- a build of the commit whose bytes are to be pinned.
usage: LA_GPU_LIB=<parent's libla_gpu.so> python tools/record_zstd_entropy_digests.py [output file]"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import libarchive_amd as la
import test_gpu_zstd_compress_entropy as T

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN_ENTROPY
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    digests = {key: hashlib.sha256(img).hexdigest() for key, img in T.pinned_entropy_images(ctx)}
    ctx.close()
    with open(out, "w") as f:
        json.dump(digests, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d digests from %s -> %s" % (len(digests), la._native.GPU_LIB_PATH, out))
