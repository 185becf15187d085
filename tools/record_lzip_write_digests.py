#!/usr/bin/env python3
"""Records tests/golden/lzip_write_digests.json: size and SHA-256 of what la_gpu_lzip_compress writes for every named
input of tests/lzip_write_support.inputs() at levels 6 and 9 (one of each group of levels).  The bytes come from the CPU
stand-in of tests/mock_gpu/la_gpu_lzip_comp_mock.c, which compiles libarchive_amd/csrc/la_lzip_enc_dev.h as the kernels do; no GPU is
needed.  tests/test_lzip_write_digests.py holds the stand-in to the file, tests/test_gpu_lzip_compress.py the device.

    python3 tools/record_lzip_write_digests.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lzip_write_support as W     # noqa: E402


def main():
    s = W.StandIn()
    out = {"%s/%d" % (name, level): W.digest(s.compress(data, level)) for name, data in sorted(W.inputs().items()) for level in W.LEVELS}
    with open(W.GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d entries" % (W.GOLDEN, len(out)))


if __name__ == "__main__":
    main()
