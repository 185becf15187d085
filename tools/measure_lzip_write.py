#!/usr/bin/env python3
"""lzip write side.  Two parts:

  --sizes     no GPU: the CPU stand-in of tests/mock_gpu (the kernels' rules header, so the device's bytes) over the
              first `baseline-mib` MiB of each input at levels 6 and 9, against liblzma's raw LZMA1 (preset 0 and 6, one
              stream with the end marker) and against the same coded per 64 KiB piece; the expansion on noise.
  (default)   on the device: la_gpu_lzip_compress on a window resident in HBM at levels 6 and 9 (median of three calls
              after a warm-up, timed by stream events, split by stage), la_gpu_xz_compress level 0 on the same input in
              the same run (the same chain per 64 KiB), and liblzma's raw LZMA1 on one host core.

    python tools/measure_lzip_write.py [--sizes] [--mib 64] [--baseline-mib 8] [--out FILE]

Inputs: text (xz_support.text), noise, and the C2-like plain side of the bench's synthetic lz4 corpus."""
import argparse
import lzma
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from measure_xz_write import c2_like, noise, text_like  # noqa: E402


def raw_lzma1(data, preset, piece=None):
    """bytes of liblzma's raw LZMA1 streams (lc 3, lp 0, pb 2, end marker) over `data` cut every `piece` bytes"""
    f = [{"id": lzma.FILTER_LZMA1, "preset": preset, "lc": 3, "lp": 0, "pb": 2}]
    piece = piece or max(len(data), 1)
    return sum(len(lzma.compress(data[i:i + piece], format=lzma.FORMAT_RAW, filters=f)) for i in range(0, max(len(data), 1), piece))


def sizes(args, say):
    import lzip_write_support as W
    s = W.StandIn()
    for name, gen in (("text", text_like), ("noise", noise), ("c2_like", c2_like)):
        sample = gen(args.baseline_mib)
        n = len(sample)
        ours = {lv: len(s.compress(sample, lv)) for lv in (6, 9)}
        members = {lv: -(-n // W.member_bytes(lv)) for lv in (6, 9)}
        say("%s, %d MiB: level 6 %d bytes (ratio %.3f), level 9 %d bytes (ratio %.3f): the 256 KiB member is %.4f of the 64 KiB one"
            % (name, args.baseline_mib, ours[6], n / ours[6], ours[9], n / ours[9], ours[9] / ours[6]))
        for preset in (0, 6):
            one, per64, per256 = raw_lzma1(sample, preset), raw_lzma1(sample, preset, 1 << 16), raw_lzma1(sample, preset, 1 << 18)
            say("  liblzma raw LZMA1 preset %d: one stream %d bytes, per 64 KiB %d, per 256 KiB %d; streams alone (framing of 26 bytes taken off): "
                "level 6 is %.3f of per-64-KiB, level 9 %.3f of per-256-KiB, %.3f and %.3f of one stream"
                % (preset, one, per64, per256, (ours[6] - 26 * members[6]) / per64, (ours[9] - 26 * members[9]) / per256,
                   (ours[6] - 26 * members[6]) / one, (ours[9] - 26 * members[9]) / one))
        if name == "noise":
            say("  expansion on noise: level 6 %.4f, level 9 %.4f of the input (the bound is 7.00)" % (ours[6] / n, ours[9] / n))


def device(args, say):
    import torch
    import libarchive_amd as la
    from libarchive_amd import _native as N
    from libarchive_amd import lzip as L
    from libarchive_amd import xz as X
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for name, gen in (("text", text_like), ("noise", noise), ("c2_like", c2_like)):
        plain = gen(args.mib)
        n = len(plain)
        sample = plain[:args.baseline_mib << 20]
        for preset in (0, 6):
            t = time.time()
            ref = raw_lzma1(sample, preset)
            dt = time.time() - t
            say("%s: liblzma raw LZMA1 preset %d on one core: %.1f MiB/s, ratio %.3f (first %d MiB)"
                % (name, preset, len(sample) / 2 ** 20 / dt, len(sample) / ref, args.baseline_mib))
        d_src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        runs = [("lzip level %d" % lv, lv, L.compress_bound(n, lv), int(N.gpu_lib().la_gpu_lzip_compress_workspace_bytes(n, lv))) for lv in (6, 9)]
        runs.append(("xz level 0", None, X.compress_bound(n, 0), int(N.gpu_lib().la_gpu_xz_compress_workspace_bytes(n))))
        for label, level, cap, ws in runs:
            ctx.reserve(ws)
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            if level is None:
                bt, call = N._XzcBatchC(), ctx.xz_compress
                bt.level, bt.flags = 0, X.LA_XZC_FIRST
            else:
                bt, call = N._LzcBatchC(), ctx.lzip_compress
                bt.level, bt.flags = level, 0
            bt.d_src, bt.src_bytes = d_src.data_ptr(), n
            bt.d_out, bt.out_cap, bt.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
            call(bt)        # warm-up
            ctx.sync()
            total = int(d_len.cpu()[0])
            say("%s, %s: %d MiB plain, %.2f MiB compressed (ratio %.3f), workspace %.0f MiB, output buffer %.0f MiB"
                % (name, label, n >> 20, total / 2 ** 20, n / total, ws / 2 ** 20, cap / 2 ** 20))
            ctx.profile_enable(True)
            times = []
            for _ in range(3):
                ctx.timer_start()
                call(bt)
                times.append(ctx.timer_stop())
            stages = ctx.profile_read()
            ctx.profile_enable(False)
            ms = sorted(times)[1]
            say("  one call, median of three: %.1f ms = %.0f MiB/s of input (%s)" % (ms, n / 2 ** 20 / (ms / 1e3), ", ".join("%.1f" % t for t in times)))
            say("  stages of the last call (ms): " + ", ".join("%s %.1f" % kv for kv in sorted(stages, key=lambda kv: -kv[1])))
            del d_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--baseline-mib", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# tools/measure_lzip_write.py%s --mib %d --baseline-mib %d" % (" --sizes" if args.sizes else "", args.mib, args.baseline_mib))
    (sizes if args.sizes else device)(args, say)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
