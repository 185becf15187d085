#!/usr/bin/env python3
"""lzop write side on the device: la_gpu_lzop_compress on one write window resident in HBM, against la_gpu_lz4_compress
at 64 KiB blocks on the same buffers in the same run (the same matcher, the natural yardstick), alternating; the CPU
stand-in of tests/mock_gpu compiled -O2 on ONE host core (the project's own emitter under a serial matcher: NOT liblzo2,
which is not on the machine); and the output size against the input and against tests/lzop_support.compress (an
exact-table greedy coder in Python) on one unit.

    python tools/measure_lzop_write.py [--mib 64] [--unit 4] [--reps 5] [--device-only] [--out FILE]

Three inputs, word text, noise and the bench stream's kind of data (tests/streams.synth_lz4_stream's plain bytes), `unit`
MiB each, tiled in HBM to `mib` MiB (blocks are coded alone, so a tile costs what its first copy costs).  One warm-up
call, then `reps` calls timed with events on the context's stream: median, min and max.  Before timing counts, the image
is walked on the host and every block is decoded by la_gpu_lzop_decode with its Adler-32 verified; the bytes have to be
the input.  --device-only leaves the host-side figures out (for a run under a profiler)."""
import argparse
import ctypes as C
import os
import random
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

BLOCK = 65536


def inputs(mib):
    import deflate_find_support as F
    import streams as S
    n = mib << 20
    frames = max(1, n // (16 * 65536))
    synth = S.synth_lz4_stream(0x4C413335, 0, frames, blocks_per_frame=16, block_size=65536, nthreads=8)[1].tobytes()[:n]
    return (("word text", F.word_text(n, seed=41)), ("noise", random.Random(18).randbytes(n)), ("bench-stream data", synth))


def stand_in(plain):
    """(image bytes, seconds) of the CPU stand-in's la_gpu_lzop_compress on one core: best of three"""
    import mock_build
    from libarchive_amd import _native as N
    lib = mock_build.gpu_lib()
    lib.la_gpu_lzop_compress.argtypes = [C.c_void_p, C.POINTER(N._LzopcBatchC)]
    cap = len(plain) + 12 * (len(plain) // BLOCK + 1)
    src, out, need = C.create_string_buffer(plain, len(plain)), C.create_string_buffer(cap), C.c_uint64(0)
    bt = N._LzopcBatchC()
    bt.d_src, bt.src_bytes, bt.block_size, bt.lead_bytes = C.addressof(src), len(plain), BLOCK, 0
    bt.d_out, bt.out_cap, bt.d_out_bytes = C.addressof(out), cap, C.addressof(need)
    best = None
    for _ in range(3):
        t = time.perf_counter()
        assert lib.la_gpu_lzop_compress(C.addressof(bt), C.byref(bt)) == 0
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return need.value, best


def walk(img):
    """[(payload offset, csize, usize, adler)] of blocks back to back"""
    out, at = [], 0
    while at < len(img):
        usize, csize, adler = struct.unpack_from(">III", img, at)
        out.append((at + 12, csize, usize, adler))
        at += 12 + csize
    assert at == len(img)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--unit", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import _native as N
    from libarchive_amd import lzop
    import lzop_support as L
    say("# tools/measure_lzop_write.py --mib %d --unit %d --reps %d%s" % (args.mib, args.unit, args.reps, " --device-only" if args.device_only else ""))
    tiles = max((args.mib + args.unit - 1) // args.unit, 1)
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    for name, plain in inputs(args.unit):
        n = tiles * len(plain)
        d_src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda().repeat(tiles)
        d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        # the image once, decoded by the device's own reader before any timing counts
        d_img = lzop.compress_window(ctx, d_src)
        img = d_img.cpu().numpy().tobytes()
        blocks = walk(img)
        entries, dst = [], 0
        for off, csize, usize, adler in blocks:
            entries.append({"src_off": off, "src_len": csize, "dst_off": dst, "dst_len": usize, "flags": lzop.U_ADLER32, "sum_u": adler})
            dst += usize
        plan = lzop.LzopDevicePlan(ctx, d_img, lzop.block_table(entries), dst_cap=n).run()
        res = plan.results()
        assert (res["status"] == 0).all() and torch.equal(plan.d_dst[:n], d_src)
        stored = sum(1 for _, c, u, _ in blocks if c == u)
        say("%s: %d MiB plain in %d blocks of 64 KiB (%d stored), image %.2f MiB = %.4f of the input (ratio %.3f); decoded by la_gpu_lzop_decode, "
            "Adler-32 verified, equal to the input" % (name, n >> 20, len(blocks), stored, len(img) / 2 ** 20, len(img) / n, n / len(img)))
        del plan, d_img
        # both compressors on the same buffers, alternating
        lz_cap = lzop.compress_bound(n)
        l4_cap = int(N.gpu_lib().la_gpu_lz4_compress_bound(n, BLOCK, 16))
        ctx.reserve(max(int(N.gpu_lib().la_gpu_lzop_compress_workspace_bytes(n, BLOCK)), int(N.gpu_lib().la_gpu_lz4_compress_workspace_bytes(n, BLOCK, 16))))
        d_out = torch.empty(max(lz_cap, l4_cap), dtype=torch.uint8, device="cuda")
        lz, l4 = N._LzopcBatchC(), N._Lz4cBatchC()
        lz.d_src, lz.src_bytes, lz.block_size, lz.lead_bytes = d_src.data_ptr(), n, BLOCK, 0
        lz.d_out, lz.out_cap, lz.d_out_bytes = d_out.data_ptr(), lz_cap, d_len.data_ptr()
        l4.d_src, l4.src_bytes, l4.block_size, l4.blocks_per_frame, l4.flags = d_src.data_ptr(), n, BLOCK, 16, 0
        l4.d_out, l4.out_cap, l4.d_out_bytes = d_out.data_ptr(), l4_cap, d_len.data_ptr()
        times = {"lzop": [], "lz4": []}
        sizes = {}
        for rep in range(args.reps + 1):     # the first round warms the workspace and the code objects
            for label, call, bt in (("lzop", ctx.lzop_compress, lz), ("lz4", ctx.lz4_compress, l4)):
                ctx.timer_start()
                call(bt)
                t_ms = ctx.timer_stop()
                sizes[label] = int(d_len.cpu()[0])
                if rep:
                    times[label].append(t_ms)
        for label in ("lzop", "lz4"):
            med = statistics.median(times[label])
            say("  la_gpu_%s_compress, 64 KiB blocks: median of %d calls %.2f ms (min %.2f, max %.2f) = %.1f GiB/s of input; %d bytes = %.4f of the input"
                % (label, len(times[label]), med, min(times[label]), max(times[label]), n / 2 ** 30 / (med / 1e3), sizes[label], sizes[label] / n))
        del d_out, d_src
        torch.cuda.empty_cache()
        if args.device_only:
            continue
        size, secs = stand_in(plain)
        say("  the CPU stand-in -O2 on one host core (the project's emitter under a serial matcher, NOT liblzo2): %.0f MiB/s, %d bytes = %.4f of the unit"
            % (len(plain) / 2 ** 20 / secs, size, size / len(plain)))
        greedy = sum(12 + min(len(L.compress(plain[i:i + BLOCK])), len(plain[i:i + BLOCK])) for i in range(0, len(plain), BLOCK))
        unit_img = len(img) // tiles
        say("  one unit of %d MiB: the device %d bytes, lzop_support.compress (exact-table greedy, Python) %d bytes: the device writes %.4f of it"
            % (args.unit, unit_img, greedy, unit_img / greedy))
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
