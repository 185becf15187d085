#!/usr/bin/env python3
"""bzip2 write side on the device: la_gpu_bzip2_compress on input resident in HBM, time per stage, against libbz2
(Python's bz2) on one host core of the same machine, and the write filter end to end, file to memory.

    python tools/measure_bzip2_write.py [--mib 64] [--levels 1,9] [--reps 2] [--baseline-mib 16] [--out FILE]

Two inputs, C2-like (the bench's synthetic lz4 corpus, plain side) and text-like (random words), one write window
(`mib` MiB) each.  Every repetition prints its own line: stream-ordered HIP events around the one call, buffers
allocated and the workspace reserved before.  Stages are la_gpu_profile_read's of the last repetition.  The libbz2
baseline compresses the first `baseline-mib` MiB of the same input (its rate does not depend on the length)."""
import argparse
import bz2
import ctypes as C
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def c2_like(mib):
    import streams as S
    _, plain = S.synth_lz4_stream(0x4C413335, 0, mib, blocks_per_frame=16, block_size=65536, nthreads=8)
    return plain.tobytes()


def text_like(mib):
    import zip_write_support as W
    return W.word_text(17, mib << 20)


def filter_write(lib, path, level, cap):
    """the archive path: read the file in 1 MiB pieces, archive_write_data, the stream in a memory buffer"""
    a = lib.archive_write_new()
    assert lib.archive_write_add_filter_bzip2(a) == 0 and lib.archive_write_set_format_raw(a) == 0
    assert lib.archive_write_set_filter_option(a, b"bzip2", b"compression-level", str(level).encode()) == 0
    buf = C.create_string_buffer(cap)
    used = C.c_size_t(0)
    assert lib.archive_write_open_memory(a, buf, cap, C.byref(used)) == 0
    assert lib.archive_write_header(a, None) == 0
    with open(path, "rb") as f:
        while True:
            piece = f.read(1 << 20)
            if not piece:
                break
            assert lib.archive_write_data(a, piece, len(piece)) == len(piece)
    assert lib.archive_write_close(a) == 0, lib.archive_error_string(a)
    lib.archive_write_free(a)
    return buf.raw[:used.value]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--levels", default="1,9")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--baseline-mib", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import _native as N
    from libarchive_amd import bzip2 as B
    from test_gpu_lz4_write import _lib_setup
    lib = _lib_setup(la.host_lib())
    lib.archive_write_add_filter_bzip2.argtypes = [C.c_void_p]
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    say("# tools/measure_bzip2_write.py --mib %d --levels %s --reps %d --baseline-mib %d" % (args.mib, args.levels, args.reps, args.baseline_mib))
    for name, gen in (("c2_like", c2_like), ("text_like", text_like)):
        plain = gen(args.mib)
        d_src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        n = len(plain)
        for level in [int(x) for x in args.levels.split(",")]:
            sample = plain[:args.baseline_mib << 20]
            t = time.time()
            ref = bz2.compress(sample, level)
            t_ref = time.time() - t
            cap = B.compress_bound(n, level)
            ws = int(N.gpu_lib().la_gpu_bzip2_compress_workspace_bytes(n, level))
            ctx.reserve(ws)
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
            d_state = torch.zeros(16, dtype=torch.uint8, device="cuda")
            b = N._Bz2cBatchC()
            b.d_src, b.src_bytes, b.level, b.flags = d_src.data_ptr(), n, level, B.LA_BZ2C_FIRST | B.LA_BZ2C_LAST
            b.d_state, b.d_out, b.out_cap, b.d_out_bytes = d_state.data_ptr(), d_out.data_ptr(), cap, d_len.data_ptr()
            ctx.bzip2_compress(b)       # warm-up
            ctx.sync()
            total = int(d_len.cpu()[0])
            img = d_out[:total].cpu().numpy().tobytes()
            assert bz2.decompress(img) == plain
            say("%s level %d: %d MiB plain, %d blocks, %.1f MiB compressed (ratio %.2f), workspace %.0f MiB; libbz2 on one core: %.1f MiB/s "
                "(ratio %.2f on the first %d MiB)" % (name, level, n >> 20, -(-n // B.compress_block_bytes(level)), total / 2 ** 20, n / total,
                                                     ws / 2 ** 20, len(sample) / 2 ** 20 / t_ref, len(sample) / len(ref), args.baseline_mib))
            ctx.profile_enable(True)
            for rep in range(args.reps):
                ctx.timer_start()
                ctx.bzip2_compress(b)
                ms = ctx.timer_stop()
                say("  rep %d: %.1f ms = %.0f MiB/s of input" % (rep, ms, n / 2 ** 20 / (ms / 1e3)))
            stages = ctx.profile_read()
            rounds = int(N.gpu_lib().la_gpu_bzip2_compress_sort_rounds(ctx._h))
            ctx.profile_enable(False)
            say("  stages (ms): " + ", ".join("%s %.1f" % kv for kv in sorted(stages, key=lambda kv: -kv[1])))
            say("  sort rounds run before every rank was distinct: %d (the later rounds' launches return at once)" % rounds)
            with tempfile.NamedTemporaryFile(suffix=".plain") as f:
                f.write(plain)
                f.flush()
                t = time.time()
                out = filter_write(lib, f.name, level, cap + 65536)
                dt = time.time() - t
            assert bz2.decompress(out) == plain
            say("  filter, file to memory: %.2f s = %.0f MiB/s of input (device open, pinned window, copies both ways included)"
                % (dt, n / 2 ** 20 / dt))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
