#!/usr/bin/env python3
"""xz write side on the device: la_gpu_xz_compress on input resident in HBM (median of three calls after a warm-up, timed
by stream events, split by stage), and the write filter end to end, file to memory, against liblzma on one host core
(Python's lzma) on the same box and the same bytes: preset 0 and preset 6, as one stream and as raw LZMA2 per 1 MiB block.
A CPU-only comparison says what the state reset per 64 KiB costs in size: liblzma preset 0 coded per 1 MiB block against
the same coded per 64 KiB piece.

    python tools/measure_xz_write.py [--mib 64] [--levels 0,6] [--baseline-mib 8] [--out FILE]

Inputs: text (xz_support.text), noise, and the C2-like plain side of the bench's synthetic lz4 corpus.  The liblzma
baselines compress the first `baseline-mib` MiB of the same input."""
import argparse
import ctypes as C
import lzma
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def text_like(mib):
    import xz_support as XS
    unit = XS.text(17, 1 << 20)
    r = random.Random(17)
    out = bytearray()
    while len(out) < mib << 20:      # 1 MiB of the generator's text, cut at random places: no two blocks alike
        a = r.randrange(len(unit) // 2)
        out += unit[a:a + r.randrange(1000, len(unit) // 2)]
    return bytes(out[:mib << 20])


def noise(mib):
    return random.Random(18).randbytes(mib << 20)


def c2_like(mib):
    import streams as S
    _, plain = S.synth_lz4_stream(0x4C413335, 0, mib, blocks_per_frame=16, block_size=65536, nthreads=8)
    return plain.tobytes()


def raw_pieces(data, preset, piece):
    f = [{"id": lzma.FILTER_LZMA2, "preset": preset, "dict_size": 1 << 20}]
    return sum(len(lzma.compress(data[i:i + piece], format=lzma.FORMAT_RAW, filters=f)) for i in range(0, len(data), piece))


def filter_write(lib, path, level, cap):
    a = lib.archive_write_new()
    assert lib.archive_write_add_filter_xz(a) == 0 and lib.archive_write_set_format_raw(a) == 0
    assert lib.archive_write_set_filter_option(a, b"xz", b"compression-level", str(level).encode()) == 0
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
    ap.add_argument("--levels", default="0,6")
    ap.add_argument("--baseline-mib", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import _native as N
    from libarchive_amd import xz as X
    from test_gpu_lz4_write import _lib_setup
    lib = _lib_setup(la.host_lib())
    lib.archive_write_add_filter_xz.argtypes = [C.c_void_p]
    ctx = la.GpuContext(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    say("# tools/measure_xz_write.py --mib %d --levels %s --baseline-mib %d" % (args.mib, args.levels, args.baseline_mib))
    for name, gen in (("text", text_like), ("noise", noise), ("c2_like", c2_like)):
        plain = gen(args.mib)
        n = len(plain)
        sample = plain[:args.baseline_mib << 20]
        base = {}
        for preset in (0, 6):
            t = time.time()
            ref = lzma.compress(sample, preset=preset, check=lzma.CHECK_CRC64)
            dt = time.time() - t
            per_block = raw_pieces(sample, preset, 1 << 20)
            base[preset] = len(ref)
            say("%s: liblzma preset %d on one core: %.1f MiB/s, ratio %.3f as one stream, %.3f as raw LZMA2 per 1 MiB block (first %d MiB)"
                % (name, preset, len(sample) / 2 ** 20 / dt, len(sample) / len(ref), len(sample) / per_block, args.baseline_mib))
        a, b = raw_pieces(sample, 0, 1 << 20), raw_pieces(sample, 0, 1 << 16)
        say("%s: the state reset per 64 KiB: liblzma preset 0 per 64 KiB piece is %.4f of its size per 1 MiB block (%d / %d bytes)"
            % (name, b / a, b, a))
        d_src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
        for level in [int(x) for x in args.levels.split(",")]:
            cap = X.compress_bound(n, level)
            ws = int(N.gpu_lib().la_gpu_xz_compress_workspace_bytes(n))
            ctx.reserve(ws)
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_len = torch.zeros(1, dtype=torch.int64, device="cuda")
            bt = N._XzcBatchC()
            bt.d_src, bt.src_bytes, bt.level, bt.flags = d_src.data_ptr(), n, level, X.LA_XZC_FIRST
            bt.d_out, bt.out_cap, bt.d_out_bytes = d_out.data_ptr(), cap, d_len.data_ptr()
            ctx.xz_compress(bt)       # warm-up
            ctx.sync()
            total = int(d_len.cpu()[0])
            head = int(X.compress_window(ctx, d_src[:len(sample)], level).numel())
            say("%s level %d: %d MiB plain, %.2f MiB compressed (ratio %.3f), workspace %.0f MiB; first %d MiB: %.3f of preset 0, %.3f of preset 6"
                % (name, level, n >> 20, total / 2 ** 20, n / total, ws / 2 ** 20, args.baseline_mib, head / base[0], head / base[6]))
            ctx.profile_enable(True)
            times = []
            for _ in range(3):
                ctx.timer_start()
                ctx.xz_compress(bt)
                times.append(ctx.timer_stop())
            stages = ctx.profile_read()
            ctx.profile_enable(False)
            ms = sorted(times)[1]
            say("  one call, median of three: %.1f ms = %.0f MiB/s of input (%s)" % (ms, n / 2 ** 20 / (ms / 1e3), ", ".join("%.1f" % t for t in times)))
            say("  stages of the last call (ms): " + ", ".join("%s %.1f" % kv for kv in sorted(stages, key=lambda kv: -kv[1])))
            with tempfile.NamedTemporaryFile(suffix=".plain") as f:
                f.write(plain)
                f.flush()
                t = time.time()
                out = filter_write(lib, f.name, level, cap + 65536)
                dt = time.time() - t
            assert lzma.decompress(out) == plain
            say("  filter, file to memory: %.2f s = %.0f MiB/s of input (device open, pinned window, copies both ways included)"
                % (dt, n / 2 ** 20 / dt))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
