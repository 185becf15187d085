"""lzop read side on the device: la_gpu_lzop_decode on blocks resident in HBM, Adler-32 verified on both sides, and
la_gpu_adler32_many alone, against libarchive_amd/csrc/la_lzo_dev.h compiled -O2 on ONE host core of the same machine
over the same blocks.  That baseline is the project's own rules header; it is NOT liblzo2, which is not on the machine.

    python tools/measure_lzop.py [--mib 256] [--unit 4] [--blocks 256,64] [--reps 3] [--out FILE]

Two inputs, word text and the bench stream's kind of data (tests/streams.synth_lz4_stream's plain bytes), `unit` MiB
each, cut into blocks of 256 KiB (what lzop writes) and 64 KiB, every block compressed by tests/lzop_support.compress (a
greedy matcher: lzop -1's kind of stream, not its ratio) and kept stored where that does not shrink it, as lzop does; the
unit tiled in HBM to `mib` MiB.  One la_gpu_lzop_decode call takes the whole table.  One warm-up call, then `reps` calls
timed with events on the context's stream: the median is reported.  Every status has to be OK and the first and last
tile's bytes are compared with the plain text on the device."""
import argparse
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def inputs(mib):
    import deflate_find_support as F
    import streams as S
    n = mib << 20
    frames = max(1, n // (16 * 65536))
    synth = S.synth_lz4_stream(0x4C413335, 0, frames, blocks_per_frame=16, block_size=65536, nthreads=8)[1].tobytes()[:n]
    return (("word text", F.word_text(n, seed=41)), ("bench-stream data", synth))


def host_baseline(tmp, blocks, reps):
    """(bytes, seconds) of the rules header on one host core: best of `reps` passes over the unit's blocks"""
    import mock_build
    exe = mock_build.program("lzo_rules_bench")
    path = os.path.join(tmp, "blocks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blocks)))
        for comp, plain in blocks:
            f.write(struct.pack("<II", len(comp), len(plain)) + comp)
    out = subprocess.check_output([exe, path, str(reps)], text=True).split()
    return int(out[0]), float(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--unit", type=int, default=4)
    ap.add_argument("--blocks", default="256,64", help="block sizes in KiB")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import lzop
    import lzop_support as L
    say("# tools/measure_lzop.py --mib %d --unit %d --blocks %s --reps %d" % (args.mib, args.unit, args.blocks, args.reps))
    tiles = max((args.mib + args.unit - 1) // args.unit, 1)
    tmp = tempfile.mkdtemp(prefix="measure_lzop")
    for name, plain in inputs(args.unit):
        for bs in [int(x) << 10 for x in args.blocks.split(",")]:
            parts = [plain[i:i + bs] for i in range(0, len(plain), bs)]
            blocks = []
            for p in parts:
                c = L.compress(p)
                blocks.append((c if len(c) < len(p) else p, p))
            stored = sum(1 for c, p in blocks if len(c) == len(p))
            nbytes, secs = host_baseline(tmp, blocks, 3)
            unit_img, unit_entries, dst = b"", [], 0
            for c, p in blocks:
                unit_entries.append((len(unit_img), len(c), len(p), dst, zlib.adler32(c), zlib.adler32(p)))
                unit_img += c
                dst += len(p)
            entries = [{"src_off": k * len(unit_img) + so, "src_len": cl, "dst_off": k * len(plain) + do, "dst_len": ul,
                        "flags": lzop.C_ADLER32 | (lzop.U_ADLER32 if cl != ul else 0), "sum_c": sc, "sum_u": su}
                       for k in range(tiles) for so, cl, ul, do, sc, su in unit_entries]
            total = tiles * len(plain)
            say("%s, blocks of %d KiB: %d MiB plain in %d blocks (%d of a unit's %d stored), %.1f MiB compressed (ratio %.2f); "
                "la_lzo_dev.h -O2 on one host core (NOT liblzo2): %.0f MiB/s decoded"
                % (name, bs >> 10, total >> 20, len(entries), stored, len(blocks), tiles * len(unit_img) / 2 ** 20, len(plain) / len(unit_img),
                   nbytes / 2 ** 20 / secs))
            ctx = la.GpuContext(0)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            d_unit = torch.from_numpy(np.frombuffer(unit_img, dtype=np.uint8).copy()).cuda()
            d_src = d_unit.repeat(tiles)
            d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
            plan = lzop.LzopDevicePlan(ctx, d_src, lzop.block_table(entries), dst_cap=total)
            times = []
            for rep in range(args.reps + 1):    # the first call warms the workspace and the code objects
                ctx.timer_start()
                plan.run()
                t_ms = ctx.timer_stop()
                if rep:
                    times.append(t_ms)
            res = plan.results()
            assert (res["status"] == 0).all(), res["status"][res["status"] != 0][:8]
            assert torch.equal(plan.d_dst[:len(plain)], d_plain) and torch.equal(plan.d_dst[total - len(plain):total], d_plain)
            med = statistics.median(times)
            say("  resident in HBM, Adler-32 verified on both sides: median of %d calls %.2f ms (min %.2f, max %.2f) = %.0f MiB/s decoded"
                % (len(times), med, min(times), max(times), total / 2 ** 20 / (med / 1e3)))
            # the Adler-32 kernel alone, over the decoded bytes in ranges of the block size
            jobs = np.zeros(len(entries), dtype=la.HASH_JOB_DTYPE)
            jobs["off"] = [e["dst_off"] for e in entries]
            jobs["len"] = [e["dst_len"] for e in entries]
            jobs["seed"] = 1
            d_jobs = torch.from_numpy(jobs.view(np.uint8).reshape(-1).copy()).cuda()
            d_out = torch.zeros(len(entries), dtype=torch.int32, device="cuda")
            times = []
            for rep in range(args.reps + 1):
                ctx.timer_start()
                ctx.adler32_many(plan.d_dst.data_ptr(), d_jobs.data_ptr(), len(entries), d_out.data_ptr())
                t_ms = ctx.timer_stop()
                if rep:
                    times.append(t_ms)
            got = d_out.cpu().numpy().view(np.uint32)
            assert [int(g) for g in got[:len(blocks)]] == [zlib.adler32(p) for _, p in blocks]
            med = statistics.median(times)
            say("  la_gpu_adler32_many alone over the %d MiB: median %.2f ms = %.0f GiB/s" % (total >> 20, med, total / 2 ** 30 / (med / 1e3)))
            ctx.close()
            del d_src, d_unit, d_plain, plan, d_jobs, d_out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
