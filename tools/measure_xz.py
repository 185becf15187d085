"""xz read side on the device: la_gpu_xz_decode on blocks resident in HBM, checks verified, against liblzma (Python's
lzma) on one host core of the same machine on the same bytes.

    python tools/measure_xz.py [--mib 1024] [--unit 24] [--blocks 1,24] [--preset 6] [--reps 3] [--out FILE]

Two inputs, text-like (random words) and noise-like (random bytes), `unit` MiB each, cut into blocks of 1 MiB and of
24 MiB (what xz -6 -T writes), every block compressed as raw LZMA2 with a CRC64 behind it and tiled in HBM to `mib` MiB.
One la_gpu_xz_decode call takes the whole table.  One warm-up call, then `reps` calls timed with events on the
context's stream: the median is reported, and the per-kernel split of the last call.  Every status has to be OK and the
first and last tile's bytes are compared with the plain text on the device."""
import argparse
import lzma
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def text_like(n):
    r = np.random.RandomState(17)
    words = [bytes(r.randint(97, 123, size=2 + i % 9).astype(np.uint8)) + b" " for i in range(4000)]
    picks = r.randint(0, len(words), size=n // 5)
    return b"".join(words[i] for i in picks)[:n]


def noise_like(n):
    return np.random.RandomState(18).randint(0, 256, size=n).astype(np.uint8).tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=1024)
    ap.add_argument("--unit", type=int, default=24)
    ap.add_argument("--blocks", default="1,24")
    ap.add_argument("--preset", type=int, default=6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    import torch
    import libarchive_amd as la
    from libarchive_amd import xz as X
    import xz_build as XB
    say("# tools/measure_xz.py --mib %d --unit %d --blocks %s --preset %d --reps %d" % (args.mib, args.unit, args.blocks, args.preset, args.reps))
    tiles = max((args.mib + args.unit - 1) // args.unit, 1)
    filt = [{"id": lzma.FILTER_LZMA2, "preset": args.preset}]
    dict_size = lzma._decode_filter_properties(lzma.FILTER_LZMA2, lzma._encode_filter_properties(filt[0]))["dict_size"]
    for name, gen in (("text_like", text_like), ("noise_like", noise_like)):
        plain = gen(args.unit << 20)
        for bs in [int(x) << 20 for x in args.blocks.split(",")]:
            t = time.time()
            parts = [plain[i:i + bs] for i in range(0, len(plain), bs)]
            raws = [lzma.compress(p, format=lzma.FORMAT_RAW, filters=filt) for p in parts]
            t_comp = time.time() - t
            t = time.time()
            for p, r in zip(parts, raws):
                assert lzma.decompress(r, format=lzma.FORMAT_RAW, filters=filt) == p
            t_host = time.time() - t
            unit_img, unit_entries = b"", []
            dst = 0
            for p, r in zip(parts, raws):
                blob = r + bytes(-len(r) % 4) + struct.pack("<Q", XB.crc64(p))
                unit_entries.append((len(unit_img), len(r), len(p), dst))
                unit_img += blob
                dst += len(p)
            entries = [{"src_off": k * len(unit_img) + so, "comp_size": cs, "uncomp_size": us, "dst_off": k * len(plain) + do, "dst_cap": us,
                        "check_id": 4, "dict_size": dict_size} for k in range(tiles) for so, cs, us, do in unit_entries]
            total = tiles * len(plain)
            say("%s, blocks of %d MiB: %d MiB plain in %d blocks, %.1f MiB compressed (ratio %.2f); liblzma on one core: %.1f MiB/s decoded (compress %.1f s per unit)"
                % (name, bs >> 20, total >> 20, len(entries), tiles * len(unit_img) / 2 ** 20, len(plain) / len(unit_img), len(plain) / 2 ** 20 / t_host, t_comp))
            ctx = la.GpuContext(0)
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            ctx.profile_enable(True)
            d_unit = torch.from_numpy(np.frombuffer(unit_img, dtype=np.uint8).copy()).cuda()
            d_src = d_unit.repeat(tiles)
            d_plain = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
            plan = X.XzDevicePlan(ctx, d_src, X.block_table(entries), dst_cap=total)
            times = []
            for rep in range(args.reps + 1):    # the first call warms the workspace and the code objects
                ctx.timer_start()
                plan.run()
                ms = ctx.timer_stop()
                if rep:
                    times.append(ms)
            phases = dict(ctx.profile_read())
            res = plan.results()
            assert (res["status"] == 0).all(), res["status"][res["status"] != 0][:8]
            assert torch.equal(plan.d_dst[:len(plain)], d_plain) and torch.equal(plan.d_dst[total - len(plain):total], d_plain)
            med = statistics.median(times)
            say("  resident in HBM, checks verified: median of %d calls %.1f ms (min %.1f, max %.1f) = %.0f MiB/s decoded; last call: %s"
                % (len(times), med, min(times), max(times), total / 2 ** 20 / (med / 1e3), ", ".join("%s %.1f ms" % kv for kv in sorted(phases.items()))))
            ctx.close()
            del d_src, d_unit, d_plain, plan
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
